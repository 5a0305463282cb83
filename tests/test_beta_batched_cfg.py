"""BetaConfig.batched / VerifyConfig.beta_batched (the two-phase beta level, csrc/beta_opt16.hip) on
the CPU tier: the flag is accepted and changes nothing on a CPU backend (the torch reference runs), and
FAIRIFY_BETA_BATCHED=1 sets the default."""
import os
import subprocess
import sys

import numpy as np

from fairify_amd import presets
from fairify_amd.engine.beta_bab import BetaBaBSolver, BetaConfig
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import processing_order


def test_batched_flag_is_a_no_op_on_cpu():
    """The setup of test_beta_bab.py::test_beta_bab_matches_bruteforce, seed 3: same verdicts, same
    witnesses, same node counts with the flag on and off."""
    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    ids = processing_order(grid, 0)[:24]
    lo, hi = grid.decode(ids)
    hi = np.minimum(hi, lo + 1)
    m = random_mlp(13, [8, 6, 4], seed=3, bias_scale=0.5)
    out = []
    for batched in (False, True):
        sol = BetaBaBSolver(Backend(m), q, BetaConfig(node_budget=256, iters=20, root_iters=40, branch="kernel",
                                                      batched=batched))
        res = sol.solve(lo, hi, m)
        assert sol.stats.get("batched") is False          # a CPU backend never takes the batched path
        out.append(res)
    assert np.array_equal(out[0].status, out[1].status)
    assert np.array_equal(out[0].cex_x, out[1].cex_x)
    assert np.array_equal(out[0].nodes, out[1].nodes)


def test_backend_accepts_batched_on_cpu():
    import inspect

    assert "batched" in inspect.signature(Backend.beta_level).parameters


def _defaults(env_value):
    env = {k: v for k, v in os.environ.items() if k != "FAIRIFY_BETA_BATCHED"}
    if env_value is not None:
        env["FAIRIFY_BETA_BATCHED"] = env_value
    code = ("from fairify_amd.engine.beta_bab import BetaConfig\n"
            "from fairify_amd.engine.pipeline import VerifyConfig\n"
            "print(int(BetaConfig().batched), int(VerifyConfig().beta_batched))\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr
    return r.stdout.split()[-2:]


def test_env_sets_the_default():
    """A fresh interpreter per setting (the default is read when the module is imported)."""
    assert _defaults(None) == ["0", "0"]
    assert _defaults("1") == ["1", "1"]
    assert _defaults("0") == ["0", "0"]
