"""bench.py self-launch: ``--gpus N`` starts N ranks itself (gloo on CPU here, RCCL on GPUs) and
the verdict totals of the strong-scaling step do not depend on N."""
import json
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(gpus: int, extra=()):
    env = dict(os.environ, FAIRIFY_DIST_BACKEND="gloo", FAIRIFY_CPU_THREADS="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--device", "cpu",
           "--models", "AC-8,AC-9", "--limit", "48", "--chunk", "16", "--steps", "1", "--warmup", "1", "--unit", "4",
           "--budget-pass", "0", "--escalate-budget", "4096", *extra]   # CPU: the torch BaB path
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # only rank 0 prints
    return json.loads(lines[0])


def test_self_launch_totals_match_one_rank():
    """Totals do not depend on the rank count, and the LPT unit assignment of the timed step
    (previous step's node counts, weighted by each model's multiply-adds) keeps every rank's cost
    within LPT's bound (mean + largest unit) -- within 10 % of the mean at 2 ranks."""
    one = _bench(1)
    assert one["n_gpus"] == 1 and one["dist"]["backend"] == "none"
    for n in (2, 4, 8):
        d = _bench(n)
        assert d["n_gpus"] == n and d["dist"]["world"] == n and d["dist"]["backend"] == "gloo"
        assert len(d["dist"]["rank_ms_per_step"]) == n
        assert d["config"]["parallelism"] == f"dp{n}"
        for k in ("sat", "unsat", "unknown", "unsat_sound", "unsat_heuristic"):
            assert d[k] == one[k], (n, k)
        assert d["sat_by_stage"] == one["sat_by_stage"]
        dd = d["dist"]
        # LPT's guarantee (mean + largest unit); at 2 ranks the 24 units balance within 10 %.  At 4 / 8
        # ranks a single heavy unit (a partition escalated after the relu stage) dominates 3-6 units
        # per rank, so only the guarantee is asserted there
        assert dd["balance"] == "lpt" and dd["predicted_cost_ratio"] <= (
            min(dd["predicted_cost_bound"], 1.1) if n == 2 else dd["predicted_cost_bound"]), dd
    # every key the bench docstring names is emitted
    import re

    src = open(os.path.join(ROOT, "bench.py")).read()
    doc = src.split('"""')[1]
    para = doc.split("JSON keys")[1].split(":", 1)[1].split("\n\n")[0]
    names = re.findall(r"[a-z_]+", para)
    assert len(names) >= 20, names
    missing = [k for k in names if k not in one]
    assert not missing, missing
    # honest accounting fields add up
    assert one["unsat_sound"] + one["unsat_heuristic"] == one["unsat"]
    # per-model residue and stage node counts (per timed step) add up to the totals
    pm = one["per_model"]
    assert set(pm) == {"AC-8", "AC-9"}
    assert sum(v["attempted"] for v in pm.values()) == one["sat"] + one["unsat"] + one["unknown"]
    assert abs(sum(v["unknown"] for v in pm.values()) - one["unknown"]) < 1e-6
    sound_dec = one["sat"] - one["sat_by_stage"]["heuristic"] + one["unsat_sound"]
    assert abs(sum(v["unknown_sound"] for v in pm.values()) - (pm["AC-8"]["attempted"] + pm["AC-9"]["attempted"]
                                                               - sound_dec)) < 1e-6
    assert all(set(v["nodes"]) == {"bab", "relu", "beta", "anytime", "heuristic"} for v in pm.values())
    assert sum(v["nodes"]["bab"] for v in pm.values()) > 0
    assert "cross-regime" in one["vs_baseline_note"]
    assert sum(one["sat_by_stage"].values()) == one["sat"]


def test_bench_refuses_reference_fallback():
    env = dict(os.environ, FAIRIFY_FORCE_REFERENCE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--steps", "1"],
                       capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "FAIRIFY_FORCE_REFERENCE" in r.stderr


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device", "cpu",
                        "--steps", "1"], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_sound_fields_exclude_heuristic_and_milp():
    """pct_verified_sound / unsat_sound = decided minus heuristic-retry verdicts minus MILP UNSAT
    (a trusted HiGHS dual bound is still no proof), on a small run where both stages fire."""
    d = _bench(1, ("--models", "AC-8", "--node-budget", "8", "--escalate-budget", "0", "--smt", "milp",
                   "--trust-milp", "--relu-budget", "0"))
    att = d["sat"] + d["unsat"] + d["unknown"]
    us = d["unsat_by_stage"]
    assert sum(us.values()) == d["unsat"] and sum(d["sat_by_stage"].values()) == d["sat"]
    assert us["milp"] > 0, us                     # the test exercises the MILP stage
    assert d["unsat_sound"] == d["unsat"] - us["milp"] - us["heuristic"]
    sound = d["sat"] + d["unsat"] - us["milp"] - us["heuristic"] - d["sat_by_stage"]["heuristic"]
    assert abs(d["pct_verified_sound"] - round(100.0 * sound / att, 3)) < 1e-9
    # the headline value is the SOUND decided rate (heuristic / MILP verdicts excluded); the
    # all-verdict rate is the secondary field
    wall = d["ms_per_step"] * d["steps"] / 1000.0
    assert abs(d["value"] - sound / wall) <= 1e-3 * max(1.0, d["value"]), (d["value"], sound, wall)
    assert abs(d["decided_per_s_all"] - (d["sat"] + d["unsat"]) / wall) <= 1e-3 * max(1.0, d["decided_per_s_all"])
    assert d["value"] < d["decided_per_s_all"]
    # default: an untrusted MILP 'unsat' is no verdict (MILP stage: --lp-budget 0) ...
    d2 = _bench(1, ("--models", "AC-8", "--node-budget", "8", "--escalate-budget", "0", "--smt", "milp",
                    "--relu-budget", "0", "--lp-budget", "0"))
    assert d2["unsat_by_stage"]["milp"] == 0
    assert d2["unsat"] + d2["unknown"] >= d["unsat"] + d["unknown"] - 1e-9
    # ... and the verified-LP stage's UNSAT (rigorous dual certificates) counts as sound
    d3 = _bench(1, ("--models", "AC-8", "--limit", "16", "--node-budget", "8", "--escalate-budget", "0",
                    "--smt", "milp", "--relu-budget", "0", "--lp-budget", "64"))
    us3 = d3["unsat_by_stage"]
    assert us3["milp"] == 0 and us3["lp"] > 0, us3
    assert d3["unsat_sound"] == d3["unsat"] - us3["heuristic"]


def test_budget_pass_only_with_full():
    """A plain run stops after the timed steps; the untimed budget pass and its fields need --full."""
    small = ("--models", "AC-8", "--limit", "16", "--budget-pass", "0.5")
    plain = _bench(1, small)
    assert not {"budget_pass", "pct_verified_at_budget", "pct_verified_at_budget_sound"} & set(plain)
    full = _bench(1, small + ("--full",))
    assert full["budget_pass"]["attempted"] == 16 and full["budget_pass"]["seconds_per_model"] == 0.5
    assert 0.0 <= full["pct_verified_at_budget_sound"] <= full["pct_verified_at_budget"] <= 100.0
    for k in ("sat", "unsat", "unknown", "sat_by_stage", "unsat_by_stage", "steps", "warmup"):
        assert full[k] == plain[k], k


def test_dump_outputs_last_step_records(tmp_path):
    """--dump-outputs: one .npy per record column of the last timed step, float32 / float64, rows by
    (model, grid id), consistent with the JSON totals and identical from run to run."""
    import numpy as np

    runs = []
    for name, steps in (("a", "1"), ("b", "2")):
        d = _bench(1, ("--dump-outputs", str(tmp_path / name), "--steps", steps, "--limit", "16"))
        assert d["steps"] == int(steps)
        runs.append((d, {f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}))
    (da, a), (db, b) = runs
    assert set(a) == set(b) >= {"model", "grid_id", "verdict", "stage", "nodes", "stage_nodes", "agree", "cex_x",
                                "cex_xp"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and len(a[k]) == 32, k
        assert np.array_equal(a[k], b[k]), k          # the last step only, whatever --steps is
    assert a["cex_x"].shape == (32, 13) and a["stage_nodes"].shape == (32, 5)
    assert a["model"].tolist() == [0.0] * 16 + [1.0] * 16
    assert all((np.diff(a["grid_id"][a["model"] == m]) > 0).all() for m in (0, 1))
    assert ((a["verdict"] == 1).sum(), (a["verdict"] == 2).sum(), (a["verdict"] == 0).sum()) == \
        (da["sat"], da["unsat"], da["unknown"])
    assert 2 * da["sat"] == db["sat"]                  # the JSON totals cover every timed step
    sat = a["verdict"] == 1
    assert (a["cex_x"][~sat] == 0).all() and (a["cex_x"][sat] != a["cex_xp"][sat]).any(axis=1).all()
    for i, col in enumerate(("bab", "relu", "beta", "anytime", "heuristic")):
        assert a["stage_nodes"][:, i].sum() == sum(m["nodes"][col] for m in da["per_model"].values()), col


def test_emulated_lpt_shards_cover_the_grid():
    """--emulate-shard r/N with the LPT balancer: the warmup step measures every unit, the timed
    step runs rank r's units; the N emulated shards partition the grid (attempted and decided
    totals add up to the one-rank run) and their assigned costs are balanced."""
    one = _bench(1)
    tot = {"sat": 0, "unsat": 0, "unknown": 0}
    for r in range(4):
        d = _bench(1, ("--emulate-shard", f"{r}/4"))
        dd = d["dist"]
        assert dd["balance"] == "lpt" and dd["predicted_cost_ratio"] <= dd["predicted_cost_bound"], dd
        for k in tot:
            tot[k] += d[k]
    for k in tot:
        assert tot[k] == one[k], (k, tot, one)
