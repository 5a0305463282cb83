"""The chunk-group state of the pipeline (engine/chunk_group.py): its merge and confirmation
operations against the inline blocks they replaced, and the node accounting of whole chunks."""
import numpy as np
import pytest

from fairify_amd import presets
from fairify_amd.engine import exact
from fairify_amd.engine.bab import RUNNING, SAT, UNKNOWN, UNSAT, BaBResult
from fairify_amd.engine.chunk_group import GroupState
from fairify_amd.engine.pipeline import VerifyConfig, verify_chunk
from fairify_amd.models.mlp import MLP
from fairify_amd.models.zoo import get_model
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import processing_order
from fairify_amd.spec import Domain, Feature, ResolvedQuery
from fairify_amd.utils import faults

# f1 is the protected attribute; logit = f1 - (1 - f1) + 2 relu(f0 - 3): flips with f1 where f0 <= 3
DOM = Domain("toy", (Feature("f0", 0, 4), Feature("f1", 0, 1), Feature("f2", 0, 4)))
Q = ResolvedQuery(domain=DOM, pa_idx=(1,), ra_idx=(), tau=0)
NET = MLP([np.array([[0, 0, 1], [1, -1, 0], [0, 0, 0]], np.float32), np.array([[1], [-1], [2]], np.float32)],
          [np.array([0, 1, -3], np.float32), np.zeros(1, np.float32)], name="toy")


def _state(P):
    lo = np.tile(DOM.lo(), (P, 1))
    hi = np.tile(np.array([f.hi for f in DOM.features], dtype=np.int64), (P, 1))
    return GroupState(Backend(NET), NET, Q, np.arange(P, dtype=np.int64), lo, hi)


@pytest.mark.parametrize("open_left", [False, True])
def test_absorb_matches_the_inline_merge(open_left):
    """absorb against the block the escalation, relu, beta, anytime and heuristic stages spelled
    out: decided rows, their stage, SAT witnesses, the nodes of the whole subset, and -- only when
    asked, as only the escalation did -- the frontier sizes, from a copy."""
    rng = np.random.default_rng(3)
    s = _state(10)
    s.status[:] = [UNKNOWN, UNKNOWN, SAT, UNKNOWN, UNKNOWN, UNSAT, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN]
    s.stage[[2, 5]] = "sim", "bab"
    s.cex_x[:] = rng.integers(0, 5, size=(10, 3))
    s.cex_xp[:] = rng.integers(0, 5, size=(10, 3))
    s.nodes[:] = rng.integers(1, 50, size=10)
    s.open_left = first_open = rng.integers(1, 9, size=10)
    idx = np.array([1, 3, 4, 6, 8, 9])
    res = BaBResult(status=np.array([SAT, UNSAT, UNKNOWN, SAT, RUNNING, UNSAT], dtype=np.int8),
                    cex_x=100 + np.arange(18).reshape(6, 3), cex_xp=200 + np.arange(18).reshape(6, 3),
                    nodes=np.array([7, 11, 13, 17, 19, 23]), open_left=np.array([0, 0, 31, 0, 37, 0]))
    status, stage, cex_x, cex_xp = s.status.copy(), s.stage.copy(), s.cex_x.copy(), s.cex_xp.copy()
    nodes, open_before = s.nodes.copy(), first_open.copy()
    # the inline block (escalate(), with the names of the parent commit)
    unk, eres = idx, res
    dec_e = np.isin(eres.status, (SAT, UNSAT))
    hit = unk[dec_e]
    status[hit] = eres.status[dec_e]
    stage[hit] = "relu"
    es = eres.status == SAT
    cex_x[unk[es]] = eres.cex_x[es]
    cex_xp[unk[es]] = eres.cex_xp[es]
    nodes[unk] += eres.nodes
    want_open = open_before.copy()
    if open_left:
        want_open[unk] = eres.open_left

    assert s.absorb(idx, res, "relu", open_left=open_left) == int(dec_e.sum()) == 4
    for got, want in ((s.status, status), (s.stage, stage), (s.cex_x, cex_x), (s.cex_xp, cex_xp), (s.nodes, nodes),
                      (s.open_left, want_open)):
        assert np.array_equal(got, want)
    assert np.array_equal(first_open, open_before)            # the first pass's array is not written
    rest = np.setdiff1d(np.arange(10), idx)
    assert s.status[rest].tolist() == [UNKNOWN, SAT, UNSAT, UNKNOWN] and s.stage[rest].tolist() == ["", "sim", "bab", ""]
    assert s.status[[4, 8]].tolist() == [UNKNOWN, UNKNOWN] and s.stage[[4, 8]].tolist() == ["", ""]
    assert np.array_equal(s.cex_x[[1, 6]], res.cex_x[[0, 3]]) and np.array_equal(s.cex_x[3], cex_x[3])
    # a result without frontier sizes (the PyTorch loop) leaves them alone
    s.absorb(idx[:1], BaBResult(res.status[:1], res.cex_x[:1], res.cex_xp[:1], res.nodes[:1]), "bab", open_left=True)
    assert np.array_equal(s.open_left, want_open)


def test_confirm_writes_only_exact_violations_inside_the_box():
    s = _state(4)
    s.status[:] = UNKNOWN
    X = np.array([[1, 0, 2], [1, 0, 2], [4, 0, 2]]) + np.array([[0.2, -0.2, 0.1]])
    XP = np.array([[1, 1, 2],        # flips the sign, admissible
                   [1, 1, 3],        # flips the sign, but a shared coordinate differs
                   [4, 1, 2]])       # admissible, both logits positive
    assert exact.is_violation(NET, X.round().astype(np.int64), XP).tolist() == [True, True, False]
    hit = s.confirm(np.array([0, 1, 2]), X.astype(np.float32), XP.astype(np.float32), "falsify")
    assert hit.tolist() == [0]
    assert s.status.tolist() == [SAT, UNKNOWN, UNKNOWN, UNKNOWN] and s.stage.tolist() == ["falsify", "", "", ""]
    assert s.cex_x[0].tolist() == [1, 0, 2] and s.cex_xp[0].tolist() == [1, 1, 2] and s.cex_x.dtype == np.int64
    assert not s.cex_x[1:].any() and not s.cex_xp[1:].any()
    # x outside the partition's box is no witness of that partition
    s.lo_np[3, 0] = 2
    assert s.confirm(np.array([3]), X[:1], XP[:1].astype(np.float64), "sim").size == 0 and s.status[3] == UNKNOWN
    # none of the five replaced sites could meet a decided partition (the simulation's rows are all
    # RUNNING, the others pass UNKNOWN rows only) and each wrote unconditionally: so does confirm
    s.confirm(np.array([0]), np.array([[2, 1, 0]]), np.array([[2, 0, 0]]), "milp")
    assert s.cex_x[0].tolist() == [2, 1, 0] and s.cex_xp[0].tolist() == [2, 0, 0] and s.stage[0] == "milp"


def test_unknown_excludes_forced_partitions_unless_asked():
    s = _state(5)
    s.status[:] = [UNKNOWN, SAT, UNKNOWN, UNSAT, UNKNOWN]
    s.forced[[2, 3]] = True
    assert s.unknown().tolist() == [0, 4] and s.unknown(with_forced=True).tolist() == [0, 2, 4]


def test_charging_adds_the_node_delta_of_its_block_to_one_column():
    s = _state(3)
    s.nodes[:] = [5, 6, 7]
    with s.charging(1):
        s.nodes[[0, 2]] += [10, 30]
    with s.charging(1), s.charging(4):
        s.nodes[1] += 2
    assert s.stage_nodes.tolist() == [[0, 10, 0, 0, 0], [0, 2, 0, 0, 2], [0, 30, 0, 0, 0]]


@pytest.fixture(scope="module")
def ac8():
    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    m = get_model("AC-8", weights="random", seed=0)
    ids = processing_order(grid, 0)[:64]
    return Backend(m), m, q, grid, ids, grid.decode(ids)


def _check_accounting(setup, cfg):
    be, m, q, grid, ids, (lo, hi) = setup
    c = verify_chunk(be, m, q, grid, ids, cfg).core
    assert np.array_equal(c["stage_nodes"].sum(axis=1), c["nodes"])
    sat = np.nonzero(c["verdict"] == "sat")[0]
    X, XP = c["cex_x"][sat], c["cex_xp"][sat]
    assert exact.check_pair_constraints(X, XP, lo[sat], hi[sat], q.pa_idx, q.ra_idx, q.tau).all()
    sound = c["stage"][sat] != "heuristic"
    assert exact.is_violation(m, X[sound], XP[sound]).all()
    return c


BASE = dict(sim_size=128, smt_backend="none")


def test_node_accounting_relu_first_with_masks_and_metrics(ac8):
    c = _check_accounting(ac8, VerifyConfig(node_budget=16, escalate_budget=256, relu_budget=128, residual_samples=256,
                                            heuristic=True, keep_masks=True, pruned_metrics=True, **BASE))
    assert {"bab", "relu"} <= set(c["stage"])


def test_node_accounting_escalation_stages_and_beta(ac8):
    c = _check_accounting(ac8, VerifyConfig(node_budget=16, escalate_budget=64, escalate_stages=((256, 0),),
                                            relu_budget=0, beta_budget=64, beta_min_width=1, residual_samples=0,
                                            heuristic=True, heuristic_node_budget=16, **BASE))
    assert {"bab", "beta"} <= set(c["stage"])


def test_node_accounting_with_forced_unknowns_reaching_the_heuristic(ac8, monkeypatch):
    """Fault-injected partitions (forced UNKNOWN after the first pass) are skipped by the sound residue
    stages but not by the heuristic retry: the asymmetry docs/DESIGN.md lists is pinned here."""
    be, m, q, grid, ids, _ = ac8
    cfg = VerifyConfig(node_budget=64, relu_budget=64, residual_samples=256, heuristic=True, **BASE)
    clean = verify_chunk(be, m, q, grid, ids, cfg).core      # no escalation: "bab" = the first pass
    monkeypatch.setenv("FAIRIFY_FAULT_FORCE_UNKNOWN", "0.5")
    forced = faults.forced_unknown(ids) & (clean["stage"] == "bab")
    c = _check_accounting(ac8, cfg)
    assert forced.any() and (c["stage"][forced] == "heuristic").any()
    assert not np.isin(c["stage"][forced], ("relu", "bab", "beta")).any()
