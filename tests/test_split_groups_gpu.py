"""Split kernel with a 16-lane group per node (csrc/bab.hip fa_split_group_kernel, networks with
2 n0 <= 32) against the one-wave-per-node kernel (FAIRIFY_SPLIT_GROUPS=0): native BaB solves give
exactly the same verdicts, node counts, open frontiers and counterexamples, and on small lattices the
verdicts of exhaustive enumeration."""
import itertools

import numpy as np
import pytest

from fairify_amd.engine import exact
from fairify_amd.engine.bab import SAT, UNSAT, BaBConfig, BaBSolver
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops.backend import Backend
from fairify_amd.spec import Domain, Feature, Query

pytestmark = pytest.mark.gpu

DOM = Domain("toy", tuple(Feature(f"f{i}", 0, w) for i, w in enumerate([3, 4, 2, 4, 5])))
HI = np.array([3, 4, 2, 4, 5])


def brute(m, q, lo, hi):
    pts = np.array(list(itertools.product(*[range(a, b + 1) for a, b in zip(lo, hi)])))
    s = dict(zip(map(tuple, pts), exact.exact_signs(m, pts)))
    for x in pts:
        rngs = []
        for i in range(len(lo)):
            if i in q.pa_idx:
                rngs.append([v for v in range(lo[i], hi[i] + 1) if v != x[i]])
            elif i in q.ra_idx:
                rngs.append(range(x[i] - q.tau, x[i] + q.tau + 1))
            else:
                rngs.append([x[i]])
        xps = np.array(list(itertools.product(*rngs)))
        if len(xps) and np.any(s[tuple(x)] * exact.exact_signs(m, xps) < 0):
            return SAT
    return UNSAT


def solve_both(monkeypatch, be, q, cfg, lo, hi, m):
    """The same solve with the grouped split kernel and with the one-wave-per-node kernel: equal."""
    res = {}
    for groups in ("1", "0"):
        monkeypatch.setenv("FAIRIFY_SPLIT_GROUPS", groups)
        res[groups] = BaBSolver(be, q, cfg).solve(lo, hi, m)
    a, b = res["1"], res["0"]
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.nodes, b.nodes)
    assert np.array_equal(a.open_left, b.open_left)
    assert np.array_equal(a.cex_x, b.cex_x)
    assert np.array_equal(a.cex_xp, b.cex_xp)
    return a


@pytest.mark.parametrize("hidden", [[5, 5], [16, 8]])
def test_split_groups_adult_budget_and_wide_first_levels(cuda, monkeypatch, hidden):
    """64 Adult partitions, split_target 256: one root per partition, so the first level splits along
    6 dims (64 children, four ballot rounds), the next ones along fewer; the small node budget stops
    part of the partitions (budget rule, open_left)."""
    from fairify_amd import presets
    from fairify_amd.partition import processing_order

    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    lo, hi = grid.decode(processing_order(grid, 0)[:64])
    m = random_mlp(13, hidden, seed=3, bias_scale=0.0)
    be = Backend(m, cuda)
    assert be.hip
    r = solve_both(monkeypatch, be, q, BaBConfig(node_budget=128, split_target=256), lo, hi, m)
    assert np.any(r.status == 0) and np.all(r.open_left[r.status == 0] > 0)     # some stopped on budget
    assert r.nodes.max() > 64                                                  # the 64-children level ran


@pytest.mark.parametrize("pa,ra,tau", [
    (("f2",), ("f3",), 1),          # relaxed: infeasible children, sparse feasibility masks, x' boxes
    (("f2", "f0"), (), 0),          # 12 PA values: 132 (orientation, pair) tests per leaf, 9 ballot rounds
])
def test_split_groups_lattice_matches_old_kernel_and_bruteforce(cuda, monkeypatch, pa, ra, tau):
    q = Query(pa=pa, ra=ra, tau=tau).resolve(DOM)
    lo = np.zeros(5, int)
    for seed in range(4):
        m = random_mlp(5, [6, 4], seed=200 + seed, bias_scale=1.0 if seed % 3 else 0.0)
        be = Backend(m, cuda)
        cfg = BaBConfig(node_budget=10 ** 6, batch_nodes=512, max_pool=1 << 16)
        r = solve_both(monkeypatch, be, q, cfg, lo[None], HI[None], m)
        assert r.status[0] == brute(m, q, lo, HI), seed
        if r.status[0] == SAT:
            assert exact.check_pair_constraints(r.cex_x, r.cex_xp, lo[None], HI[None], q.pa_idx, q.ra_idx, tau)[0]
            assert exact.is_violation(m, r.cex_x, r.cex_xp)[0]


def test_split_groups_wide_input_takes_the_fallback(cuda, monkeypatch):
    """n0 = 20 (40 scores > 32): the one-wave-per-node kernel whatever the switch says."""
    dom = Domain("toy20", tuple(Feature(f"g{i}", 0, 2) for i in range(20)))
    q = Query(pa=("g7",)).resolve(dom)
    free = [1, 7, 11, 19]                        # 3^4 lattice points per partition, the rest fixed
    g = np.random.default_rng(1)
    lo = g.integers(0, 3, size=(6, 20))
    hi = lo.copy()
    lo[:, free], hi[:, free] = 0, 2
    for seed in range(3):
        m = random_mlp(20, [8, 6], seed=900 + seed, bias_scale=0.5 if seed else 0.0)
        be = Backend(m, cuda)
        r = solve_both(monkeypatch, be, q, BaBConfig(node_budget=10 ** 6, batch_nodes=512, max_pool=1 << 16), lo, hi, m)
        for k in range(len(lo)):
            assert r.status[k] == brute(m, q, lo[k], hi[k]), (seed, k)
