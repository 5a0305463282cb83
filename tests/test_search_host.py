"""The host layer the three Python BaB solvers share (engine/search.py): each helper against the
inline block it replaced (copied from the solvers as they were before the split), and the
``max_pool`` truncation of each solver's torch loop end to end against brute force."""
import itertools
import time

import numpy as np
import pytest
import torch

from fairify_amd.engine import exact, search
from fairify_amd.engine.bab import BaBConfig, BaBSolver
from fairify_amd.engine.beta_bab import BetaBaBSolver, BetaConfig
from fairify_amd.engine.relu_bab import ReluBaBSolver, ReluConfig
from fairify_amd.engine.search import RUNNING, SAT, UNKNOWN, UNSAT, BaBResult, Verdicts
from fairify_amd.models.mlp import MLP, random_mlp
from fairify_amd.ops.backend import Backend
from fairify_amd.spec import Domain, Feature, Query, ResolvedQuery

# f1 is the protected attribute; logit = f1 - (1 - f1) + 2 relu(f0 - 3): flips with f1 where f0 <= 3
DOM = Domain("toy", (Feature("f0", 0, 4), Feature("f1", 0, 1), Feature("f2", 0, 4)))
Q = ResolvedQuery(domain=DOM, pa_idx=(1,), ra_idx=(), tau=0)
NET = MLP([np.array([[0, 0, 1], [1, -1, 0], [0, 0, 0]], np.float32), np.array([[1], [-1], [2]], np.float32)],
          [np.array([0, 1, -3], np.float32), np.zeros(1, np.float32)], name="toy")
FLAT = MLP([np.zeros((3, 3), np.float32), np.zeros((3, 1), np.float32)],
           [np.zeros(3, np.float32), np.zeros(1, np.float32)], name="flat")       # logit 0: never a violation


def _boxes(P):
    return np.tile(DOM.lo(), (P, 1)), np.tile(np.array([f.hi for f in DOM.features], dtype=np.int64), (P, 1))


# ------------------------------------------------------------------------------------------ confirmer
def _old_confirm_given_order(parts, X, XP, status, cex_x, cex_xp, mlp_exact, exact_models, lo_np, hi_np, q):
    """BaBSolver._confirm (without its device mirror): candidates in the order given."""
    ok = exact.check_pair_constraints(X, XP, lo_np[parts], hi_np[parts], q.pa_idx, q.ra_idx, q.tau)
    if exact_models is None:
        viol = exact.is_violation(mlp_exact, X, XP) & ok
    else:
        viol = np.zeros(len(parts), dtype=bool)
        for k, p in enumerate(parts):
            if ok[k]:
                viol[k] = exact.is_violation(exact_models[p], X[k:k + 1], XP[k:k + 1])[0]
    newly = []
    for k in np.nonzero(viol)[0]:
        p = parts[k]
        if status[p] != SAT:
            status[p] = SAT
            cex_x[p] = X[k]
            cex_xp[p] = XP[k]
            newly.append(p)
    return newly


def _old_confirm_lex_order(parts, X, XP, status, cex_x, cex_xp, mlp_exact, lo_np, hi_np, q):
    """ReluBaBSolver._confirm / BetaBaBSolver._confirm (they were identical)."""
    ok = exact.check_pair_constraints(X, XP, lo_np[parts], hi_np[parts], q.pa_idx, q.ra_idx, q.tau)
    viol = exact.is_violation(mlp_exact, X, XP) & ok
    order = np.lexsort(tuple(np.concatenate([X, XP], axis=1).T[::-1]) + (parts,))
    for k in order:
        p = parts[k]
        if viol[k] and status[p] != SAT:
            status[p] = SAT
            cex_x[p], cex_xp[p] = X[k], XP[k]


CAND_PARTS = np.array([2, 0, 0, 1, 3, 0, 4])
CAND_X = np.array([[2, 0, 1], [3, 0, 2], [1, 0, 0], [1, 0, 1], [4, 0, 1], [0, 0, 0], [2, 1, 3]])
CAND_XP = np.array([[2, 1, 1],      # partition 2: a true pair, but the partition is SAT already
                    [3, 1, 2],      # partition 0: a true pair, first in the order given
                    [1, 1, 0],      # partition 0: a true pair, first in lexicographic order
                    [1, 1, 1],      # partition 1: a true pair outside its box (lo[1, 0] = 2)
                    [4, 1, 1],      # partition 3: admissible, both logits positive
                    [0, 1, 1],      # partition 0: a shared coordinate differs
                    [2, 0, 3]])     # partition 4: a true pair


@pytest.mark.parametrize("lex_order", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_confirm_pairs_matches_the_inline_confirmers(lex_order, masked):
    P = 5
    lo, hi = _boxes(P)
    lo[1, 0] = 2
    v = Verdicts(P, 3, np.array([RUNNING, RUNNING, SAT, RUNNING, UNKNOWN], np.int8))
    v.cex_x[2], v.cex_xp[2] = [9, 9, 9], [8, 8, 8]
    status, cex_x, cex_xp = v.status.copy(), v.cex_x.copy(), v.cex_xp.copy()
    models = [NET, NET, NET, NET, FLAT] if masked else None       # partition 4's masked net never flips
    # candidates arrive as float tensors a little off the lattice
    xa = torch.from_numpy(CAND_X + 0.2).float()
    xb = torch.from_numpy(CAND_XP - 0.3).float()
    want_new = None
    if not lex_order:
        want_new = _old_confirm_given_order(CAND_PARTS, CAND_X, CAND_XP, status, cex_x, cex_xp, NET, models, lo, hi, Q)
    elif not masked:
        _old_confirm_lex_order(CAND_PARTS, CAND_X, CAND_XP, status, cex_x, cex_xp, NET, lo, hi, Q)
    newly = search.confirm_pairs(v, Q, lo, hi, NET, CAND_PARTS, xa, xb, exact_models=models, lex_order=lex_order)
    if not (masked and lex_order):      # (relu and beta never passed masked nets: no inline block to compare with)
        assert np.array_equal(v.status, status) and np.array_equal(v.cex_x, cex_x) and np.array_equal(v.cex_xp, cex_xp)
    if want_new is not None:
        assert [int(p) for p in newly] == [int(p) for p in want_new]
    # which candidate wins, what is rejected
    assert v.cex_x[0].tolist() == ([1, 0, 0] if lex_order else [3, 0, 2])
    assert v.status.tolist() == [SAT, RUNNING, SAT, RUNNING, UNKNOWN if masked else SAT]
    assert v.cex_x[2].tolist() == [9, 9, 9] and 2 not in newly
    assert sorted(int(p) for p in newly) == ([0] if masked else [0, 4])


# ------------------------------------------------------------------------------------------ group scatter
def _mixed_boxes():
    lo, hi = _boxes(6)
    hi[[1, 4], 1] = 0            # PA range [0, 0]: a second group, its rows not contiguous
    lo[5, 1] = 1                 # PA range [1, 1]: a third
    return lo, hi


def _old_bab_solve_groups(self, groups, lo_np, hi_np, mlp_exact, init_status, exact_models, t0):
    """BaBSolver._solve_groups as it was."""
    from dataclasses import replace

    P, n = lo_np.shape
    status = np.full(P, RUNNING, dtype=np.int8) if init_status is None else init_status.astype(np.int8).copy()
    cex_x = np.zeros((P, n), dtype=np.int64)
    cex_xp = np.zeros((P, n), dtype=np.int64)
    nodes = np.zeros(P, dtype=np.int64)
    open_left = np.zeros(P, dtype=np.int64)
    iters = 0
    dead_all = self.dead
    for g in groups:
        sub = BaBSolver(self.be, self.q, replace(self.cfg, time_budget=max(0.0, self.cfg.time_budget -
                                                                              (time.time() - t0))),
                        dead=None if dead_all is None else dead_all[torch.from_numpy(g).to(dead_all.device)],
                        timer=self.tm)
        em = None if exact_models is None else [exact_models[int(k)] for k in g]
        r = sub.solve(lo_np[g], hi_np[g], mlp_exact, init_status=status[g], exact_models=em)
        status[g], cex_x[g], cex_xp[g], nodes[g] = r.status, r.cex_x, r.cex_xp, r.nodes
        if r.open_left is not None:
            open_left[g] = r.open_left
        iters += r.iters
    return BaBResult(status, cex_x, cex_xp, nodes, iters, time.time() - t0, open_left=open_left)


def _fake_group_result(lo_g, status_g, with_open):
    """A synthetic group result that depends on the rows it was given."""
    st = np.where(status_g == RUNNING, np.where(lo_g[:, 1] == 1, UNKNOWN, UNSAT), status_g).astype(np.int8)
    return BaBResult(st, lo_g * 10 + 1, lo_g * 10 + 2, lo_g.sum(1) + 5, iters=3,
                     open_left=(np.arange(len(lo_g)) + 7) if with_open else None)


@pytest.mark.parametrize("with_init", [False, True])
def test_bab_group_scatter_hands_each_group_its_rows(monkeypatch, with_init):
    lo, hi = _mixed_boxes()
    groups = search.pa_groups(Q, lo, hi)
    assert sorted(len(g) for g in groups) == [1, 2, 3]
    init = np.array([RUNNING, SAT, RUNNING, UNKNOWN, RUNNING, UNSAT], np.int8) if with_init else None
    dead = (torch.arange(6)[:, None] >> torch.arange(3)[None, :]) % 2 == 1        # row p: the bits of p
    models = [MLP(NET.weights, NET.biases, name=f"m{p}") for p in range(6)]
    seen = []

    def fake_solve(self, lo_g, hi_g, mlp_exact, init_status=None, exact_models=None):
        seen.append((lo_g.copy(), self.dead.clone(), [m.name for m in exact_models], init_status.copy(),
                     self.cfg.time_budget))
        return _fake_group_result(lo_g, init_status, with_open=len(lo_g) != 2)     # one group reports none

    monkeypatch.setattr(BaBSolver, "solve", fake_solve)
    solver = BaBSolver(Backend(NET), Q, BaBConfig(time_budget=50.0), dead=dead)
    want = _old_bab_solve_groups(solver, groups, lo, hi, NET, init, models, time.time())
    old_calls, seen[:] = list(seen), []
    got = solver._solve_groups(groups, lo, hi, NET, init, models, time.time())
    for k in ("status", "cex_x", "cex_xp", "nodes", "iters", "open_left"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert got.iters == 9 and got.open_left.dtype == np.int64
    two = [g for g in groups if len(g) == 2][0]
    assert not got.open_left[two].any() and got.open_left[np.setdiff1d(np.arange(6), two)].all()
    status0 = np.full(6, RUNNING, np.int8) if init is None else init
    for g, new, old in zip(groups, seen, old_calls):
        assert np.array_equal(new[0], lo[g]) and torch.equal(new[1], dead[torch.from_numpy(g)])
        assert new[2] == [f"m{int(p)}" for p in g] and np.array_equal(new[3], status0[g])
        assert 49.0 < new[4] <= 50.0            # the group's remaining time
        assert np.array_equal(new[0], old[0]) and torch.equal(new[1], old[1]) and new[2] == old[2]
    if with_init:
        assert got.status[[1, 3, 5]].tolist() == [SAT, UNKNOWN, UNSAT]


def test_group_scatter_without_open_left_and_with_no_time_left():
    """Relu and beta: ``open_left`` stays None, ``iters`` 0; against ReluBaBSolver._solve_groups_all as it was."""
    lo, hi = _mixed_boxes()
    groups = search.pa_groups(Q, lo, hi)
    init = np.array([RUNNING, SAT, RUNNING, UNKNOWN, RUNNING, RUNNING], np.int8)
    lefts = []

    def group(g, status_g, left):
        lefts.append(left)
        r = _fake_group_result(lo[g], status_g, with_open=False)
        r.iters = 0
        return r

    got = search.solve_pa_groups(groups, lo, hi, init, 0.0, time.time() - 1.0, group)
    # the inline loop
    P, n = lo.shape
    status = init.copy()
    cex_x = np.zeros((P, n), dtype=np.int64)
    cex_xp = np.zeros((P, n), dtype=np.int64)
    nodes = np.zeros(P, dtype=np.int64)
    for g in groups:
        r = _fake_group_result(lo[g], status[g], with_open=False)
        status[g], cex_x[g], cex_xp[g], nodes[g] = r.status, r.cex_x, r.cex_xp, r.nodes
    assert np.array_equal(got.status, status) and np.array_equal(got.cex_x, cex_x)
    assert np.array_equal(got.cex_xp, cex_xp) and np.array_equal(got.nodes, nodes)
    assert got.open_left is None and got.iters == 0 and lefts == [0.0, 0.0, 0.0]
    assert np.array_equal(init, [RUNNING, SAT, RUNNING, UNKNOWN, RUNNING, RUNNING])     # the caller's array: unwritten


# ------------------------------------------------------------------------------------------ orientation merge
def test_merge_orientations_matches_the_inline_merge():
    status = np.array([RUNNING, RUNNING, RUNNING, RUNNING, SAT, UNSAT, RUNNING], np.int8)
    r1 = BaBResult(np.array([UNSAT, UNSAT, SAT, UNKNOWN, SAT, UNSAT, UNSAT], np.int8),
                   np.arange(21).reshape(7, 3), 100 + np.arange(21).reshape(7, 3), np.array([1, 2, 3, 4, 0, 0, 5]))
    r2 = BaBResult(np.array([UNSAT, SAT, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN], np.int8),
                   200 + np.arange(21).reshape(7, 3), 300 + np.arange(21).reshape(7, 3),
                   np.array([10, 20, 0, 0, 0, 0, 30]))
    asked = []

    def second(st2):
        asked.append(st2)
        return r2

    got = search.merge_orientations(r1, status, second, time.time())
    # the inline block (ReluBaBSolver.solve / BetaBaBSolver.solve)
    closed = (r1.status == UNSAT) & (status == RUNNING)
    st2 = np.where(closed, RUNNING, UNKNOWN).astype(np.int8)
    out = r1.status.copy()
    out[closed] = r2.status[closed]
    cx, cxp = r1.cex_x.copy(), r1.cex_xp.copy()
    s2 = closed & (r2.status == SAT)
    cx[s2], cxp[s2] = r2.cex_x[s2], r2.cex_xp[s2]
    assert np.array_equal(asked[0], st2) and asked[0].dtype == np.int8 and closed.tolist() == [1, 1, 0, 0, 0, 0, 1]
    assert np.array_equal(got.status, out) and np.array_equal(got.cex_x, cx) and np.array_equal(got.cex_xp, cxp)
    assert np.array_equal(got.nodes, r1.nodes + r2.nodes) and got.iters == 0 and got.open_left is None
    # UNSAT only where both closed; a witness from whichever found one; an UNSAT given in stays
    assert got.status.tolist() == [UNSAT, SAT, SAT, UNKNOWN, SAT, UNSAT, UNKNOWN]
    assert got.cex_x[1].tolist() == r2.cex_x[1].tolist() and got.cex_x[2].tolist() == r1.cex_x[2].tolist()
    # nothing closed by the first solve: its result, the second never runs
    r0 = BaBResult(np.array([SAT, UNKNOWN], np.int8), np.zeros((2, 3), int), np.zeros((2, 3), int), np.ones(2, int))
    assert search.merge_orientations(r0, np.full(2, RUNNING, np.int8), None, time.time()) is r0


# ------------------------------------------------------------------------------------------ sweep, early return
@pytest.mark.parametrize("timed_out", [False, True])
def test_sweep_matches_the_inline_loop(timed_out):
    init = np.array([RUNNING, SAT, RUNNING, UNKNOWN, RUNNING, UNSAT, RUNNING], np.int8)
    part = torch.tensor([2, 2, 6, 1, 3])                 # the pool when the loop stopped
    status = init.copy()
    left = set(part.cpu().numpy().tolist()) if (timed_out and part.numel()) else set()
    for p in np.nonzero(status == RUNNING)[0]:
        status[p] = UNKNOWN if p in left else UNSAT
    v = Verdicts(7, 3, init)
    v.sweep(part.cpu().numpy() if timed_out else ())
    assert np.array_equal(v.status, status)
    assert v.status.tolist() == ([UNSAT, SAT, UNKNOWN, UNKNOWN, UNSAT, UNSAT, UNKNOWN] if timed_out else
                                 [UNSAT, SAT, UNSAT, UNKNOWN, UNSAT, UNSAT, UNSAT])
    assert Verdicts(7, 3, init).sweep(torch.zeros(0, dtype=torch.long).numpy()).status.tolist().count(UNSAT) == 5


def test_verdicts_early_return_and_result():
    init = np.array([RUNNING, SAT, UNKNOWN, RUNNING], np.int64)
    r = Verdicts(4, 3, init).close_running(UNSAT).result()
    assert r.status.tolist() == [UNSAT, SAT, UNKNOWN, UNSAT] and r.status.dtype == np.int8 and init[0] == RUNNING
    assert r.cex_x.shape == r.cex_xp.shape == (4, 3) and r.cex_x.dtype == np.int64 and not r.nodes.any()
    assert r.iters == 0 and r.time == 0.0 and r.open_left is None
    r = Verdicts(2, 3).result(time.time() - 2.0, iters=4, open_left=np.ones(2))
    assert r.status.tolist() == [RUNNING, RUNNING] and r.iters == 4 and r.time >= 2.0 and r.open_left.tolist() == [1, 1]


# ------------------------------------------------------------------------------------------ box operations
def test_tau_clamp_and_tau_apart():
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-5, 6, (50, 2), generator=g).float()
    xp = torch.randint(-9, 10, (50, 2), generator=g).float()
    for tau in (1.0, 3.0):
        assert torch.equal(search.clamp_tau(xp, x, tau), torch.minimum(torch.maximum(xp, x - tau), x + tau))
    lo, plo = x, xp
    hi, phi = lo + torch.randint(0, 3, (50, 2), generator=g), plo + torch.randint(0, 3, (50, 2), generator=g)
    want = ((plo > hi + 2.0) | (phi < lo - 2.0)).any(dim=1)
    assert torch.equal(search.tau_apart(lo, hi, plo, phi, 2.0), want) and want.any() and not want.all()


def test_pool_overflow_matches_the_inline_cut():
    part = torch.tensor([0, 1, 1, 2, 3, 3, 4, 1, 5])
    init = np.array([RUNNING, RUNNING, RUNNING, SAT, RUNNING, UNKNOWN], np.int8)
    max_pool = 4
    # the relu / beta block (host status) and the input-split block (device status)
    status = init.copy()
    lost = torch.unique(part[max_pool:]).cpu().numpy()
    lost = lost[status[lost] == RUNNING]
    status[lost] = UNKNOWN
    status_t = torch.from_numpy(init.copy())
    lost_t = torch.unique(part[max_pool:])
    status_t[lost_t[status_t[lost_t] == RUNNING]] = UNKNOWN
    got = init.copy()
    assert search.pool_overflow(part, max_pool, got) == lost.size == 2 and np.array_equal(got, status)
    got_t = torch.from_numpy(init.copy())
    assert search.pool_overflow(part, max_pool, got_t) == 2 and torch.equal(got_t, status_t)
    assert got.tolist() == [RUNNING, UNKNOWN, RUNNING, SAT, UNKNOWN, UNKNOWN]
    assert search.pool_overflow(part, 20, got) == 0


def test_halve_matches_the_inline_split():
    g = torch.Generator().manual_seed(1)
    lo = torch.randint(-4, 5, (12, 4), generator=g).float()
    hi = lo + torch.randint(0, 6, (12, 4), generator=g)
    rows = torch.tensor([0, 3, 4, 7, 11])
    dims = torch.tensor([1, 0, 3, 3, 2])
    lo1, hi1, lo2, hi2 = lo.clone(), hi.clone(), lo.clone(), hi.clone()
    mid = torch.floor((lo[rows, dims] + hi[rows, dims]) / 2)
    hi1[rows, dims] = mid
    lo2[rows, dims] = mid + 1
    for got, want in zip(search.halve(lo, hi, rows, dims), (lo1, hi1, lo2, hi2)):
        assert torch.equal(got, want)
    assert torch.equal(hi1[0], torch.where(torch.arange(4) == 1, torch.floor((lo[0] + hi[0]) / 2), hi[0]))
    none = torch.zeros(0, dtype=torch.long)
    assert all(torch.equal(a, b) for a, b in zip(search.halve(lo, hi, none, none), (lo, hi, lo, hi)))


# ------------------------------------------------------------------------------------------ max_pool, end to end
TOY5_HI = np.array([3, 4, 2, 4, 5])
TOY5 = Domain("toy5", tuple(Feature(f"f{i}", 0, int(w)) for i, w in enumerate(TOY5_HI)))


def _toy5_boxes():
    """f4 halved, three ranges of the PA f2: three PA groups of two partitions."""
    lo, hi = [], []
    for a, b in ((0, 2), (3, 5)):
        for pl, ph in ((0, 2), (0, 1), (1, 2)):
            l, h = np.zeros(5, np.int64), TOY5_HI.astype(np.int64).copy()
            l[4], h[4], l[2], h[2] = a, b, pl, ph
            lo.append(l)
            hi.append(h)
    return np.array(lo), np.array(hi)


def _brute(m, q, lo, hi):
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


@pytest.mark.parametrize("which", ["bab", "relu", "beta"])
def test_max_pool_truncation_gives_unknown_never_a_wrong_verdict(which):
    """A pool of a few nodes: the partitions that lose nodes end UNKNOWN, every decided verdict equals
    brute force and every witness is a true pair (node budgets far away, no time budget)."""
    lo, hi = _toy5_boxes()
    if which == "bab":
        q = Query(pa=("f2",)).resolve(TOY5)
        m = random_mlp(5, [8, 8], seed=400, bias_scale=0.5)
        solver = BaBSolver(Backend(m), q, BaBConfig(node_budget=10 ** 6, max_pool=3))
    elif which == "relu":
        q = Query(pa=("f2",), ra=("f3",), tau=1).resolve(TOY5)
        m = random_mlp(5, [6, 4], seed=304, bias_scale=1.0)
        solver = ReluBaBSolver(Backend(m), q, ReluConfig(node_budget=4096, max_pool=4))
    else:
        q = Query(pa=("f2",), ra=("f3",), tau=1).resolve(TOY5)
        m = random_mlp(5, [6, 4], seed=304, bias_scale=1.0)
        solver = BetaBaBSolver(Backend(m), q, BetaConfig(node_budget=256, iters=20, root_iters=40, max_pool=6))
    res = solver.solve(lo, hi, m)
    assert (res.status == UNKNOWN).any() and (res.status != UNKNOWN).any()
    assert not np.isin(res.status, (RUNNING,)).any()
    if which == "beta":
        assert solver.stats["pool_lost"] == int((res.status == UNKNOWN).sum())
    for k in np.nonzero(res.status != UNKNOWN)[0]:
        assert res.status[k] == _brute(m, q, lo[k], hi[k]), k
    sat = np.nonzero(res.status == SAT)[0]
    if sat.size:
        assert exact.check_pair_constraints(res.cex_x[sat], res.cex_xp[sat], lo[sat], hi[sat], q.pa_idx, q.ra_idx,
                                            q.tau).all()
        assert exact.is_violation(m, res.cex_x[sat], res.cex_xp[sat]).all()
