"""The infeasibility pass of the beta stage on the GPU: the per-node pass (csrc/beta.hip, ``a.feas``)
and the two-phase pass of ``BetaConfig.batched_feas`` (proposals by the feas mode of
fa_beta_opt16_kernel, 16 nodes per wave; decision by fa_beta_kernel at iters = 0 on its rigorous fp64
value) against ops/beta.py:feasibility_ref and lattice enumeration, on the node sets of
tests/test_beta_feas_cpu.py (48 rows: three wave groups; every row reaches the pass)."""
import numpy as np
import pytest
import torch

from fairify_amd import presets
from fairify_amd.engine import exact
from fairify_amd.engine.bab import SAT, UNKNOWN
from fairify_amd.engine.beta_bab import BetaBaBSolver, BetaConfig
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import hip
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import processing_order

from test_beta_bab import _brute_pair
from test_beta_feas_cpu import LR, LR_FEW, feas_ref, feas_set, lattice_empty, unstable_rows

pytestmark = pytest.mark.gpu

# (seed, widths, n0, R, tie): one case per instance of the batched kernel -- 1 tile; 2 tiles with a
# ragged second input tile; 4 tiles; 7 tiles (AC-4's shape) -- and the relaxed tie variant
T1, T2, T4, T7 = ((6, 5, 4), 4, 48), ((20, 17, 4), 17, 48), ((50, 8), 8, 48), ((100, 100), 13, 20)


def _pass(cuda, case, iters, batched, osg=1, rows=None, bound=None, proposal=None, ret=False, lr=LR):
    """hip.beta_feas on the rows ``rows`` (default all) of ``feas_set(*case)``, bound = -1 unless given:
    CPU copies of (closed, value[, (fpar, fgt)])."""
    S, rx, ra, al, t = feas_set(*case)
    m, ws, bs, pa, lo, hi, va, vb, bnd, ph = S
    R = lo.shape[0]
    idx = torch.arange(R) if rows is None else torch.as_tensor(rows)
    d = lambda x: x[idx].to(cuda).contiguous()  # noqa: E731
    rxg = None if rx is None else (rx[0], d(rx[1]), d(rx[2]), rx[3], d(rx[4]), d(rx[5]))
    b = torch.full((R,), -1.0, dtype=torch.float64) if bound is None else bound
    og = None if osg == 1 else torch.full((idx.numel(),), osg, dtype=torch.int8, device=cuda)
    out = hip.beta_feas(Backend(m, cuda), d(lo), d(hi), pa, d(va), d(vb), d(bnd[0][0]), d(bnd[0][1]), d(bnd[1][0]),
                        d(bnd[1][1]), d(ph[0]), d(ph[1]), d(al[0]), d(al[1]), d(t), d(b), iters, lr, batched, rx=rxg,
                        osg=og, proposal=proposal, return_proposal=ret)
    torch.cuda.synchronize()
    if ret:
        return out[0].cpu(), out[1].cpu(), tuple(None if x is None else x.cpu() for x in out[2])
    return out[0].cpu(), out[1].cpu()


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", [(0,) + T1 + (False,), (0,) + T1 + (True,), (6,) + T2 + (False,)])
def test_per_node_pass_matches_reference(cuda, case):
    """The per-node pass (batched off: the kernel this feature leaves unchanged).  iters = 0: both
    evaluate the pass's start values in fp64 -- the values agree at the tolerance of
    test_beta_gpu.py's rigorous bounds against level_ref (1e-9), and the kernel closes exactly the rows
    the reference closes, outside rows whose reference value is within that tolerance of 0.  Three
    steps at the few-step step sizes (test_beta_feas_cpu.py:LR_FEW): the same at the few-step tolerance
    1e-5."""
    for iters, tol in ((0, 1e-9), (3, 1e-5)):
        rc, rv = feas_ref(*case, iters=iters, lr=LR_FEW)
        closed, val = _pass(cuda, case, iters, False, lr=LR_FEW)
        if iters:
            _stable(case, val, rv, "per-node")
        print("per-node", case, iters, "max |value - ref|", float((val - rv).abs().max()), "closed",
              int(closed.sum()), "ref", int(rc.sum()))
        assert torch.allclose(val, rv, rtol=tol, atol=tol)
        far = rv.abs() > tol
        assert torch.equal(closed[far], rc[far])
        assert torch.equal(closed, val > 0)
    assert int(rc.sum()) >= 2


# ---------------------------------------------------------------------------------------------- 2
# Three steps at the few-step step sizes (test_beta_feas_cpu.py:LR_FEW, and why).  Seeds for which the
# reference alone has at most 4 of 48 rows within 1e-5 of 0 (these have none) and no row on which its own
# three-step value is undefined at fp32 accuracy (unstable_rows), checked on the CPU over seeds 0-11 of
# every shape; both are asserted again where the test runs.
FEW = [((0,) + T1 + (False,), 1), ((3,) + T1 + (False,), -1), ((0,) + T1 + (True,), 1), ((11,) + T1 + (True,), -1),
       ((6,) + T2 + (False,), 1), ((0,) + T4 + (False,), 1), ((5,) + T7 + (False,), 1)]


def _stable(case, val, rv, what):
    """Asserts that the reference's few-step value is defined on every row (prints the rows off by more
    than 1e-5)."""
    off = torch.nonzero((val - rv).abs() > 1e-5 * (1 + rv.abs())).flatten().tolist()
    print(what, case, "rows off by > 1e-5:", [(r, float(val[r]), float(rv[r])) for r in off])
    assert int(unstable_rows(*case).sum()) == 0


@pytest.mark.parametrize("case,osg", FEW)
def test_batched_few_steps_track_reference(cuda, case, osg):
    """Three steps, batched: the rigorous value at the proposals equals the reference's at the few-step
    tolerance of test_two_phase_few_steps_track_reference (rtol = atol = 1e-5), and the closed sets are
    equal outside the rows whose reference value lies within that tolerance of 0 -- at most 4 of 48."""
    rc, rv = feas_ref(*case, iters=3, osg=osg, lr=LR_FEW)
    near = rv.abs() <= 1e-5
    assert int(near.sum()) <= (4 if case[3] == 48 else 2)
    closed, val = _pass(cuda, case, 3, True, osg=osg, lr=LR_FEW)
    _stable(case, val, rv, "batched")
    print("few steps", case, osg, "max |value - ref|", float((val - rv).abs().max()), "closed", int(closed.sum()),
          "ref", int(rc.sum()), "near 0", int(near.sum()))
    assert torch.allclose(val, rv, rtol=1e-5, atol=1e-5)
    assert torch.equal(closed[~near], rc[~near])
    assert torch.equal(closed, val > 0)
    assert int(closed.sum()) > 0
    assert bool(lattice_empty(*case)[closed].all())         # (test 4: zero slack)


# ---------------------------------------------------------------------------------------------- 3
FULL = [((0,) + T1 + (False,), 1), ((1,) + T1 + (False,), -1), ((0,) + T1 + (True,), 1), ((7,) + T1 + (True,), -1),
        ((0,) + T2 + (False,), 1), ((0,) + T4 + (False,), 1), ((7,) + T7 + (False,), 1)]


@pytest.mark.parametrize("case,osg", FULL)
def test_batched_full_pass(cuda, case, osg):
    """64 steps, batched: |value - ref| < 0.05 (1 + max |ref|) (the bar of
    test_two_phase_optimises_soundly), every row whose reference value exceeds that band is closed, at
    least 8 rows close and at least 8 stay open (asserted on the reference first), and no closed row has
    a lattice point that satisfies its phases."""
    rc, rv = feas_ref(*case, iters=64, osg=osg)
    assert int(rc.sum()) >= 8 and int((~rc).sum()) >= 8
    band = 0.05 * (1 + float(rv.abs().max()))
    assert int((rv > band).sum()) > 0
    closed, val = _pass(cuda, case, 64, True, osg=osg)
    print("full pass", case, osg, "max |value - ref|", float((val - rv).abs().max()), "band", band, "closed",
          int(closed.sum()), "ref", int(rc.sum()))
    assert float((val - rv).abs().max()) < band
    assert bool(closed[rv > band].all())
    assert int(closed.sum()) >= 8 and int((~closed).sum()) >= 8
    assert torch.equal(closed, val > 0)
    assert bool(lattice_empty(*case)[closed].all())         # (test 4: zero slack)


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case", [(0,) + T1 + (False,), (0,) + T1 + (True,), (0,) + T2 + (False,)])
def test_rigorous_phase_is_sound_on_untrusted_proposals(cuda, case):
    """The rigorous phase called directly: with the pass's start values as the proposal it is the
    reference at iters = 0 (so it does read the buffers); with hostile ones -- NaN, infinities, negative
    values, values > 1, non-zero multipliers on unfixed neurons, in the parameters and in the tie
    multipliers -- no row with a phase-feasible lattice point closes."""
    S, rx, ra, al, t = feas_set(*case)
    ph = S[9]
    R, NH = ph[0].shape
    n0 = S[4].shape[1]
    emp = lattice_empty(*case)
    g = torch.Generator().manual_seed(5)
    start = torch.stack([al[0], al[1], (ph[0] != 0).float() * 0.5, (ph[1] != 0).float() * 0.5], 1)
    zgt = torch.zeros(R, 2, n0)
    rc, rv = feas_ref(*case, iters=0)
    closed, val = _pass(cuda, case, 0, True, proposal=(start.to(cuda), zgt.to(cuda)))
    assert torch.allclose(val, rv, rtol=1e-9, atol=1e-9)
    assert torch.equal(closed[rv.abs() > 1e-9], rc[rv.abs() > 1e-9])
    rnd = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    best = _pass(cuda, case, 64, True, ret=True)[2]         # honest proposals to corrupt
    hostile = {
        "nan": (torch.full((R, 4, NH), float("nan")), torch.full((R, 2, n0), float("nan"))),
        "inf": (torch.full((R, 4, NH), float("inf")), torch.full((R, 2, n0), float("inf"))),
        "-inf": (torch.full((R, 4, NH), -float("inf")), torch.full((R, 2, n0), -float("inf"))),
        "negative": (-3 * rnd(R, 4, NH), -3 * rnd(R, 2, n0)),
        "large": (1 + 5 * rnd(R, 4, NH), 1 + 5 * rnd(R, 2, n0)),
        "unfixed": (rnd(R, 4, NH), rnd(R, 2, n0)),
        "mixed sign": (4 * rnd(R, 4, NH) - 2, 4 * rnd(R, 2, n0) - 2),
        "best, slopes out of range": (torch.cat([best[0][:, :2] * 40 - 20, best[0][:, 2:]], 1),
                                      zgt if best[1] is None else -best[1]),
        "best, some NaN": (torch.where(rnd(R, 4, NH) < 0.1, torch.full((R, 4, NH), float("nan")), best[0]), zgt),
    }
    n_closed = 0
    for name, (fp, fg) in hostile.items():
        closed, val = _pass(cuda, case, 0, True, proposal=(fp.to(cuda), fg.to(cuda)))
        print("untrusted", case, name, "closed", int(closed.sum()))
        assert bool(emp[closed].all()), name
        assert torch.equal(closed, val > 0), name
        n_closed += int(closed.sum())
    assert n_closed > 0          # (some hostile proposals still prove rows empty: the check is not vacuous)


# ---------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("case", [(0,) + T1 + (False,), (0,) + T1 + (True,), (0,) + T2 + (False,)])
def test_batched_pass_moves_nothing_else(cuda, case):
    """hip.beta_level (two main steps, two-phase level) with and without the batched infeasibility
    pass: par, t, the tie multipliers, split, xstar, xpstar and binit are bitwise the same, and bound
    differs only by +inf on the rows the pass closes (some, but not all of the open ones)."""
    S, rx, ra, al, t = feas_set(*case)
    m, ws, bs, pa, lo, hi, va, vb, bnd, ph = S
    d = lambda x: x.to(cuda).contiguous()  # noqa: E731
    be = Backend(m, cuda)
    out = []
    for fi in (0, 64):
        p = [d(al[0].clone()), d(al[1].clone()), d(torch.zeros_like(al[0])), d(torch.zeros_like(al[0])), d(t.clone())]
        rxg = None if rx is None else (rx[0], d(rx[1]), d(rx[2]), rx[3], d(rx[4].clone()), d(rx[5].clone()))
        lev = hip.beta_level(be, d(lo), d(hi), pa, d(va), d(vb), d(bnd[0][0]), d(bnd[0][1]), d(bnd[1][0]),
                             d(bnd[1][1]), d(ph[0]), d(ph[1]), *p, iters=2, lr_a=LR[0], lr_b=LR[1], lr_t=LR[2], rx=rxg,
                             feas_iters=fi, batched=True, batched_feas=True)
        torch.cuda.synchronize()
        out.append((lev, [x.cpu() for x in p] + ([] if rx is None else [rxg[4].cpu(), rxg[5].cpu()])))
    (l0, p0), (l1, p1) = out
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)
    for k in ("split", "xstar", "xpstar", "binit"):
        assert torch.equal(getattr(l0, k).cpu(), getattr(l1, k).cpu()), k
    b0, b1 = l0.bound.cpu(), l1.bound.cpu()
    moved = ~((b0 == b1) | (torch.isnan(b0) & torch.isnan(b1)))
    assert int(moved.sum()) > 0
    assert bool((b0[moved] < 0).all()) and bool((b1[moved] == float("inf")).all())
    assert int(((b0 < 0) & ~moved).sum()) > 0


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("case", [(0,) + T2 + (False,), (0,) + T1 + (True,)])
def test_batched_pass_neighbour_independence(cuda, case):
    """A row's proposals and value are bitwise the same alone, in the full set and in the reversed
    set (40 steps: rows freeze at different steps while their wave goes on); rows that do not qualify
    (bound >= 0 here) get no output -- the proposal buffers keep what they held, no value, not closed."""
    R, iters = case[3], 40
    bound = torch.full((R,), -1.0, dtype=torch.float64)
    out_rows = list(range(3, R, 7))
    bound[out_rows] = 1.0
    rev = list(range(R - 1, -1, -1))
    cf, vf, pf = _pass(cuda, case, iters, True, bound=bound, ret=True)
    cr, vr, pr = _pass(cuda, case, iters, True, bound=bound, rows=rev, ret=True)
    assert int(cf.sum()) >= 8 and int((~cf).sum()) >= 8          # frozen and running columns share waves
    for k in out_rows:
        assert not bool(cf[k]) and bool(torch.isnan(vf[k]))
        assert bool((pf[0][k] == 0).all()) and (pf[1] is None or bool((pf[1][k] == 0).all()))
    ran = [k for k in range(R) if k not in out_rows]
    assert not bool(torch.isnan(vf[ran]).any())
    for k in range(R):
        assert torch.equal(pr[0][R - 1 - k], pf[0][k]), k
        assert torch.equal(vr[R - 1 - k], vf[k]) or (k in out_rows), k
        assert bool(cr[R - 1 - k]) == bool(cf[k]), k
        if pf[1] is not None:
            assert torch.equal(pr[1][R - 1 - k], pf[1][k]), k
    for k in (0, 15, 16, 21, R - 1):
        ca, va_, pa_ = _pass(cuda, case, iters, True, bound=bound, rows=[k], ret=True)
        assert torch.equal(pa_[0][0], pf[0][k]), k
        assert torch.equal(va_[0], vf[k]), k
        assert bool(ca[0]) == bool(cf[k]), k
        if pf[1] is not None:
            assert torch.equal(pa_[1][0], pf[1][k]), k


# ---------------------------------------------------------------------------------------------- 8
def _solve_both(cuda, m, q, lo, hi, budget, branch, check, **kw):
    out = {}
    for native in (True, False):
        sol = BetaBaBSolver(Backend(m, cuda), q, BetaConfig(node_budget=budget, iters=20, root_iters=40, branch=branch,
                                                            native=native, batched=True, **kw))
        res = sol.solve(lo, hi, m)
        assert bool(sol.stats.get("native")) == native
        assert sol.stats.get("batched") is True
        assert sol.stats.get("batched_feas") is bool(kw.get("batched_feas", False))
        assert int((res.status == UNKNOWN).sum()) == 0, res.status
        check(res)
        out[native] = res.status
    assert bool((out[True] == out[False]).all())


@pytest.mark.parametrize("seed,branch", [(3, "kernel"), (6, "kernel"), (3, "pgap")])
def test_batched_feas_bab_matches_bruteforce(cuda, seed, branch):
    """BetaBaBSolver with batched and batched_feas on (the setup and budgets of
    test_beta_opt16_gpu.py::test_batched_bab_matches_bruteforce): native and torch loops, no UNKNOWN,
    verdicts equal to lattice enumeration and to each other, every SAT pair exactly confirmed,
    stats["batched_feas"] true -- and false with the switch off."""
    from test_beta_opt16_gpu import BUDGETS

    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    ids = processing_order(grid, 0)[:24]
    lo, hi = grid.decode(ids)
    hi = np.minimum(hi, lo + 1)
    m = random_mlp(13, [8, 6, 4], seed=seed, bias_scale=0.5)
    pa = q.pa_idx[0]

    def check(res):
        for k in range(len(ids)):
            assert (res.status[k] == SAT) == _brute_pair(m, lo[k], hi[k], pa), k
        sat = np.nonzero(res.status == SAT)[0]
        if sat.size:
            assert exact.is_violation(m, res.cex_x[sat], res.cex_xp[sat]).all()

    _solve_both(cuda, m, q, lo, hi, BUDGETS[("pa", seed, branch)], branch, check, batched_feas=True)
    if seed == 6:
        _solve_both(cuda, m, q, lo, hi, BUDGETS[("pa", seed, branch)], branch, check)


@pytest.mark.parametrize("seed,tau", [(21, 2), (24, 3)])
def test_batched_feas_bab_relaxed_matches_bruteforce(cuda, seed, tau):
    """Relaxed twin (test_beta_opt16_gpu.py::test_batched_bab_relaxed_matches_bruteforce): x' RA boxes,
    the tie's multipliers and both orientations through the two-phase infeasibility pass."""
    from fairify_amd.spec import ADULT, Query
    from test_beta_bab import _relaxed_truth
    from test_beta_opt16_gpu import BUDGETS

    q = Query(pa=("sex",), ra=("age",), tau=tau).resolve(ADULT)
    grid = presets.get("src/AC-sex").grid()
    ids = processing_order(grid, 0)[:16]
    lo, hi = grid.decode(ids)
    hi = np.minimum(hi, lo + 1)
    pa, ra = q.pa_idx[0], q.ra_idx[0]
    m = random_mlp(13, [8, 6, 4], seed=seed, bias_scale=0.5)
    truth = [_relaxed_truth(m, lo[k], hi[k], pa, ra, tau) for k in range(len(ids))]

    def check(res):
        for k in range(len(ids)):
            assert (res.status[k] == SAT) == truth[k], k
            if res.status[k] == SAT:
                ok = exact.check_pair_constraints(res.cex_x[k:k + 1], res.cex_xp[k:k + 1], lo[k:k + 1], hi[k:k + 1],
                                                  q.pa_idx, q.ra_idx, q.tau)
                assert ok[0] and exact.is_violation(m, res.cex_x[k:k + 1], res.cex_xp[k:k + 1])[0]

    _solve_both(cuda, m, q, lo, hi, BUDGETS[("rx", seed, tau)], "kernel", check, batched_feas=True)
