"""The infeasibility pass of the beta stage (ops/beta.py:feasibility_ref) on the CPU, on node sets built
for it -- three wave groups of rows that all reach the pass -- and the plumbing of
``BetaConfig.batched_feas`` on the CPU backend.  tests/test_beta_feas16_gpu.py runs the kernels on the
same sets (it imports the builders below)."""
import functools

import numpy as np
import pytest
import torch

from fairify_amd import presets
from fairify_amd.engine.bab import UNKNOWN
from fairify_amd.engine.beta_bab import BetaBaBSolver, BetaConfig
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import beta as B
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import processing_order

from test_beta_bab import _setup, _true_min

LR = (0.1, 0.5, 0.1)          # lr_a, lr_b, lr_t: the step sizes of the kernel tests (BetaConfig's defaults)
# Few-step comparisons of two fp32 implementations use a smaller multiplier step.  At lr_b = 0.5 the
# first Adam step (of size lr, whatever the gradient) takes every multiplier from its start 0.5 to
# within rounding of the box's ends 0 or 1; on rows where all of them reach 0 the second evaluation
# sees coefficients of size 1e-8, whose signs -- the concretising vertex, each unstable neuron's
# relaxation -- are rounding noise, and the third step differs between any two implementations (the
# per-node kernel against the reference too, and the reference between machines).
LR_FEW = (0.1, 0.1, 0.1)


def _wide(seed, widths, n0, R):
    from test_beta_opt16_gpu import _setup_wide_input

    return _setup_wide_input(seed, widths=widths, n0=n0, R=R)


def _relaxed(S, seed):
    from test_beta_opt16_gpu import _relax

    return _relax(S, seed, True)


@functools.lru_cache(maxsize=None)
def feas_set(seed, widths=(6, 5, 4), n0=4, R=48, tie=False):
    """A node set for the infeasibility pass: ``_setup`` / ``_setup_wide_input`` rows (R = 48: three wave
    groups of the batched kernel) whose phases are replaced -- per copy, three neurons unstable over
    the row's bounds fixed to random signs (seeded) --, so that every row has a fixed phase and no
    crossed bound; with ``bound = -1`` all of them run.  ``tie``: the relaxed variant (RA dim 2, the
    tau tie's multipliers, zeroed: the pass starts them at 0 whatever they hold).
    Returns (S, rx, ra, al, t): the setup tuple, the relaxed arguments (or None), the main pass's
    slopes [2 x (R, NH)] and pair weights [R]."""
    S = _setup(seed, widths=widths, R=R) if n0 == 4 else _wide(seed, widths, n0, R)
    rx = ra = None
    if tie:
        S, rx, ra = _relaxed(S, seed)
        rx = (rx[0], rx[1], rx[2], rx[3], torch.zeros_like(rx[4]), torch.zeros_like(rx[5]))
    m, ws, bs, pa, lo, hi, va, vb, bnd, _ = S
    NH = bnd[0][0].shape[1]
    g = np.random.default_rng(1000 + seed)
    ph = []
    for c in range(2):
        lb, ub = bnd[c][0].numpy(), bnd[c][1].numpy()
        p = np.zeros((R, NH), np.int8)
        for r in range(R):
            un = np.nonzero((lb[r] < 0) & (ub[r] > 0))[0]
            pick = g.choice(un, size=min(3, un.size), replace=False)
            p[r, pick] = g.choice(np.array([-1, 1], np.int8), size=pick.size)
        ph.append(torch.from_numpy(p))
    S = (m, ws, bs, pa, lo, hi, va, vb, bnd, ph)
    gt = torch.Generator().manual_seed(seed)
    al = [torch.rand(R, NH, generator=gt) for _ in range(2)]
    t = torch.rand(R, generator=gt)
    return S, rx, ra, al, t


@functools.lru_cache(maxsize=None)
def feas_ref(seed, widths=(6, 5, 4), n0=4, R=48, tie=False, iters=64, osg=1, pert=0, lr=LR):
    """(closed [R] bool, value [R] float64) of ops/beta.py:feasibility_ref on ``feas_set``, every row
    running (computed once per case and shared; callers must not modify it).  ``pert`` > 0: every start
    slope, pair weight and pre-activation bound moved by a relative N(0, 1) x 1e-6 drawn with that seed
    (:func:`unstable_rows`)."""
    S, rx, ra, al, t = feas_set(seed, widths, n0, R, tie)
    m, ws, bs, pa, lo, hi, va, vb, bnd, ph = S
    w = [x.shape[1] for x in ws[:-1]]
    lbA, ubA, iA = B.clamp_bounds(bnd[0][0], bnd[0][1], ph[0])
    lbB, ubB, iB = B.clamp_bounds(bnd[1][0], bnd[1][1], ph[1])
    assert not bool((iA | iB).any())
    run = torch.ones(R, dtype=torch.bool)
    og = None if osg == 1 else torch.full((R,), osg, dtype=torch.int8)
    alA, alB = al
    if pert:
        g = torch.Generator().manual_seed(pert)
        mv = lambda x: x * (1 + 1e-6 * torch.randn(x.shape, generator=g))  # noqa: E731
        alA, alB, t, lbA, ubA, lbB, ubB = (mv(x) for x in (alA, alB, t, lbA, ubA, lbB, ubB))
    return B.feasibility_ref(ws, bs, w, lo, hi, pa, va, vb, lbA, ubA, lbB, ubB, ph[0], ph[1], alA, alB, t, iters,
                             *lr, 1.0, rx, og, run, value=True)


@functools.lru_cache(maxsize=None)
def unstable_rows(seed, widths=(6, 5, 4), n0=4, R=48, tie=False, iters=3, lr=LR_FEW):
    """[R] bool: rows on which the REFERENCE's own few-step value is not defined to fp32 accuracy: it
    moves by more than 5e-6 under one of 16 random relative perturbations of size 1e-6 of its inputs
    (a smooth row moves by about the perturbation's size).  The pass's objective is piecewise linear --
    the concretising vertex and each unstable neuron's relaxation are step functions of a
    coefficient's sign -- and with objective weight 0 many coefficients start at or near 0: a row
    whose coefficient passes within rounding of 0 during the steps takes the other piece, another
    gradient and another trajectory (moves of 1e-3 .. 1e-1 on these sets).  Two fp32 implementations
    that sum in different orders cannot agree on such a row (the reference itself differs between
    machines there); the kernel tests compare few-step values on the others.  Computed from the
    reference alone, on the machine the test runs on."""
    base = feas_ref(seed, widths, n0, R, tie, iters, 1, 0, lr)[1]
    mv = torch.zeros(R, dtype=torch.float64)
    for k in range(1, 17):
        mv = torch.maximum(mv, (feas_ref(seed, widths, n0, R, tie, iters, 1, k, lr)[1] - base).abs())
    return mv > 5e-6


@functools.lru_cache(maxsize=None)
def lattice_empty(seed, widths=(6, 5, 4), n0=4, R=48, tie=False):
    """[R] bool: no lattice point of the row's box satisfies both copies' phases (relaxed: no pair
    within the tie)."""
    S, rx, ra, al, t = feas_set(seed, widths, n0, R, tie)
    m, ws, bs, pa, lo, hi, va, vb, bnd, ph = S
    w = [x.shape[1] for x in ws[:-1]]
    out = np.zeros(R, bool)
    for r in range(R):
        if tie:
            from test_beta_gpu import _true_min_rx

            tm = _true_min_rx(m, lo[r].numpy(), hi[r].numpy(), rx[1][r].numpy(), rx[2][r].numpy(), pa, ra,
                              va[r].numpy(), vb[r].numpy(), ph[0][r].numpy(), ph[1][r].numpy(), 0.5, float(rx[3]))
        else:
            tm = _true_min(m, lo[r].numpy(), hi[r].numpy(), pa, va[r].numpy(), vb[r].numpy(), ph[0][r].numpy(),
                           ph[1][r].numpy(), 0.5, w)
        out[r] = not np.isfinite(tm)
    return torch.from_numpy(out)


CASES = [(s, (6, 5, 4), 4) for s in range(4)] + [(s, (20, 17, 4), 17) for s in range(2)]


@pytest.mark.parametrize("seed,widths,n0", CASES)
def test_reference_closes_only_lattice_empty_rows(seed, widths, n0):
    """feasibility_ref(value=True): the mask is ``value > 0``; at 3 steps it closes 12-21 of the 48 rows,
    at 64 steps 28-40 and leaves 8-20 open; every closed row has no lattice point satisfying its phases
    (zero slack)."""
    emp = lattice_empty(seed, widths, n0)
    for iters, lo_n, hi_n in ((3, 12, 21), (64, 28, 40)):
        closed, val = feas_ref(seed, widths, n0, iters=iters)
        assert val.dtype == torch.float64 and tuple(val.shape) == (48,)
        assert torch.equal(closed, val > 0)
        assert lo_n <= int(closed.sum()) <= hi_n, int(closed.sum())
        assert bool(emp[closed].all())
    assert 8 <= int((~closed).sum()) <= 20


@pytest.mark.parametrize("seed", [0, 7, 8, 9])
def test_reference_relaxed_tie_closes_only_pairless_rows(seed):
    """The relaxed tie variant: 28-33 of 48 close at 64 steps, none with a lattice pair within the tie.
    (The count depends on the generator that draws the phases: with ``feas_set``'s, seeds 0-11 close
    25-38; the seeds here are those inside the range.)"""
    closed, val = feas_ref(seed, tie=True)
    assert torch.equal(closed, val > 0)
    assert 28 <= int(closed.sum()) <= 33, int(closed.sum())
    assert bool(lattice_empty(seed, tie=True)[closed].all())


def test_reference_mask_is_unchanged_without_value():
    S, rx, ra, al, t = feas_set(0)
    m, ws, bs, pa, lo, hi, va, vb, bnd, ph = S
    w = [x.shape[1] for x in ws[:-1]]
    lbA, ubA, _ = B.clamp_bounds(bnd[0][0], bnd[0][1], ph[0])
    lbB, ubB, _ = B.clamp_bounds(bnd[1][0], bnd[1][1], ph[1])
    run = torch.ones(48, dtype=torch.bool)
    run[::5] = False
    args = (ws, bs, w, lo, hi, pa, va, vb, lbA, ubA, lbB, ubB, ph[0], ph[1], al[0], al[1], t, 8, *LR, 1.0, None, None,
            run)
    mask = B.feasibility_ref(*args)
    mask2, val = B.feasibility_ref(*args, value=True)
    assert isinstance(mask, torch.Tensor) and torch.equal(mask, mask2)
    assert torch.equal(mask, run & (val > 0))


def test_batched_feas_is_inert_on_the_cpu_backend():
    """BetaConfig.batched_feas on the CPU backend: the torch reference runs unchanged --
    stats["batched_feas"] stays false and the verdicts are the default config's."""
    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    ids = processing_order(grid, 0)[:6]
    lo, hi = grid.decode(ids)
    hi = np.minimum(hi, lo + 1)
    m = random_mlp(13, [8, 6, 4], seed=3, bias_scale=0.5)
    out = []
    for kw in ({}, dict(batched=True, batched_feas=True)):
        sol = BetaBaBSolver(Backend(m), q, BetaConfig(node_budget=128, iters=20, root_iters=40, **kw))
        res = sol.solve(lo, hi, m)
        assert sol.stats["batched_feas"] is False
        assert sol.stats["batched"] is False
        out.append(res.status.copy())
    assert int((out[0] == UNKNOWN).sum()) == 0
    assert bool((out[0] == out[1]).all())


def test_batched_feas_default_is_off():
    assert BetaConfig().batched_feas is False


@pytest.mark.parametrize("bad", [-1, 4, 8])
def test_pgap_weights_are_validated(bad):
    """pgap_weights outside 0..3 would spill into the infeasibility pass's bit of the kernels' flags
    word: both the solver and the flag packing refuse it."""
    from fairify_amd.ops import hip

    q = presets.get("src/AC-sex").resolved()
    m = random_mlp(13, [8, 6, 4], seed=3, bias_scale=0.5)
    with pytest.raises(ValueError):
        BetaBaBSolver(Backend(m), q, BetaConfig(pgap_weights=bad))
    with pytest.raises(ValueError):
        hip.beta_flags(True, bad)
    assert [hip.beta_flags(True, p) for p in range(4)] == [1, 3, 5, 7]
    assert hip.beta_flags(False, 0, feas=True) == 8
