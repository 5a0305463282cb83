"""The pair certificate's CPU reference (ops/reference.py:pair_certify, the CPU backend's node test and
the comparison of tests/test_kernels_gpu.py) against lattice enumeration and the float64 oracle of
tests/certify_cases.py."""
import dataclasses

import numpy as np
import pytest
import torch

import certify_cases as cc
from fairify_amd.ops import reference as ref


def _ref(s):
    return s.be.pair_certify(*cc.certify_args(s))


def test_oracle_breakpoints_reach_the_grid_minimum():
    """The oracle evaluates t in {0, 1} and the breakpoints only: on a 2001-point grid of t the objective
    (with and without the margin, both convex piecewise linear with the same breakpoints) never goes
    below the oracle's minimum."""
    grid = np.linspace(0.0, 1.0, 2001)
    n_inner = 0
    for name in ("f16_q4_n257", "t16_q132_n65", "f32_q4_n65"):
        s = cc.build(cc.MATRIX[name]._replace(Nn=12))
        o = cc.oracle(s)
        for n in range(o.Nn):
            for qq in range(o.Q):
                gg = cc.g64(o.Ac[n, qq], o.A0[n, qq], o.Bc[n, qq], o.B0[n, qq], o.sh, o.xlo[n], o.xhi[n],
                            o.xplo[n], o.xphi[n], grid)
                k = int(np.sum(~np.isnan(o.ts[n, qq])))
                assert np.nanmin(o.g[n, qq]) <= gg.min() + 1e-12 * (1 + abs(gg.min()))
                mg = ((2 * o.n0 + 6) * cc.UNIT / (1 - (2 * o.n0 + 6) * cc.UNIT)
                      * (grid * o.magA[n, qq] + (1 - grid) * o.magB[n, qq])
                      + 8 * cc.UNIT * (o.magA[n, qq] + o.magB[n, qq]))
                assert np.nanmin(o.g[n, qq] + 3 * o.marg[n, qq]) <= (gg + 3 * mg).min() + 1e-12 * (1 + abs(gg.min()))
                n_inner += int(np.argmin(o.g[n, qq, :k]) >= 2)
    assert n_inner > 20          # minima at breakpoints inside (0, 1) took part


@pytest.mark.parametrize("shape", list(cc.SOUND_SHAPES))
def test_reference_closes_no_violating_node(shape):
    """Soundness by enumeration on the toy lattice: a node the reference closes holds no pair (x, x') of
    opposite float64 logit signs.  Not vacuous: at least 10 % of the nodes are closed and at least
    10 % hold a violation."""
    closed, viol = [], []
    for c, truth in zip(cc.sound_cases(shape), cc.sound_truth(shape)):
        dec = _ref(cc.build(c))
        closed.append(~dec.open_.numpy())
        viol.append(truth)
    closed, viol = np.concatenate(closed), np.concatenate(viol)
    print(f"{shape}: closed {closed.mean():.3f} violating {viol.mean():.3f} of {closed.size} nodes")
    assert not np.any(closed & viol)
    assert closed.mean() >= 0.10 and viol.mean() >= 0.10


@pytest.mark.parametrize("name", list(cc.MATRIX))
def test_reference_against_oracle(name):
    """The fp32 reference never scores a node below the float64 oracle (the margin covers its rounding),
    leaves open what the oracle leaves open, and stays within twice the margin above it; the smallest k
    with score <= max_q min_t (g64 + k marg) is at most cc.K_REF (1.026459 measured, on f16_q4_n257), the
    figure the kernels' upper bound in tests/test_certify_gpu.py doubles."""
    s = cc.build(cc.MATRIX[name])
    o = cc.oracle(s)
    dec = _ref(s)
    score = dec.score.numpy().astype(np.float64)
    low = cc.node_values(o, 0.0)
    assert np.all(score >= low)
    assert np.array_equal(dec.open_.numpy(), score > 0)
    assert np.all(dec.open_.numpy()[low > 0])
    k = cc.smallest_k(o, score)
    print(f"{name}: largest k {k.max():.6f}, (score - oracle) / (|score| + 1) <= "
          f"{((score - low) / (np.abs(score) + 1)).max():.2e}")
    # the margin is added once and bounds the rounding: never more than twice the margin above the oracle
    assert np.all(score <= cc.node_values(o, 2.0))
    assert k.max() <= cc.K_REF


def test_reference_keeps_a_nan_node_open():
    """A non-finite certificate value never closes a node (the kernels' rule): NaN in one row's form
    leaves the node open, and its neighbours as they were."""
    s = cc.build(cc.NAN_CASE)
    base = _ref(s)
    n = cc.nan_target(s, base.open_.numpy())
    dec = _ref(cc.with_nan(s, n))
    assert bool(dec.open_[n]) and not bool(base.open_[n])
    keep = torch.arange(64) != n
    assert torch.equal(dec.open_[keep], base.open_[keep]) and torch.equal(dec.score[keep], base.score[keep])


@pytest.mark.parametrize("npairs", [3, None])
def test_reference_exact_forms(npairs):
    """Forms that fp32 evaluates without rounding (cc.exact_case): the score is the exact objective plus
    the margin -- both terms of it, with the PA terms' magnitudes summed, not their cancelling sum."""
    s = cc.exact_case(npairs)
    want, tol = cc.exact_bounds(s)
    got = _ref(s).score.numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= tol)


def test_wide_input_falls_back_to_the_reference(monkeypatch):
    """n0 = 33 on a backend that runs the HIP kernels: pair_certify takes the reference on the backend's
    tensors instead of the kernels (which hold at most 32 dims in registers)."""
    from fairify_amd.ops import hip

    s = cc.build(cc.Case(33, (8, 6), (2,), (), 0, 9, 30, 0.0))
    want = _ref(s)
    monkeypatch.setattr(s.be, "hip", True)
    monkeypatch.setattr(hip, "pair_certify", lambda *a, **k: pytest.fail("the kernel wrapper was called"))
    got = _ref(s)
    for f in dataclasses.fields(ref.PairDecision):
        assert torch.equal(getattr(got, f.name), getattr(want, f.name))
    narrow = cc.build(cc.Case(32, (8, 6), (2,), (), 0, 2, 31, 0.0))
    monkeypatch.setattr(narrow.be, "hip", True)
    with pytest.raises(BaseException, match="the kernel wrapper was called"):
        _ref(narrow)
