"""Compile-time-shape instances of the paired / packed symbolic kernels and of the AC-11 refine kernel
(csrc/symbolic.hip SymShape, csrc/refine.hip FaShape) against the run-time-shape kernels they
specialise: every output bitwise equal.  BaB verdicts on the zero-bias narrow nets hang on exact
zeros, so "equal to rounding" is not enough here."""
import numpy as np
import pytest
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

PA = 8                      # Adult's protected attribute (sex): folded in the node-row expansion
# the bench's narrow chains: paired (two box rows per wave) and packed (PG = 2 boxes per MFMA tile)
NARROW = [
    ("AC-1", [16, 8]), ("AC-6", [12, 12]), ("AC-11", [10, 10, 10, 10]),            # paired
    ("AC-8", [5, 5]), ("AC-10", [5, 5, 5, 5]), ("AC-12", [5] * 9),                # packed
]
# 1 / 2 / 3 / 5: a last wave pass with one valid row (paired: 1 of 2, packed: 1 of 4) and with three
# (packed); 701: several workgroups and an odd tail
ROWS = (1, 2, 3, 5, 701)
FIELDS = ("out_lb", "out_ub", "Lc", "Uc", "L0", "U0", "Le", "Ue")


def _boxes(n0, R, seed):
    g = np.random.default_rng(seed)
    lo = g.integers(-5, 20, size=(R, n0)).astype(np.float32)
    hi = lo + g.integers(0, 6, size=(R, n0)).astype(np.float32)
    hi[:, PA] = lo[:, PA] = g.integers(0, 2, size=R).astype(np.float32)
    return torch.from_numpy(lo), torch.from_numpy(hi)


def _assert_equal(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert torch.equal(x, y), f
    assert len(a.layer_lb) == len(b.layer_lb) and len(a.layer_ub) == len(b.layer_ub)
    for k, (x, y) in enumerate(zip(a.layer_lb, b.layer_lb)):
        assert torch.equal(x, y), ("layer_lb", k)
    for k, (x, y) in enumerate(zip(a.layer_ub, b.layer_ub)):
        assert torch.equal(x, y), ("layer_ub", k)
    assert (a.dead is None) == (b.dead is None)
    if a.dead is not None:
        assert torch.equal(a.dead, b.dead)


@pytest.mark.parametrize("dead", [False, True])
@pytest.mark.parametrize("name,hidden", NARROW)
def test_shaped_narrow_symbolic_is_bitwise_the_generic_one(cuda, monkeypatch, name, hidden, dead):
    from fairify_amd.ops import ext, hip

    # zero biases (the bench's random-init nets: exact zeros decide partitions) and non-zero ones
    for bias in (0.0, 0.3):
        m = random_mlp(13, hidden, seed=31 + len(hidden) + hidden[0], bias_scale=bias)
        be = Backend(m, cuda)
        assert be.hip
        # the launch's own selection: a shaped instance for every chain but AC-12 (its ten unrolled
        # layers spill, csrc/symbolic.hip: both runs take the run-time-shape kernel), none with the
        # switch off
        fold = hip._fold_mask((PA,), 13)
        monkeypatch.setenv("FAIRIFY_SYM_SHAPED", "1")
        assert ext().sym_shaped(hip._net(be), fold) == (name != "AC-12")
        monkeypatch.setenv("FAIRIFY_SYM_SHAPED", "0")
        assert not ext().sym_shaped(hip._net(be), fold)
        for R in ROWS:
            lo, hi = _boxes(13, R, 17 + R)
            dm = None
            if dead:
                dm = (torch.rand(R, m.n_neurons - 1, generator=torch.Generator().manual_seed(R)) < 0.2).to(cuda)
            outs = []
            for shaped in ("1", "0"):
                monkeypatch.setenv("FAIRIFY_SYM_SHAPED", shaped)
                outs.append(be.bounds(lo.to(cuda), hi.to(cuda), mode="symbolic", keep_layers=True, fold=(PA,), dead=dm))
            torch.cuda.synchronize()
            _assert_equal(*outs)


@pytest.mark.parametrize("dead", [False, True])
def test_shaped_ac11_refine_is_bitwise_the_generic_one(cuda, monkeypatch, dead):
    """AC-11 (13-10-10-10-10-1), the only narrow model on the refine path: back-substituted hidden
    bounds + backward logit pass with the compile-time-shape refine kernel and with the generic one."""
    from fairify_amd.ops import ext, hip

    for bias in (0.0, 0.3):
        m = random_mlp(13, [10, 10, 10, 10], seed=77, bias_scale=bias)
        be = Backend(m, cuda)
        # refine=True, crown=True is one launch without and one with the logit's backward pass
        for logit in (False, True):
            monkeypatch.setenv("FAIRIFY_REFINE_SHAPED", "1")
            assert ext().refine_shaped(hip._net(be), logit)
            monkeypatch.setenv("FAIRIFY_REFINE_SHAPED", "0")
            assert not ext().refine_shaped(hip._net(be), logit)
        for R in ROWS:
            lo, hi = _boxes(13, R, 5 + R)
            dm = None
            if dead:
                dm = (torch.rand(R, m.n_neurons - 1, generator=torch.Generator().manual_seed(R)) < 0.2).to(cuda)
            outs = []
            for shaped in ("1", "0"):
                monkeypatch.setenv("FAIRIFY_REFINE_SHAPED", shaped)
                outs.append(be.bounds(lo.to(cuda), hi.to(cuda), mode="symbolic", keep_layers=True, fold=(PA,),
                                      dead=dm, crown=True, refine=True))
            torch.cuda.synchronize()
            _assert_equal(*outs)
