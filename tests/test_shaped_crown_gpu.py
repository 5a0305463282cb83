"""Compile-time-shape instances of the backward output pass (csrc/crown.hip, fa_crown_mfma_kernel<TM,
FaShape<...>>) against the run-time-shape kernel they specialise: every output bitwise equal, through
the Python entry (row boxes) and through the native BaB level (node rows, V = 2).  One shape is also
held against the fp64 reference and against exact logits."""
import numpy as np
import pytest
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import reference as ref
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

PA = 8                      # Adult's protected attribute (sex): pinned per row, folded by the forward pass
# every instantiated shape (hidden widths, 13 inputs, one logit), then one the table does not hold
SHAPED = [[100, 100], [100], [64, 64], [50], [5, 5], [16, 8], [12, 12], [3, 3, 3, 3]]
FALLBACK = [17, 3]
# 1: one valid row in the tile; 15 / 16 / 17: around a full tile; 701: several workgroups, odd tail
ROWS = (1, 15, 16, 17, 701)
FIELDS = ("out_lb", "out_ub", "Lc", "Uc", "L0", "U0", "Le", "Ue")


def _boxes(n0, R, seed):
    g = np.random.default_rng(seed)
    lo = g.integers(-5, 20, size=(R, n0)).astype(np.float32)
    hi = lo + g.integers(0, 6, size=(R, n0)).astype(np.float32)
    hi[:, PA] = lo[:, PA] = (np.arange(R) % 2).astype(np.float32)     # the V = 2 node rows of a BaB level
    return torch.from_numpy(lo), torch.from_numpy(hi)


def _ident(h):
    return "13," + ",".join(map(str, h)) + ",1"


@pytest.mark.parametrize("dead", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("hidden", SHAPED + [FALLBACK], ids=_ident)
def test_shaped_crown_is_bitwise_the_generic_one(cuda, monkeypatch, hidden, dead):
    from fairify_amd.ops import ext, hip

    # zero biases (the bench's random-init nets: exact zeros decide partitions) and non-zero ones
    for bias in (0.0, 0.3):
        m = random_mlp(13, hidden, seed=53 + len(hidden) + hidden[0], bias_scale=bias)
        be = Backend(m, cuda)
        assert be.hip
        # the launch's own selection: a shaped instance for every listed shape, none with the switch
        # off; the fallback shape has none, both runs take the run-time-shape kernel and agree trivially
        monkeypatch.setenv("FAIRIFY_CROWN_SHAPED", "1")
        assert ext().crown_shaped(hip._net(be), dead) == (hidden != FALLBACK)
        monkeypatch.setenv("FAIRIFY_CROWN_SHAPED", "0")
        assert not ext().crown_shaped(hip._net(be), dead)
        for R in ROWS:
            lo, hi = _boxes(13, R, 23 + R)
            dm = None
            if dead:
                dm = (torch.rand(R, m.n_neurons - 1, generator=torch.Generator().manual_seed(R)) < 0.2).to(cuda)
            outs = []
            for shaped in ("1", "0"):
                monkeypatch.setenv("FAIRIFY_CROWN_SHAPED", shaped)
                outs.append(be.bounds(lo.to(cuda), hi.to(cuda), mode="symbolic", crown=True, fold=(PA,), dead=dm))
            torch.cuda.synchronize()
            for f in FIELDS:
                assert torch.equal(getattr(outs[0], f), getattr(outs[1], f)), (f, R, bias)


def test_shaped_crown_against_fp64_reference(cuda):
    """13-100-100-1 (the shaped 7-tile instance, the default): logit bounds within the existing crown
    test's tolerance of ops/reference.py in fp64, never looser than the forward pass, and the forms
    bound exact fp64 logits on sampled lattice points of every box."""
    m = random_mlp(13, [100, 100], seed=61, bias_scale=0.3)
    lo, hi = _boxes(13, 257, 9)
    gpu = Backend(m, cuda)
    rg = gpu.bounds(lo.to(cuda), hi.to(cuda), mode="symbolic", crown=True, fold=(PA,))
    rf = gpu.bounds(lo.to(cuda), hi.to(cuda), mode="symbolic", fold=(PA,))
    cpu = Backend(m, "cpu")
    ws, bs = [w.double() for w in cpu.ws], [b.double() for b in cpu.bs]
    rr = ref.bounds(ws, bs, lo.double(), hi.double(), mode="symbolic", unit=ref.FP32_UNIT, keep_layers=True)
    rr = ref.crown_output(ws, bs, lo.double(), hi.double(), rr, None, unit=ref.FP32_UNIT)
    scale = float(((rr.out_ub - rr.out_lb).abs() + rr.out_ub.abs()).max() + 1e-3)
    assert torch.allclose(rg.out_lb.cpu().double(), rr.out_lb, rtol=1e-3, atol=1e-3 * scale)
    assert torch.allclose(rg.out_ub.cpu().double(), rr.out_ub, rtol=1e-3, atol=1e-3 * scale)
    assert bool((rg.out_lb >= rf.out_lb).all()) and bool((rg.out_ub <= rf.out_ub).all())
    g = np.random.default_rng(2)
    lo_i, hi_i = lo.numpy().astype(np.int64), hi.numpy().astype(np.int64)
    pts = g.integers(lo_i[:, None, :], hi_i[:, None, :] + 1, size=(257, 32, 13))
    z = m.logits(pts.reshape(-1, 13).astype(np.float64)).reshape(257, 32)
    X = torch.from_numpy(pts).double()
    dn = torch.einsum("rsk,rk->rs", X, rg.Lc.cpu().double()) + (rg.L0 - rg.Le).cpu().double()[:, None]
    up = torch.einsum("rsk,rk->rs", X, rg.Uc.cpu().double()) + (rg.U0 + rg.Ue).cpu().double()[:, None]
    assert (dn.numpy() <= z + 1e-9).all() and (up.numpy() >= z - 1e-9).all()
    assert (z >= rg.out_lb.cpu().double().numpy()[:, None]).all() and (z <= rg.out_ub.cpu().double().numpy()[:, None]).all()


@pytest.mark.parametrize("name", ["AC-3", "AC-8"])
def test_shaped_crown_in_the_native_bab_level(cuda, monkeypatch, name):
    """The BaB runtime's crown launches (node rows: V = 2, the PA value substituted in the kernel) with
    the shaped instance and with the run-time-shape kernel: the same search, node for node."""
    from fairify_amd import presets
    from fairify_amd.engine.bab import BaBConfig, BaBSolver
    from fairify_amd.models.zoo import get_model
    from fairify_amd.partition import processing_order

    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    lo, hi = grid.decode(processing_order(grid, 0)[:64])
    m = get_model(name, weights="random", seed=0)
    be = Backend(m, cuda)
    out = []
    for shaped in ("1", "0"):
        monkeypatch.setenv("FAIRIFY_CROWN_SHAPED", shaped)
        out.append(BaBSolver(be, q, BaBConfig(node_budget=256)).solve(lo, hi, m))
    a, b = out
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.nodes, b.nodes)
    assert np.array_equal(a.open_left, b.open_left)
    assert np.array_equal(a.cex_x, b.cex_x) and np.array_equal(a.cex_xp, b.cex_xp)
