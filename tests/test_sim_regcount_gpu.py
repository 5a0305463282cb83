"""Compile-time-shape simulation kernels (activation counts in registers, one flush per workgroup;
``fa_sim_reg_kernel<TM, FaShape<...>>``) against the run-time-shape kernel of the same tile depth
(``FAIRIFY_SIM_REGCOUNT=0``), both in one process: counts equal as integers, found equal, witnesses
and z0 bitwise equal.  One case per tile count is also checked against the exact reference the way
``tests/test_kernels_gpu.py::test_sim_kernel_matches_reference`` does it.

The nets have random weights and non-zero biases of both signs (the zoo's random-init nets are
zero-bias).  The simulation launch takes no dead mask (``SimArgs`` has none: pruning happens after
it), so there is no dead-mask case.
"""
import numpy as np
import pytest
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import reference as ref
from fairify_amd.ops.backend import Backend
from fairify_amd.spec import ADULT, Query

pytestmark = pytest.mark.gpu

# one instantiated shape per tile count (1 partial, 1 full, 4 with a partial chain, 7 one layer, 7 two layers)
SHAPED = [[5, 5], [16, 8], [64, 32, 16, 8, 4], [100], [100, 100]]
FALLBACK = [17, 3]          # partial tiles, not instantiated
N_SAMPLES = [1, 63, 64, 65, 1000]
P = 3


def _query(kind):
    if kind == "sex":
        return Query(("sex",)).resolve(ADULT)
    if kind == "race":
        return Query(("race",)).resolve(ADULT)
    return Query(("sex",), ("age",), 2).resolve(ADULT)      # relaxed: nra > 0


def _setup(cuda, q, ids):
    from fairify_amd.partition import Grid

    grid = Grid.reference(ADULT, 10)
    lo, hi = grid.decode(ids)
    values = q.pa_values(lo[0], hi[0])
    pairs = q.pa_pairs(values)
    return (lo, hi, values, pairs, torch.from_numpy(lo).float().to(cuda), torch.from_numpy(hi).float().to(cuda),
            torch.from_numpy(ids).to(cuda), torch.from_numpy(values).to(cuda), torch.from_numpy(pairs).to(cuda))


def _both(monkeypatch, be, q, lo_t, hi_t, pid, S, seed, values, pairs):
    """(register counters, run-time-shape kernel) results of one launch each, z0 requested."""
    from fairify_amd.ops import hip

    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("FAIRIFY_SIM_REGCOUNT", flag)
        out.append(hip.simulate(be, q, lo_t, hi_t, pid, S, seed, values, pairs, 0, 0, return_z0=True))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(a, b, what):
    assert torch.equal(a.counts, b.counts), what
    assert torch.equal(a.found, b.found), what
    assert torch.equal(_bits(a.wit_x), _bits(b.wit_x)), what
    assert torch.equal(_bits(a.wit_xp), _bits(b.wit_xp)), what
    assert torch.equal(_bits(a.z0), _bits(b.z0)), what


@pytest.mark.parametrize("hidden", SHAPED + [FALLBACK], ids=lambda h: "13," + ",".join(map(str, h)) + ",1")
def test_sim_regcount_equals_runtime_shape_kernel(cuda, monkeypatch, hidden):
    from fairify_amd.ops import ext, hip

    m = random_mlp(13, hidden, seed=11 + len(hidden), bias_scale=0.5)
    assert all((b > 0).any() and (b < 0).any() for b in m.biases[:-1]) and m.biases[-1][0] != 0
    be = Backend(m, cuda)
    assert be.hip
    # the fallback shape has no instance: both runs take the run-time-shape kernel and agree trivially
    assert ext().sim_shaped(hip._net(be)) == (hidden != FALLBACK)
    monkeypatch.setattr(hip, "_SIM_REGCOUNT_ENV", "dynamic")
    monkeypatch.setattr(hip, "_SIM_BLOCKS_ENV", "dynamic")
    ids = np.array([5, 4321, 15999])
    assert len(ids) == P
    n_counted = 0
    for kind in ("sex", "race", "relaxed"):
        q = _query(kind)
        _, _, values, pairs, lo_t, hi_t, pid, values_t, pairs_t = _setup(cuda, q, ids)
        assert (len(values), len(pairs)) == ((5, 20) if kind == "race" else (2, 2))
        for S in N_SAMPLES:
            for blocks in ("0", str(3 * P)):                   # split 1, split min(3, sample tiles)
                monkeypatch.setenv("FAIRIFY_SIM_BLOCKS", blocks)
                split = hip._sim_split(P, S)
                assert split == (1 if blocks == "0" else min(3, (S + 63) // 64))
                a, b = _both(monkeypatch, be, q, lo_t, hi_t, pid, S, 7, values_t, pairs_t)
                _assert_same(a, b, (kind, S, split))
                n_counted += int(a.counts.sum())
    assert n_counted > 0


@pytest.mark.parametrize("hidden", SHAPED, ids=lambda h: "13," + ",".join(map(str, h)) + ",1")
def test_sim_regcount_matches_reference(cuda, hidden):
    """The register-counter kernel against exact (fp64) evaluation of the same counter-hash samples:
    counts differ from the exact ones by at most the number of samples whose pre-activation interval
    contains 0; the first flip is the exact first flip unless a sample at or before it has an
    ambiguous logit sign."""
    from fairify_amd.engine.sim import simulate
    from fairify_amd.ops import ext, hip

    q = _query("race")
    ids = np.arange(0, 16000, 497)[:32]
    lo, hi, values, pairs, lo_t, hi_t, pid, values_t, pairs_t = _setup(cuda, q, ids)
    # net seed 17: with it the fp64 logits of all five shapes are sign-unambiguous on >= 90 % of these
    # partitions (a property of the inputs, evaluated with the CPU reference), so the check below is
    # not skipped for most of them
    m = random_mlp(13, hidden, seed=17, bias_scale=0.5)
    gpu = Backend(m, cuda)
    assert hip._SIM_REGCOUNT and ext().sim_shaped(hip._net(gpu))
    S, seed = 130, 5
    b = simulate(gpu, q, lo_t, hi_t, pid, S, seed, values_t, pairs_t, 0, 0)
    X = ref.sample_points(lo_t.cpu(), hi_t.cpu(), pid.cpu(), S, seed)                # [P, S, n0]
    Pn, n0 = lo.shape
    Xf = X.reshape(-1, n0)
    acts = m.layer_outputs(Xf.numpy().astype(np.float64))
    iv = gpu.bounds(Xf.to(cuda), Xf.to(cuda), mode="ibp", keep_layers=True)
    cnt_b = b.counts.cpu().numpy()
    off = 0
    for l, w in enumerate(m.widths[:-1]):
        exact = (acts[l] > 0).reshape(Pn, S, w).sum(1)
        amb = ((iv.layer_lb[l] <= 0) & (iv.layer_ub[l] >= 0)).cpu().numpy().reshape(Pn, S, w).sum(1)
        assert (np.abs(cnt_b[:, off:off + w] - exact) <= amb).all(), l
        off += w
    V = len(values)
    XV = np.repeat(X.numpy()[:, :, None, :], V, axis=2)
    XV[:, :, :, list(q.pa_idx)] = values[None, None]
    XVf = XV.reshape(-1, n0)
    z = m.logits(XVf.astype(np.float64)).reshape(Pn, S, V)
    lb, ub = gpu.point_bounds(torch.from_numpy(XVf).float().to(cuda))
    amb = ((lb <= 0) & (ub >= 0)).cpu().numpy().reshape(Pn, S, V).any(axis=2)
    zi, zj = z[:, :, pairs[:, 0]], z[:, :, pairs[:, 1]]
    flip = ((zi < 0) & (zj > 0)) | ((zi > 0) & (zj < 0))
    found_b = b.found.cpu().numpy()
    wx, wxp = b.wit_x.cpu().numpy(), b.wit_xp.cpu().numpy()
    checked = 0
    for p in range(Pn):
        fl = np.nonzero(flip[p].reshape(-1))[0]
        key = int(fl[0]) if fl.size else S * len(pairs)
        s_key = key // len(pairs)
        if amb[p, :min(S, s_key + 1)].any():
            continue
        checked += 1
        assert bool(found_b[p]) == bool(fl.size)
        if fl.size:
            s, qi = divmod(key, len(pairs))
            assert np.array_equal(wx[p], XV[p, s, pairs[qi, 0]]) and np.array_equal(wxp[p], XV[p, s, pairs[qi, 1]])
    assert checked >= 0.9 * Pn
