"""Discrimination-rate measurement, GPU tier: the fused kernel (csrc/rate.hip) is sound against
exact arithmetic, its resolved counts are the CPU tier's integers for every sample count, query
kind, launch split and neighbourhood, and a zoo shape agrees end to end."""
import numpy as np
import pytest
import torch

from fairify_amd.engine.rate import measure_partitions
from fairify_amd.ops import rate as R
from fairify_amd.ops import reference as ref
from fairify_amd.ops.backend import Backend

import rate_cases as C

pytestmark = pytest.mark.gpu
EMPTY = 0x7FFFFFFF


def _pa_tensors(q, lo, hi, dev):
    values = q.pa_values(lo[0].numpy().astype(np.int64), hi[0].numpy().astype(np.int64))
    return torch.from_numpy(values).to(dev), torch.from_numpy(q.pa_pairs(values)).to(dev)


def _kernel(be, q, lo, hi, pids, S, seed, dev, split=None):
    from fairify_amd.ops import hip

    values, pairs = _pa_tensors(q, lo, hi, dev)
    f, a, idx = hip.rate_counts(be, q, lo.to(dev), hi.to(dev), pids.to(dev), S, seed, values, pairs, split=split)
    return f.cpu().numpy(), a.cpu().numpy(), idx.cpu().numpy()


# TM = 1, TM = 2 (a layer crossing a tile boundary), TM = 2 three layers, zero bias, TM = 7
@pytest.mark.parametrize("name", ["8x6", "20x6", "17x9x4", "5x5", "70x6"])
def test_kernel_against_exact_arithmetic(cuda, name):
    q = C.query()
    lo, hi, pids = C.boxes()
    total_amb = 0
    for k in (0, 5):
        m = C.family_net(name, k)
        be = Backend(m, cuda)
        assert be.hip
        f, a, idx = _kernel(be, q, lo, hi, pids, C.S, C.SEED, cuda)
        ex = C.brute_flags(m, q, lo, hi, pids, C.S, C.SEED)
        brute = ex.sum(1)
        print(f"{name}/{k}: kernel certain {int(f.sum())}, ambiguous {int(a.sum())}, exact {int(brute.sum())}")
        assert (f <= brute).all() and (brute <= f + a).all()
        cpu = Backend(m, "cpu")
        values, pairs = _pa_tensors(q, lo, hi, "cpu")
        X = ref.sample_points(lo, hi, pids, C.S, C.SEED)
        _, poss = R.rate_flags_ref(cpu, q, X.reshape(-1, 5), values, pairs)
        poss = poss.view(C.P, C.S).numpy()
        for p in range(C.P):
            if a[p] <= R.AMB_SLOTS:
                row = idx[p, :a[p]]
                assert (idx[p, a[p]:] == EMPTY).all() and len(set(row.tolist())) == a[p]
                assert ((row >= 0) & (row < C.S)).all()
                assert (poss[p, row] | ex[p, row]).all()
        r = measure_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), C.S, C.SEED)
        assert np.array_equal(r.flips, f)
        assert np.array_equal(r.flips_exact, brute)
        assert np.array_equal(r.flips_exact, C.cpu_counts(name, k))
        assert not r.ambiguous_left.any()
        total_amb += int(a.sum())
    if name in C.BIAS_FAMILIES:
        assert total_amb <= 0.001 * 2 * C.P * C.S


@pytest.mark.parametrize("S", [5, 16, 70, 200])
def test_sample_count_edges(cuda, S):
    q = C.query()
    lo, hi, pids = C.boxes()
    for name, k in (("17x9x4", 2), ("5x5", 5)):
        be = Backend(C.family_net(name, k), cuda)
        f, a, idx = _kernel(be, q, lo, hi, pids, S, C.SEED, cuda)
        assert (f + a <= S).all()                                   # lanes past S count nothing
        assert ((idx == EMPTY) | ((idx >= 0) & (idx < S))).all()
        r = measure_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), S, C.SEED)
        assert np.array_equal(r.flips_exact, C.cpu_counts(name, k, S))
        if S == 200:
            assert r.flips_exact.sum() > 0


def test_overflow_rule(cuda):
    q = C.query()
    lo, hi, pids = C.ambiguous_boxes()
    be = Backend(C.ambiguous_net(), cuda)
    f, a, idx = _kernel(be, q, lo, hi, pids, 40, 3, cuda)
    assert (f == 0).all() and (a == 40).all() and (idx == EMPTY).all()   # 40 > 32 slots: row not trusted
    r = measure_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), 40, 3)
    assert (r.flips_exact == 40).all() and not r.ambiguous_left.any()
    f, a, idx = _kernel(be, q, lo, hi, pids, 20, 3, cuda)
    assert (f == 0).all() and (a == 20).all()
    assert (idx[:, :20] == np.arange(20)).all() and (idx[:, 20:] == EMPTY).all()
    r = measure_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), 20, 3)
    assert (r.flips_exact == 20).all()
    r = measure_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), 40, 3, resolve=False)
    assert (r.flips == 0).all() and (r.ambiguous_left == 40).all()


@pytest.mark.parametrize("kind", ["relaxed", "two-pa", "three-values"])
def test_query_kinds_match_cpu(cuda, kind):
    lo, hi, pids = C.boxes()
    if kind == "relaxed":
        q = C.query(("f2",), ("f1",), 1)
    elif kind == "two-pa":
        q = C.query(("f2", "f4"))
    else:
        q = C.query(("f3",))
        lo[:, 3], hi[:, 3] = 0, 2
    for name, k in (("17x9x4", 2), ("5x5", 5)):
        m = C.family_net(name, k)
        want = measure_partitions(Backend(m, "cpu"), q, lo, hi, pids, 100, C.SEED).flips_exact
        got = measure_partitions(Backend(m, cuda), q, lo.to(cuda), hi.to(cuda), pids.to(cuda), 100, C.SEED)
        assert np.array_equal(got.flips_exact, want)
        assert want.sum() > 0 and (got.flips <= want).all()


def test_neighbour_and_split_independence(cuda):
    from fairify_amd.ops import hip

    q = C.query()
    lo, hi, pids = C.boxes()
    be = Backend(C.family_net("5x5", 5), cuda)
    base = _kernel(be, q, lo, hi, pids, C.S, C.SEED, cuda, split=1)
    assert base[1].sum() > 0                                        # ambiguous profiles are in play
    assert hip.rate_split_max(C.S) == 4
    for split in range(1, hip.rate_split_max(C.S) + 1):
        got = _kernel(be, q, lo, hi, pids, C.S, C.SEED, cuda, split=split)
        assert all(np.array_equal(x, y) for x, y in zip(got, base)), split
    dflt = _kernel(be, q, lo, hi, pids, C.S, C.SEED, cuda)
    assert all(np.array_equal(x, y) for x, y in zip(dflt, base))
    for p in (0, 7, int(np.argmax(base[1])), C.P - 1):
        for split in (1, 4):
            one = _kernel(be, q, lo[p:p + 1], hi[p:p + 1], pids[p:p + 1], C.S, C.SEED, cuda, split=split)
            assert all(np.array_equal(x[0], y[p]) for x, y in zip(one, base)), (p, split)
    sub = _kernel(be, q, lo[5:9], hi[5:9], pids[5:9], C.S, C.SEED, cuda)
    assert all(np.array_equal(x, y[5:9]) for x, y in zip(sub, base))


def test_uncovered_shapes_raise(cuda):
    from fairify_amd.ops import hip

    lo, hi, pids = C.boxes()
    values, pairs = _pa_tensors(C.query(), lo, hi, cuda)
    args = (lo.to(cuda), hi.to(cuda), pids.to(cuda), 16, 0, values, pairs)
    be = Backend(C.family_net("8x6", 0), cuda)
    with pytest.raises(ValueError, match="launch-shape limit"):
        hip.rate_counts(be, C.query(("f2",), ("f0", "f1"), 3), *args)
    with pytest.raises(ValueError, match="split"):
        hip.rate_counts(be, C.query(), *args, split=2)
    from fairify_amd.models.mlp import random_mlp

    wide = Backend(random_mlp(5, [161], seed=0), cuda)
    with pytest.raises(ValueError, match="160"):
        hip.rate_counts(wide, C.query(), *args)


def test_zoo_shape_end_to_end(cuda):
    from fairify_amd.analysis.rate import measure_preset

    kw = dict(n_samples=256, max_partitions=64)
    gpu = measure_preset("src/GC-age", "GC-1", device="cuda:0", **kw)
    cpu = measure_preset("src/GC-age", "GC-1", device="cpu", **kw)
    assert gpu.keys() == cpu.keys()
    for key, want in cpu.items():
        if isinstance(want, float):
            assert gpu[key] == pytest.approx(want, abs=1e-12), key
        else:
            assert gpu[key] == want, key
    assert gpu["partitions"] == 64 and gpu["ambiguous_left"] == 0
