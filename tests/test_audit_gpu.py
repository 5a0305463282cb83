"""Audit of real individuals, GPU tier: the fused kernel (csrc/audit.hip) is sound against exact
arithmetic per bit, its resolved masks are the CPU tier's integers for every row count, query kind,
launch shape and neighbourhood, shapes it declines take the composed path, and a zoo shape agrees
end to end."""
import numpy as np
import pytest
import torch

from fairify_amd.engine.audit import audit_rows
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import audit as A
from fairify_amd.ops.backend import Backend

import audit_cases as AC
import rate_cases as C

pytestmark = pytest.mark.gpu


def _kernel(be, q, X, dev, blocks=None, own=None):
    """Raw kernel triple (cert, poss uint32, own_sign int8) as numpy, or None."""
    from fairify_amd.ops import hip

    values, pairs = A.pa_domain_table(q)
    own = A.own_index(q, X, values) if own is None else own
    out = hip.audit_masks(be, q, torch.from_numpy(X).to(dev, torch.float32), torch.from_numpy(own).to(dev),
                          torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev), blocks=blocks)
    if out is None:
        return None
    cert, poss, sign = (t.cpu().numpy() for t in out)
    return cert.view(np.uint32), poss.view(np.uint32), sign


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# TM = 1, TM = 2, TM = 2 three layers, zero bias, TM = 7, TM = 4, TM = 10
@pytest.mark.parametrize("family", ["8x6", "20x6", "17x9x4", "5x5", "70x6", "50x6", "150x6"])
def test_kernel_against_exact_arithmetic(cuda, family):
    q = C.query()
    X = AC.rows()
    total_amb = 0
    ks = (2,) if family == "17x9x4" else (0, 5)
    for k in ks:
        m = AC.net(family, k)
        be = Backend(m, cuda)
        assert be.hip
        cert, poss, sign = _kernel(be, q, X, cuda)
        brute, sx = AC.brute_masks(m, q, X)
        amb = AC.popcount(poss & ~cert)
        print(f"{family}/{k}: kernel cert bits {AC.popcount(cert)}, ambiguous bits {amb}, exact {AC.popcount(brute)}")
        assert not (cert & ~brute).any() and not (brute & ~poss).any()       # cert <= brute <= poss per bit
        has_cert = cert != 0
        assert np.array_equal(sign[has_cert], sx[has_cert]) and (sx[has_cert] != 0).all()
        assert ((sign == 0) | (sign == sx)).all()
        r = audit_rows(be, q, X)
        assert r.fused and np.array_equal(r.cert, cert) and np.array_equal(r.poss, poss)
        cpu = audit_rows(Backend(m, "cpu"), q, X)
        assert np.array_equal(r.flip_mask, cpu.flip_mask) and np.array_equal(r.flip_mask, brute)
        assert np.array_equal(r.direction, cpu.direction)
        assert not r.ambiguous_bits.any()
        total_amb += amb
    if family != "5x5":
        assert total_amb <= 0.001 * len(ks) * len(X) * 1                     # one valid v' per row (V = 2)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200])
def test_row_count_edges(cuda, N):
    q = C.query()
    for name, k in (("17x9x4", 2), ("5x5", 5)):
        m = AC.net(name, k)
        X = AC.rows()[np.arange(N) * 24].copy()                               # rows of every box
        skipped = sorted({0, N // 2})                                         # two rows outside the PA domain
        X[skipped, 2] = 5
        be = Backend(m, cuda)
        cert, poss, sign = _kernel(be, q, X, cuda)
        assert cert.shape == (N,)
        for arr in (cert, poss, sign):
            assert not arr[skipped].any()
        want = audit_rows(Backend(m, "cpu"), q, X)
        got = audit_rows(be, q, X)
        assert got.fused and (got.own[skipped] == -1).all()
        assert np.array_equal(got.flip_mask, want.flip_mask) and np.array_equal(got.direction, want.direction)
        assert not (cert & ~want.flip_mask).any() and not (want.flip_mask & ~poss).any()
        if N == 200:
            assert want.flip_mask.any()


def test_launch_shape_independence(cuda):
    from fairify_amd.ops import hip

    m, q, X = AC.case("5x5")
    be = Backend(m, cuda)
    base = _kernel(be, q, X, cuda, blocks=1)
    assert (base[1] & ~base[0]).any()                                         # ambiguous bits are in play
    passes = hip.audit_passes(len(X))
    assert passes == 75
    for blocks in (2, None, passes):
        assert _same(_kernel(be, q, X, cuda, blocks=blocks), base), blocks
    with pytest.raises(ValueError, match="workgroups"):
        _kernel(be, q, X, cuda, blocks=passes + 1)


def test_neighbour_independence(cuda):
    m, q, X = AC.case("5x5")
    be = Backend(m, cuda)
    base = _kernel(be, q, X, cuda)
    amb = np.nonzero(base[1] & ~base[0])[0]
    assert amb.size
    for i in (0, 7, int(amb[0]), len(X) - 1):
        one = _kernel(be, q, X[i:i + 1], cuda)
        assert all(x[0] == y[i] for x, y in zip(one, base)), i
        s0 = max(0, i - 37)
        sl = _kernel(be, q, X[s0:i + 20], cuda)
        assert all(np.array_equal(x, y[s0:i + 20]) for x, y in zip(sl, base)), i


def test_all_ambiguous_net(cuda):
    m, q, X = AC.case("ambiguous")
    be = Backend(m, cuda)
    cert, poss, sign = _kernel(be, q, X, cuda)
    assert not cert.any() and not sign.any()
    assert np.array_equal(poss, np.uint32(1) << (1 - X[:, 2]).astype(np.uint32))   # the one valid bit of each row
    r = audit_rows(be, q, X)
    assert (r.flip_mask != 0).all() and len(X) == 800
    assert np.array_equal(r.flip_mask, AC.cpu_audit("ambiguous").flip_mask)
    assert np.array_equal(r.direction, AC.cpu_audit("ambiguous").direction)


@pytest.mark.parametrize("name", ["relaxed", "two-pa", "three-values", "three-values-5x5"])
def test_query_kinds_match_cpu(cuda, name):
    m, q, X = AC.case(name)
    want = AC.cpu_audit(name)
    got = audit_rows(Backend(m, cuda), q, X)
    assert got.fused
    assert np.array_equal(got.flip_mask, want.flip_mask) and np.array_equal(got.direction, want.direction)
    assert not (got.cert & ~want.flip_mask).any() and not (want.flip_mask & ~got.poss).any()
    assert int((got.flip_mask != 0).sum()) == AC.CASES[name][5]
    if name in AC.BIAS_CASES:
        valid = {"relaxed": 1, "two-pa": 6, "three-values": 5}[name]         # valid v' per row
        assert AC.popcount(got.poss & ~got.cert) <= 0.001 * len(X) * valid


def test_uncovered_shapes(cuda):
    q = C.query()
    X = AC.rows()[:500]
    # 63 weight tiles plus biases: over 64 KB of LDS, the fused kernel declines, the composed path answers
    m = random_mlp(5, [100, 100], seed=3, bias_scale=0.5)
    be = Backend(m, cuda)
    assert _kernel(be, q, X, cuda) is None
    got = audit_rows(be, q, X)
    want = audit_rows(Backend(m, "cpu"), q, X)
    assert not got.fused
    assert np.array_equal(got.flip_mask, want.flip_mask) and np.array_equal(got.direction, want.direction)
    assert np.array_equal(got.flip_mask, AC.brute_masks(m, q, X)[0])
    wide = Backend(random_mlp(5, [161], seed=0), cuda)
    assert _kernel(wide, q, X, cuda) is None
    small = Backend(AC.net("8x6", 0), cuda)
    from fairify_amd.ops import hip

    values, pairs = A.pa_domain_table(q)
    args = (torch.from_numpy(X).to(cuda, torch.float32), torch.from_numpy(A.own_index(q, X, values)).to(cuda),
            torch.from_numpy(values).to(cuda), torch.from_numpy(pairs).to(cuda))
    assert hip.audit_masks(small, q, *args) is not None
    with pytest.raises(ValueError, match="launch-shape limit"):
        hip.audit_masks(small, C.query(("f2",), ("f0", "f1"), 3), *args)        # 49 offset vectors
    with pytest.raises(ValueError, match="own"):
        _kernel(small, q, X, cuda, own=np.full(len(X), 2, np.int32))


def test_zoo_shape_end_to_end(cuda, tmp_path):
    from fairify_amd import presets
    from fairify_amd.analysis.audit import audit_preset
    from fairify_amd.data import tabular

    dom = presets.get("src/GC-age").domain()
    path = tmp_path / "rows.csv"
    tabular.synthetic(dom, n=2048, seed=1).df.to_csv(path, index=False)
    gpu = audit_preset("src/GC-age", "GC-1", data=str(path), device="cuda:0")
    cpu = audit_preset("src/GC-age", "GC-1", data=str(path), device="cpu")
    assert gpu == cpu
    assert gpu["rows"] == 2048 and gpu["audited"] == 2048 and gpu["ambiguous_left"] == 0
