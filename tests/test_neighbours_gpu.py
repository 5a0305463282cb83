"""Single-attribute neighbourhoods, GPU tier: the fused kernel (csrc/neighbours.hip) is sound against
the oracle per bit, its resolved bits are the CPU tier's integers for every tile count, word and row
count, launch shape, batch, query kind and table kind, shapes it declines take the composed path, and
a zoo shape agrees end to end."""
import numpy as np
import pytest
import torch

from fairify_amd.engine.neighbours import audit_neighbours, exposure
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import audit as A
from fairify_amd.ops import neighbours as NB
from fairify_amd.ops.backend import Backend

import audit_cases as AC
import neighbour_cases as NC
import rate_cases as C

pytestmark = pytest.mark.gpu


def _kernel(be, q, X, dev, table=None, blocks=None):
    """Raw kernel pair (cert, poss uint32 [N, W]) as numpy, or None."""
    from fairify_amd.ops import hip

    table = NB.neighbour_table(q) if table is None else table
    values, pairs = A.pa_domain_table(q)
    own = A.own_index(q, X, values)
    out = hip.neighbour_masks(be, q, torch.from_numpy(X).to(dev, torch.float32), torch.from_numpy(own).to(dev),
                              torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev), table, blocks=blocks)
    if out is None:
        return None
    return tuple(t.cpu().numpy().view(np.uint32) for t in out)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check(m, q, X, cuda, radii=None, oracle_radii=None, cap=True):
    """Kernel, resolved GPU result and CPU tier against the oracle; returns (gpu result, oracle flag)."""
    be = Backend(m, cuda)
    assert be.hip
    flag, valid, delta, own, feat = NC.oracle(m, q, X, oracle_radii)
    table = NB.neighbour_table(q, radii)
    M = table.M
    assert M == flag.shape[1]
    cert, poss = _kernel(be, q, X, cuda, table)
    assert cert.shape == (len(X), (M + 31) // 32)
    c, p = NC.bits(cert, M), NC.bits(poss, M)
    amb = int((p & ~c).sum())
    print(f"M {M}: kernel cert bits {int(c.sum())}, ambiguous bits {amb}, exact {int(flag.sum())}, "
          f"valid {int(valid.sum())}")
    assert not (c & ~flag).any() and not (flag & ~p).any()              # cert <= oracle <= poss per bit
    assert not (p & ~valid).any() and NC.padding_clear(cert, M) and NC.padding_clear(poss, M)
    r = audit_neighbours(be, q, X, radii=radii)
    assert r.fused and np.array_equal(r.cert, cert) and np.array_equal(r.poss, poss)
    cpu = audit_neighbours(Backend(m, "cpu"), q, X, radii=radii)
    assert np.array_equal(r.flag, cpu.flag) and np.array_equal(NC.bits(r.flag, M), flag)
    assert r.ambiguous == amb and r.ambiguous_left == 0
    if cap:
        assert amb <= 0.001 * int(valid.sum())
    return r, flag


# TM = 1, TM = 2, TM = 2 three layers, TM = 4, TM = 7, TM = 10, zero bias
@pytest.mark.parametrize("family", ["8x6", "20x6", "17x9x4", "50x6", "70x6", "150x6", "5x5"])
def test_kernel_against_oracle(cuda, family):
    k = NC.TILE_SEEDS[family][0] if family in NC.TILE_SEEDS else 2 if family == "17x9x4" else 5
    r, flag = _check(AC.net(family, k), C.query(), NC.rows(), cuda, cap=family != "5x5")
    assert flag.any()
    if family in NC.TILE_SEEDS:
        assert int(flag.sum()) == NC.TILE_SEEDS[family][1]
    if family in NC.CASES:
        assert int(flag.sum()) == NC.CASES[family][6]


def test_all_ambiguous_net(cuda):
    m, q = C.ambiguous_net(), C.query()
    X = AC.rows(ambiguous=True)[::4].copy()
    be = Backend(m, cuda)
    cert, poss = _kernel(be, q, X, cuda)
    Z, valid = NB.neighbour_rows(q, X, NB.neighbour_table(q))
    assert not cert.any() and np.array_equal(NC.bits(poss, 28), valid)
    r = audit_neighbours(be, q, X)
    flag = NC.oracle(m, q, X)[0]
    assert r.fused and r.ambiguous == int(valid.sum()) and np.array_equal(NC.bits(r.flag, 28), flag)
    assert np.array_equal(flag, valid)                                    # every neighbour flips


# half a word (radius 2), 28 bits, one full word, two words with the second partial
@pytest.mark.parametrize("M", [16, 28, 32, 42])
def test_word_edges(cuda, M):
    m = AC.net("17x9x4", 2)
    X = NC.rows()[:200]
    if M == 16:
        q, radii, orad = C.query(), 2, {k: 2 for k in range(5)}
    else:
        q, radii, orad = (C.query() if M == 28 else NC.wide_query(M - 22)), None, None
    r, flag = _check(m, q, X, cuda, radii, orad)
    assert r.table.M == M and r.flag.shape[1] == (2 if M == 42 else 1) and flag.any()
    if M == 42:
        assert flag[:, 32:].any() and flag[:, :32].any()


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200])
def test_row_count_edges(cuda, N):
    q = C.query()
    for name, k in (("17x9x4", 2), ("5x5", 5)):
        m = AC.net(name, k)
        X = NC.rows()[np.arange(N) * 3].copy()                            # rows of every box
        skipped = sorted({0, N // 2})                                     # two rows outside the PA domain
        X[skipped, 2] = 5
        be = Backend(m, cuda)
        cert, poss = _kernel(be, q, X, cuda)
        assert cert.shape == (N, 1) and not cert[skipped].any() and not poss[skipped].any()
        want = audit_neighbours(Backend(m, "cpu"), q, X)
        got = audit_neighbours(be, q, X)
        assert got.fused and (got.own[skipped] == -1).all()
        assert np.array_equal(got.flag, want.flag)
        assert not (cert & ~want.flag).any() and not (want.flag & ~poss).any()
        assert np.array_equal(NC.bits(got.flag, 28), NC.oracle(m, q, X)[0])
        if N == 200:
            assert want.flag.any()


def test_launch_shape_independence(cuda):
    from fairify_amd.ops import hip

    m = AC.net("5x5", 5)
    q = NC.wide_query(20)                                                 # two words
    X = NC.rows()
    be = Backend(m, cuda)
    base = _kernel(be, q, X, cuda, blocks=1)
    assert (base[1] & ~base[0]).any()                                     # ambiguous bits are in play
    items = hip.neighbour_items(len(X), 42)
    assert items == 10 * 2
    for blocks in (2, None, items):
        assert _same(_kernel(be, q, X, cuda, blocks=blocks), base), blocks
    with pytest.raises(ValueError, match="workgroups"):
        _kernel(be, q, X, cuda, blocks=items + 1)


def test_batch_independence(cuda):
    m, q, X = NC.case("5x5")
    be = Backend(m, cuda)
    base = _kernel(be, q, X, cuda)
    amb = np.nonzero((base[1] & ~base[0]).any(axis=1))[0]
    assert amb.size
    for i in (0, 7, int(amb[0]), len(X) - 1):
        one = _kernel(be, q, X[i:i + 1], cuda)
        assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, base)), i
        s0 = max(0, i - 37)
        sl = _kernel(be, q, X[s0:i + 20], cuda)
        assert all(np.array_equal(x, y[s0:i + 20]) for x, y in zip(sl, base)), i


@pytest.mark.parametrize("name", ["relaxed", "two-pa", "three-values", "three-values-5x5"])
def test_query_kinds_match_cpu(cuda, name):
    m, q, X = NC.case(name)
    want = NC.cpu_result(name)
    got = audit_neighbours(Backend(m, cuda), q, X)
    M = want.table.M
    flag, valid, delta, own, feat = NC.oracle_case(name)
    assert got.fused and np.array_equal(got.flag, want.flag) and np.array_equal(NC.bits(got.flag, M), flag)
    assert not (got.cert & ~want.flag).any() and not (want.flag & ~got.poss).any()
    ex = exposure(got, X, own)
    _, _, _, _, M_pin, classes, neighbours = NC.CASES[name]
    assert M == M_pin and int(ex.count.sum()) == neighbours
    assert (int(ex.flagged.sum()), int(ex.exposed.sum()), int(ex.robust.sum())) == classes
    if name in NC.BIAS_CASES:
        assert got.ambiguous <= 0.001 * int(valid.sum())


def test_relative_and_absolute_entries(cuda):
    m, q, X = NC.case("20x6")
    r, flag = _check(m, q, X, cuda, {"f0": 1}, {0: 1})
    assert r.table.abs.tolist() == [0, 0] + [1] * 21 and flag[:, :2].any() and flag[:, 2:].any()
    X = X[:64].copy()
    X[5, 0], X[6, 1], X[7, 4] = 40, -3, 9                                 # non-PA coordinates outside their range
    _check(m, q, X, cuda, {"f0": 1, "f4": 2}, {0: 1, 4: 2})


def test_uncovered_shapes(cuda):
    q = C.query()
    X = NC.rows()[:500]
    # over 64 KB of LDS: the fused kernel declines, the composed path answers
    m = random_mlp(5, [100, 100], seed=3, bias_scale=0.5)
    be = Backend(m, cuda)
    assert _kernel(be, q, X, cuda) is None
    got = audit_neighbours(be, q, X)
    want = audit_neighbours(Backend(m, "cpu"), q, X)
    assert not got.fused and np.array_equal(got.flag, want.flag)
    assert np.array_equal(NC.bits(got.flag, 28), NC.oracle(m, q, X)[0])
    assert _kernel(Backend(random_mlp(5, [161], seed=0), cuda), q, X, cuda) is None


def test_switch_selects_the_composed_path(cuda, monkeypatch):
    m, q, X = NC.case("20x6")
    be = Backend(m, cuda)
    monkeypatch.setenv("FAIRIFY_NEIGHBOURS_FUSED", "0")
    composed = audit_neighbours(be, q, X)
    monkeypatch.delenv("FAIRIFY_NEIGHBOURS_FUSED")
    fused = audit_neighbours(be, q, X)
    assert fused.fused and not composed.fused and np.array_equal(fused.flag, composed.flag)
    assert np.array_equal(fused.flag, NC.cpu_result("20x6").flag)


def test_zoo_shape_end_to_end(cuda, tmp_path):
    from fairify_amd import presets
    from fairify_amd.analysis.audit import audit_preset
    from fairify_amd.data import tabular

    dom = presets.get("src/GC-age").domain()
    path = tmp_path / "rows.csv"
    tabular.synthetic(dom, n=2048, seed=1).df.to_csv(path, index=False)
    kw = dict(data=str(path), neighbours=True, radius_of={"credit_amount": 3, "month": 5})
    gpu = audit_preset("src/GC-age", "GC-1", device="cuda:0", **kw)
    cpu = audit_preset("src/GC-age", "GC-1", device="cpu", **kw)
    assert gpu == cpu
    s = gpu["neighbours"]
    assert s["audited"] == 2048 and s["ambiguous_left"] == 0
    assert s["flagged"] + s["exposed"] + s["robust"] == 2048
