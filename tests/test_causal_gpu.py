"""Causal search over attribute sets, GPU tier: the fused kernel (csrc/causal.hip) is sound against the
oracle per byte for every kernel instance, its resolved bits are the oracle's, its bytes do not depend
on the row count, the launch shape, the order or grouping of the sets or the early exit, shapes it
declines take the composed path, and the search and the command agree with the CPU tier."""
import numpy as np
import pytest
import torch

from fairify_amd.engine.causal import causal_search
from fairify_amd.models.mlp import MLP, random_mlp
from fairify_amd.ops import causal as CS
from fairify_amd.ops.backend import Backend

import audit_cases as AC
import causal_cases as CC
import rate_cases as C

pytestmark = pytest.mark.gpu

TABLE = CS.table_of(CC.LISTS, CC.SETS)


def _kernel(be, X, dev, table=TABLE, blocks=None):
    """Raw kernel bytes uint8 [S, T] as numpy, or None."""
    from fairify_amd.ops import hip

    out = hip.causal_codes(be, torch.from_numpy(np.asarray(X)).to(dev, torch.float32), table, blocks=blocks)
    return None if out is None else out.cpu().numpy()


def _fused(monkeypatch, on=True):
    """The default path (the fused kernel), or the composed one."""
    monkeypatch.delenv("FAIRIFY_CAUSAL_FUSED", raising=False)
    if not on:
        monkeypatch.setenv("FAIRIFY_CAUSAL_FUSED", "0")


# TM = 1, TM = 2, TM = 2 three layers, TM = 4, TM = 7, TM = 10
@pytest.mark.parametrize("family,k", CC.TILE_NETS)
def test_kernel_against_oracle(cuda, monkeypatch, family, k):
    m = AC.net(family, k)
    pinned = (family, k) in CC.COUNTS
    X = CC.rows() if pinned else CC.rows()[::3]            # the wide nets: 200 rows (three passes and a ragged one)
    be = Backend(m, cuda)
    assert be.hip
    want = CC.oracle_case(family, k) if pinned else CC.oracle(m, X)
    code = _kernel(be, X, cuda)
    assert code.shape == (len(X), 30) and code.dtype == np.uint8 and set(np.unique(code)) <= {0, 1, 3}
    cert, poss = (code & 2) != 0, (code & 1) != 0
    amb = int((code == 1).sum())
    print(f"{family}: cert bytes {int(cert.sum())}, left to the host {amb} of {code.size}, exact {int(want.sum())}")
    assert not (cert & ~want).any() and not (want & ~poss).any()            # cert <= oracle <= poss per byte
    ref = CS.causal_codes_ref(Backend(m, "cpu"), torch.from_numpy(X), TABLE).numpy()
    assert not (cert & ~((ref & 1) != 0)).any() and not (((ref & 2) != 0) & ~poss).any()
    assert amb <= 0.001 * code.size
    _fused(monkeypatch)
    r = causal_search(be, CC.LISTS, X, max_size=4, threshold=2.0)
    assert r.fused and r.ambiguous == amb and [s.dims for s in r.sets] == CC.SETS
    assert all(np.array_equal(r.flip[s], want[:, t]) for t, s in enumerate(CC.SETS))
    assert want.any() and not want.all()
    if pinned:
        assert [s.flips_all for s in r.sets] == CC.COUNTS[(family, k)]


def test_zero_bias_net_resolves_to_the_oracle(cuda, monkeypatch):
    m, X = AC.net("5x5", 5), CC.rows()
    be = Backend(m, cuda)
    code = _kernel(be, X, cuda)
    want = CC.oracle_case("5x5", 5)
    assert not (((code & 2) != 0) & ~want).any() and not (want & ~((code & 1) != 0)).any()
    assert (code == 1).any()                                               # ambiguous bytes are in play
    _fused(monkeypatch)
    r = causal_search(be, CC.LISTS, X, max_size=4, threshold=2.0)
    assert r.fused and [s.flips_all for s in r.sets] == CC.COUNTS[("5x5", 5)]


@pytest.mark.parametrize("S", [1, 15, 16, 17, 63, 64, 65, 130])
def test_row_count_edges(cuda, S):
    for family, k in (("17x9x4", 2), ("5x5", 5)):
        be = Backend(AC.net(family, k), cuda)
        X = CC.rows()[380:510]                                             # rows 13 and 16: ambiguous on 5x5
        full = _kernel(be, X, cuda)
        assert full.any() and ((full == 1).any() or family != "5x5")
        assert np.array_equal(_kernel(be, X[:S], cuda), full[:S]), (family, S)


def test_launch_shape_independence(cuda):
    from fairify_amd.ops import hip

    be = Backend(AC.net("5x5", 5), cuda)
    X = CC.rows()[330:460]                                                 # with the two ambiguous rows
    items = hip.causal_items(130, 30)
    assert items == 3 * 30
    base = _kernel(be, X, cuda)
    assert (base == 1).any() and (base == 3).any()
    for blocks in (1, 2, 3, items - 1, items):
        assert np.array_equal(_kernel(be, X, cuda, blocks=blocks), base), blocks
    for blocks in (0, items + 1):
        with pytest.raises(ValueError, match="workgroups"):
            _kernel(be, X, cuda, blocks=blocks)


def test_set_order_and_grouping(cuda):
    be = Backend(AC.net("5x5", 5), cuda)
    X = CC.rows()[300:500]
    base = _kernel(be, X, cuda)
    assert (base == 1).any()
    perm = np.random.default_rng(0).permutation(30)
    assert np.array_equal(_kernel(be, X, cuda, table=TABLE.select(perm)), base[:, perm])
    for idx in (np.arange(0, 30, 3), np.array([29]), np.array([7, 2]), np.arange(25, 30)):
        assert np.array_equal(_kernel(be, X, cuda, table=TABLE.select(idx)), base[:, idx]), idx


def _step_net() -> MLP:
    """5 -> 1 -> 1: logit relu(x0) - 0.5, label [x0 >= 1]."""
    W0 = np.zeros((5, 1), np.float32)
    W0[0, 0] = 1.0
    return MLP([W0, np.ones((1, 1), np.float32)], [np.zeros(1, np.float32), np.array([-0.5], np.float32)], name="step")


def test_early_exit_changes_nothing(cuda):
    m = _step_net()
    X = CC.rows()
    X = X[X[:, 0] >= 1][:100]                                              # x0 := 0 flips every row
    assert len(X) == 100
    be = Backend(m, cuda)
    first = _kernel(be, X, cuda)                                           # f0's list is 0 .. 6: the first flips
    off0, off1 = int(TABLE.voff[0]), int(TABLE.voff[1])
    vals = TABLE.vals.copy()
    vals[off0:off1] = vals[off0:off1][::-1]                                # 6 .. 0: the last one does
    last = _kernel(be, X, cuda, table=CS.SetTable(dims=TABLE.dims, count=TABLE.count, vals=vals, voff=TABLE.voff))
    assert np.array_equal(first, last)
    has0 = np.array([0 in s for s in CC.SETS])
    assert (first[:, has0] == 3).all() and (first[:, ~has0] == 0).all()
    assert np.array_equal(first != 0, CC.oracle(m, X))


def test_all_ambiguous_net(cuda, monkeypatch):
    m = C.ambiguous_net()
    X = AC.rows(ambiguous=True)[::8].copy()
    be = Backend(m, cuda)
    code = _kernel(be, X, cuda)
    has2 = np.array([2 in s for s in CC.SETS])
    # fp32 decides no point: every f2 byte is left to the host (and no byte anywhere is certain)
    assert (code[:, has2] == 1).all() and not (code & 2).any()
    _fused(monkeypatch)
    r = causal_search(be, CC.LISTS, X, max_size=4, threshold=2.0)
    assert r.fused and r.ambiguous == int((code == 1).sum()) >= len(X) * int(has2.sum())
    assert [s.flips_all for s in r.sets] == [len(X) if h else 0 for h in has2]


def test_declined_shapes_take_the_composed_path(cuda, monkeypatch):
    _fused(monkeypatch)
    # over 64 KB of LDS
    m = random_mlp(5, [100, 100], seed=3, bias_scale=0.5)
    X = CC.rows()[:200]
    be = Backend(m, cuda)
    assert _kernel(be, X, cuda) is None
    got = causal_search(be, CC.LISTS, X, max_size=3, threshold=2.0)
    want = causal_search(Backend(m, "cpu"), CC.LISTS, X, max_size=3, threshold=2.0)
    assert not got.fused and got.sets == want.sets
    assert all(np.array_equal(got.flip[s], want.flip[s]) for s in CC.SETS3)
    assert np.array_equal(np.stack([got.flip[s] for s in CC.SETS3], 1), CC.oracle(m, X, CC.SETS3))
    assert _kernel(Backend(random_mlp(5, [161], seed=0), cuda), X, cuda) is None
    # more than 32 inputs: a synthetic 40-input toy
    m = random_mlp(40, [8, 6], seed=1, bias_scale=0.5)
    lists = [list(range(2 + k % 3)) for k in range(40)]
    sets = [(0,), (17,), (39,), (3, 38), (10, 11)]
    X = CS.draw_base(lists, 150, 5)
    be = Backend(m, cuda)
    assert _kernel(be, X, cuda, table=CS.table_of(lists, sets)) is None
    got = causal_search(be, lists, X, sets=sets, threshold=2.0)
    want = causal_search(Backend(m, "cpu"), lists, X, sets=sets, threshold=2.0)
    assert not got.fused and got.sets == want.sets
    assert np.array_equal(np.stack([got.flip[s] for s in sets], 1), CC.oracle(m, X, sets, lists))


@pytest.mark.parametrize("fused", [False, True])
def test_search_matches_cpu(cuda, monkeypatch, fused):
    _fused(monkeypatch, fused)
    for (family, k), base, size in ((("20x6", 5), CC.rows(), 3), (("5x5", 5), (300, 11), 2)):
        m = AC.net(family, k)
        kw = dict(max_size=size, threshold=0.3, min_samples=50, max_assignments=300)
        got = causal_search(Backend(m, cuda), CC.LISTS, base, **kw)
        want = causal_search(Backend(m, "cpu"), CC.LISTS, base, **kw)
        assert got.fused == fused
        assert got.sets == want.sets and got.minimal == want.minimal and got.minimal
        assert np.array_equal(got.X, want.X) and got.flip.keys() == want.flip.keys()
        assert all(np.array_equal(got.flip[s], want.flip[s]) for s in want.flip)
        assert {r.status for r in got.sets} >= {"tested", "implied"}


def test_cli_matches_cpu_bytes(cuda, monkeypatch, tmp_path):
    from fairify_amd import cli

    _fused(monkeypatch)
    args = ["causal", "--preset", "src/GC-age", "--model", "GC-1", "--samples", "300", "--max-size", "2",
            "--values", "domain", "--max-values", "6"]
    cli.main(args + ["--device", "cuda:0", "--out", str(tmp_path / "gpu")])
    cli.main(args + ["--device", "cpu", "--out", str(tmp_path / "cpu")])
    a, b = (tmp_path / "gpu" / "causal.csv").read_bytes(), (tmp_path / "cpu" / "causal.csv").read_bytes()
    assert a == b and a.count(b"\n") == 1 + 20 + 190
    import json

    with open(tmp_path / "gpu" / "causal.json") as fp:
        assert json.load(fp)["fused"] is True
