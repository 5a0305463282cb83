"""Counting branch-and-bound, GPU tier: the enumeration kernel (csrc/count.hip) against the
reference and exact arithmetic for every tile count, the level kernel against box_codes_ref /
split_ref on the same bounds, count_partitions end to end against the brute force, and
`measure --certify` on a zoo shape against the CPU."""
import csv

import numpy as np
import pytest
import torch

import count_cases as cc
import rate_cases as rc
from fairify_amd.engine.search import pa_table
from fairify_amd.engine.count import _enumerate
from fairify_amd.engine.rate import exact_flags
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import count as OC
from fairify_amd.ops import rate as R
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu
EMPTY = 0x7FFFFFFF

# TM = 1, 2, 2 (three layers), 1 (zero bias), 7, 4, 10
ENUM_NETS = ("8x6", "20x6", "17x9x4", "5x5", "70x6", "50x6", "150x6")


def _net(name, k):
    if name in rc.FAMILIES:
        return rc.family_net(name, k)
    return random_mlp(5, [int(name.split("x")[0]), 6], seed=100 + k, bias_scale=0.5)


def _tables(q, lo, hi, dev):
    values, pairs = pa_table(q, lo.numpy().astype(np.int64), hi.numpy().astype(np.int64))
    return torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)


def _enum(be, q, lo, hi, dev, **kw):
    from fairify_amd.ops import hip

    values, pairs = _tables(q, lo, hi, dev)
    c, a, idx = hip.count_enum(be, q, lo.to(dev), hi.to(dev), values, pairs, **kw)
    return c.cpu().numpy(), a.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("name", ENUM_NETS)
def test_enum_kernel_against_exact_arithmetic(cuda, name, kind):
    q = cc.query(kind)
    lo, hi, pids = cc.boxes(kind)                      # the 24 boxes are the leaves, at most 256 points each
    free = OC.free_dims(q)
    vol = cc.weights(q, lo, hi)
    assert vol.max() <= 256
    for k in (0, 5):
        m = _net(name, k)
        be = Backend(m, cuda)
        assert be.hip
        cert, amb, idx = _enum(be, q, lo, hi, cuda)
        brute = cc.brute_unfair(m, q, lo, hi)
        print(f"{name}/{k} {kind}: kernel certain {int(cert.sum())}, ambiguous {int(amb.sum())}, exact {int(brute.sum())}")
        assert (cert >= 0).all() and (cert <= brute).all() and (brute <= cert + amb).all()
        assert (cert + amb <= vol).all()                            # lanes past the volume count nothing
        cpu = Backend(m, "cpu")
        values, pairs = _tables(q, lo, hi, "cpu")
        for p in range(lo.shape[0]):
            if 0 < amb[p] <= R.AMB_SLOTS:
                row = idx[p, :amb[p]]
                assert (idx[p, amb[p]:] == EMPTY).all() and len(set(row.tolist())) == amb[p]
                assert ((row >= 0) & (row < vol[p])).all()
                X = OC.lattice_points_at(lo[p:p + 1], hi[p:p + 1], free, torch.from_numpy(row.astype(np.int64))[None])[0]
                _, poss = R.rate_flags_ref(cpu, q, X, values, pairs)
                ex = exact_flags(m, q, X.numpy().astype(np.int64), values.numpy(), pairs.numpy())
                assert (poss.numpy() | ex).all()
            else:
                assert (idx[p] == EMPTY).all()
        # resolved on the host: the exact counts, which are the CPU tier's integers
        unfair, v = _enumerate(be, q, lo.to(cuda), hi.to(cuda), *_tables(q, lo, hi, cuda), 256)
        assert np.array_equal(unfair, brute) and np.array_equal(v, vol)
        cpu_unfair, _ = _enumerate(cpu, q, lo, hi, values, pairs, 256)
        assert np.array_equal(unfair, cpu_unfair)


def test_enum_workgroups_and_neighbours_do_not_matter(cuda):
    q = cc.query("pa")
    lo, hi, pids = cc.boxes()
    be = Backend(rc.family_net("5x5", 5), cuda)
    base = _enum(be, q, lo, hi, cuda)
    assert base[1].sum() > 0                                        # ambiguous points are in play
    for blocks in (1, 2, 24):
        got = _enum(be, q, lo, hi, cuda, blocks=blocks)
        assert all(np.array_equal(x, y) for x, y in zip(got, base)), blocks
    for k in (0, 7, 23):
        got = _enum(be, q, lo[k:k + 1], hi[k:k + 1], cuda)
        assert all(np.array_equal(x[0], y[k]) for x, y in zip(got, base)), k
    got = _enum(be, q, lo, hi, cuda, max_vol=65536)
    assert all(np.array_equal(x, y) for x, y in zip(got, base))


def test_enum_ambiguous_box_index_and_overflow(cuda):
    q = cc.query("pa")
    lo, hi, pids = cc.ambiguous_box()
    m = rc.ambiguous_net()
    be = Backend(m, cuda)
    # whole: 144 ambiguous points overflow the 32 slots
    cert, amb, idx = _enum(be, q, lo, hi, cuda)
    assert cert.tolist() == [0] and amb.tolist() == [144] and (idx == EMPTY).all()
    unfair, vol = _enumerate(be, q, lo.to(cuda), hi.to(cuda), *_tables(q, lo, hi, cuda), 256)
    assert unfair.tolist() == [144] and vol.tolist() == [144]
    # in 8-point leaves: every index recorded
    lv = cc.walk(Backend(m, "cpu"), q, lo, hi, leaf_points=8)
    code, v = torch.cat([l["code"] for l in lv]), torch.cat([l["vol"] for l in lv])
    leaf = (code == OC.OPEN) & (v <= 8)
    llo, lhi = torch.cat([l["lo"] for l in lv])[leaf], torch.cat([l["hi"] for l in lv])[leaf]
    assert llo.shape[0] == 32
    cert, amb, idx = _enum(be, q, llo, lhi, cuda)
    lvol = v[leaf].numpy()
    assert not cert.any() and np.array_equal(amb, lvol) and lvol.sum() == 144
    for p in range(32):
        assert idx[p, :amb[p]].tolist() == list(range(amb[p])) and (idx[p, amb[p]:] == EMPTY).all()
    unfair, _ = _enumerate(be, q, llo.to(cuda), lhi.to(cuda), *_tables(q, lo, hi, cuda), 8)
    assert np.array_equal(unfair, lvol)


def _rows_sorted(lo, hi, part):
    """Boxes as a sorted list of tuples (partition first): a multiset per partition."""
    t = torch.cat([part.reshape(-1, 1).float().cpu(), lo.cpu(), hi.cpu()], dim=1)
    return sorted(map(tuple, t.tolist()))


@pytest.mark.parametrize("kind", ["pa", "three_valued", "relaxed"])
@pytest.mark.parametrize("leaf_points", [1, 8])
def test_level_kernel_against_reference(cuda, kind, leaf_points):
    from fairify_amd.ops import hip

    q = cc.query(kind)
    lo, hi, pids = cc.boxes(kind)
    m = rc.family_net("5x5", 5)
    # a pool from a CPU run's second and third levels, and its fifth (the first with UNFAIR nodes)
    lv = cc.walk(Backend(m, "cpu"), q, lo, hi, leaf_points=1, max_levels=5)
    assert len(lv) == 5
    lv = [lv[1], lv[2], lv[4]]
    nlo, nhi = torch.cat([l["lo"] for l in lv]).to(cuda), torch.cat([l["hi"] for l in lv]).to(cuda)
    part = torch.cat([l["part"] for l in lv]).to(cuda, torch.int32)
    N = nlo.shape[0]
    assert 200 <= N <= 400
    be = Backend(m, cuda)
    values, pairs = _tables(q, lo, hi, cuda)
    V = values.shape[0]
    assert V == (3 if kind == "three_valued" else 2)
    # the row kernel against the reference rows
    got_rows = hip.count_rows(be, q, nlo, nhi, values.float())
    want_rows = OC.node_rows(q, nlo, nhi, values)
    assert all(torch.equal(g, w) for g, w in zip(got_rows, want_rows))
    rlo, rhi, clo, chi = got_rows
    rx = be.bounds(rlo, rhi, mode="symbolic", crown=True)
    rp = be.bounds(clo, chi, mode="symbolic", crown=True) if q.relaxed else rx
    lx, ux, lxp, uxp = (t.view(N, V) for t in (rx.out_lb, rx.out_ub, rp.out_lb, rp.out_ub))
    score = OC.split_scores(m)
    free = OC.free_dims(q)
    fair = torch.zeros(24, dtype=torch.int64, device=cuda)
    unfair = torch.zeros(24, dtype=torch.int64, device=cuda)
    child_cnt = torch.zeros(24, dtype=torch.int32, device=cuda)
    code, kids, leaves, counters = hip.count_level(be, q, nlo, nhi, part, lx, ux, lxp, uxp, pairs, score, leaf_points,
                                                   fair, unfair, child_cnt)
    nk, nl, lost = counters.cpu().tolist()
    # the reference on the same bounds
    want = OC.box_codes_ref(lx.cpu(), ux.cpu(), lxp.cpu(), uxp.cpu(), pairs.cpu())
    assert torch.equal(code.cpu(), want)
    assert len(set(want.tolist())) == 3                             # all three classes occur
    vol = OC.volumes(nlo.cpu(), nhi.cpu(), free)
    pl = part.cpu().long()
    wf = torch.zeros(24, dtype=torch.int64).index_add_(0, pl[want == OC.FAIR], vol[want == OC.FAIR])
    wu = torch.zeros(24, dtype=torch.int64).index_add_(0, pl[want == OC.UNFAIR], vol[want == OC.UNFAIR])
    assert torch.equal(fair.cpu(), wf) and torch.equal(unfair.cpu(), wu)
    leaf = (want == OC.OPEN) & (vol <= leaf_points)
    inner = (want == OC.OPEN) & ~leaf
    assert lost == 0 and nl == int(leaf.sum()) and nk == 2 * int(inner.sum()) and nk > 0
    _, wlo, whi = OC.split_ref(nlo.cpu()[inner], nhi.cpu()[inner], free, score)
    assert _rows_sorted(kids[0][:nk], kids[1][:nk], kids[2][:nk]) == \
        _rows_sorted(wlo, whi, pl[inner].repeat_interleave(2))
    assert _rows_sorted(leaves[0][:nl], leaves[1][:nl], leaves[2][:nl]) == \
        _rows_sorted(nlo.cpu()[leaf], nhi.cpu()[leaf], pl[leaf])
    assert torch.equal(child_cnt.cpu().long(), torch.bincount(pl[inner], minlength=24) * 2)


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("net", cc.NETS + (("70x6", 5),), ids=lambda n: f"{n[0]}-{n[1]}")
def test_end_to_end_reproduces_the_brute_force(cuda, net, kind):
    q = cc.query(kind)
    lo, hi, pids = cc.boxes(kind)
    m = rc.family_net(*net)
    want = cc.brute_unfair(m, q, lo, hi)
    be = Backend(m, cuda)
    for leaf_points in (1, 8):
        r = cc.count(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), leaf_points=leaf_points)
        assert (r.open == 0).all() and np.array_equal(r.unfair, want)
        assert np.array_equal(r.fair + r.unfair, cc.weights(q, lo, hi))
        # exact on both devices: the CPU tier's integers
        c = cc.count(Backend(m, "cpu"), q, lo, hi, pids, leaf_points=leaf_points)
        assert np.array_equal(r.unfair, c.unfair) and np.array_equal(r.fair, c.fair)


@pytest.mark.parametrize("kind", cc.EXTRA_KINDS)
def test_end_to_end_wider_query_kinds(cuda, kind):
    q = cc.query(kind)
    lo, hi, pids = cc.boxes(kind)
    for net in cc.EXTRA_NETS:
        m = rc.family_net(*net)
        want = cc.brute(*net, kind)
        r = cc.count(Backend(m, cuda), q, lo.to(cuda), hi.to(cuda), pids.to(cuda), leaf_points=8)
        assert (r.open == 0).all() and np.array_equal(r.unfair, want)


def test_end_to_end_budget_batch_and_slices(cuda):
    q = cc.query("pa")
    lo, hi, pids = cc.boxes()
    w = cc.weights(q, lo, hi)
    dlo, dhi, dpid = lo.to(cuda), hi.to(cuda), pids.to(cuda)
    for net in (("5x5", 5), ("20x6", 5)):
        be = Backend(rc.family_net(*net), cuda)
        want = cc.brute(*net, "pa")
        prev = None
        for budget in (7, 40):
            r = cc.count(be, q, dlo, dhi, dpid, node_budget=budget, leaf_points=8)
            assert np.array_equal(r.fair + r.unfair + r.open, w)
            assert (r.unfair <= want).all() and (want <= r.unfair + r.open).all()
            assert (r.nodes <= budget).all()
            assert prev is None or (r.open <= prev).all()
            prev = r.open
            base = cc.four(r)
            for k in (0, 5, 23):
                alone = cc.four(cc.count(be, q, dlo[k:k + 1], dhi[k:k + 1], dpid[k:k + 1], node_budget=budget,
                                         leaf_points=8))
                assert np.array_equal(alone[0], base[k]), (net, budget, k)
            for slice_nodes in (1, 5, 10 ** 6):
                got = cc.four(cc.count(be, q, dlo, dhi, dpid, node_budget=budget, leaf_points=8,
                                       slice_nodes=slice_nodes))
                assert np.array_equal(got, base), (net, budget, slice_nodes)


def test_ambiguous_box_end_to_end(cuda, monkeypatch):
    from fairify_amd.engine import count as EC

    q = cc.query("pa")
    lo, hi, pids = cc.ambiguous_box()
    be = Backend(rc.ambiguous_net(), cuda)
    for chunk in (EC._EXACT_CHUNK, 40):                  # 40: the host passes run in several groups
        monkeypatch.setattr(EC, "_EXACT_CHUNK", chunk)
        for leaf_points in (8, 64):
            r = cc.count(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), leaf_points=leaf_points)
            assert (int(r.unfair[0]), int(r.fair[0]), int(r.open[0])) == (144, 0, 0)
            assert r.stats["overflowed_leaves"] == (4 if leaf_points == 64 else 0)
            assert r.stats["host_points"] == 144 and r.stats["leaf_points"] == 144


def test_measure_certify_zoo_shape(cuda, tmp_path):
    from fairify_amd.analysis.rate import BOUNDS_HEADER, measure_preset

    kw = dict(n_samples=64, max_partitions=16, certify=True, node_budget=256)
    gpu = measure_preset("src/GC-age", "GC-1", device="cuda:0", out_dir=str(tmp_path / "gpu"), **kw)
    cpu = measure_preset("src/GC-age", "GC-1", device="cpu", out_dir=str(tmp_path / "cpu"), **kw)
    assert gpu.keys() == cpu.keys() and {"certified_lower", "certified_exact", "count_nodes"} <= gpu.keys()
    tabs = []
    for d in ("gpu", "cpu"):
        with open(tmp_path / d / "bounds.csv", newline="") as f:
            rows = list(csv.DictReader(f))
        assert list(rows[0]) == BOUNDS_HEADER and len(rows) == 16
        for r in rows:
            w, fa, un, op, nodes = (int(r[k]) for k in ("weight", "fair", "unfair", "open", "nodes"))
            assert fa + un + op == w and nodes <= 256
            assert 0.0 <= float(r["lower"]) <= float(r["upper"]) <= 1.0
        tabs.append(rows)
    for g, c in zip(*tabs):
        assert (g["grid_id"], g["weight"]) == (c["grid_id"], c["weight"])
        if int(g["open"]) == 0 and int(c["open"]) == 0:               # the two trees may differ otherwise
            assert (g["fair"], g["unfair"]) == (c["fair"], c["unfair"])
    for out in (gpu, cpu):
        assert 0.0 <= out["certified_lower"] <= out["certified_upper"] <= 1.0


def test_uncovered_shapes_raise(cuda):
    from fairify_amd.ops import hip

    lo, hi, pids = cc.boxes()
    q = cc.query("pa")
    values, pairs = _tables(q, lo, hi, cuda)
    args = (lo.to(cuda), hi.to(cuda), values, pairs)
    be = Backend(rc.family_net("8x6", 0), cuda)
    with pytest.raises(ValueError, match="launch-shape limit"):
        hip.count_enum(be, rc.query(("f2",), ("f0", "f1"), 3), *args)
    with pytest.raises(ValueError, match="workgroups"):
        hip.count_enum(be, q, *args, blocks=25)
    with pytest.raises(ValueError, match="leaf volume"):
        hip.count_enum(be, q, *args, max_vol=65537)
    big = torch.full((1, 5), 40.0, device=cuda)                      # 41^4 points
    with pytest.raises(ValueError, match="leaf volume"):
        hip.count_enum(be, q, torch.zeros(1, 5, device=cuda), big, values, pairs)
    with pytest.raises(ValueError, match="1..32"):
        hip.count_enum(be, q, *args[:2], torch.zeros(33, 1, dtype=torch.int64, device=cuda), pairs)
    wide = Backend(random_mlp(5, [161], seed=0), cuda)
    with pytest.raises(ValueError, match="160"):
        hip.count_enum(wide, q, *args)
    with pytest.raises(ValueError, match="leaf_points"):
        cc.count(be, q, *args[:2], pids.to(cuda), leaf_points=65537)
