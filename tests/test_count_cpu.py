"""Counting branch-and-bound, CPU tier: the reference path of engine/count.py against a brute-force
count written in tests/count_cases.py, the budget rule, independence from the batch and the slicing,
the ambiguous-point paths, the lattice decode, `measure --certify` end to end and its consistency
checks."""
import csv
import itertools
import json

import numpy as np
import pytest
import torch

import count_cases as cc
import rate_cases as rc
from fairify_amd.analysis import rate as AR
from fairify_amd.analysis.hybrid import VerdictTable
from fairify_amd.engine import exact
from fairify_amd.engine.count import count_partitions, witness_pair
from fairify_amd.ops import count as OC
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import Grid, processing_order


def _be(name, k):
    return Backend(rc.family_net(name, k), "cpu")


def test_toy_domain_and_brute_force_totals():
    lo, hi, _ = cc.boxes()
    assert int(cc.weights(cc.query("pa"), lo, hi).sum()) == cc.TOY_POINTS
    for net in cc.NETS:
        got = tuple(int(cc.brute(*net, kind).sum()) for kind in cc.KINDS)
        print(net, got)
        assert got == cc.TOTALS[net]


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("net", cc.NETS, ids=lambda n: f"{n[0]}-{n[1]}")
def test_exact_counts_match_brute_force(net, kind):
    q = cc.query(kind)
    lo, hi, pids = cc.boxes(kind)
    w = cc.weights(q, lo, hi)
    want = cc.brute(*net, kind)
    for leaf_points in (1, 8):
        r = cc.count(_be(*net), q, lo, hi, pids, leaf_points=leaf_points)
        assert (r.open == 0).all()
        assert np.array_equal(r.unfair, want)
        assert np.array_equal(r.fair + r.unfair, w)


@pytest.mark.parametrize("kind", cc.EXTRA_KINDS)
@pytest.mark.parametrize("net", cc.EXTRA_NETS, ids=lambda n: f"{n[0]}-{n[1]}")
def test_exact_counts_wider_query_kinds(net, kind):
    q = cc.query(kind)
    lo, hi, pids = cc.boxes(kind)
    want = cc.brute(*net, kind)
    assert want.sum() > 0
    for leaf_points in (1, 8):
        r = cc.count(_be(*net), q, lo, hi, pids, leaf_points=leaf_points)
        assert (r.open == 0).all() and np.array_equal(r.unfair, want)
        assert np.array_equal(r.fair + r.unfair, cc.weights(q, lo, hi))


def test_every_branch_is_exercised():
    q = cc.query("pa")
    lo, hi, pids = cc.boxes()
    be = _be("5x5", 5)
    lv = cc.walk(be, q, lo, hi, leaf_points=1)
    code, vol = torch.cat([l["code"] for l in lv]), torch.cat([l["vol"] for l in lv])
    unfair_big = int(((code == OC.UNFAIR) & (vol > 1)).sum())
    fair_big = int(((code == OC.FAIR) & (vol > 1)).sum())
    splits = int(((code == OC.OPEN) & (vol > 1)).sum())
    print("UNFAIR / FAIR nodes of volume > 1, splits:", unfair_big, fair_big, splits)
    assert unfair_big >= 1 and fair_big >= 1 and splits >= 1
    # the written-out loop and the engine bound the same nodes
    r = cc.count(be, q, lo, hi, pids, leaf_points=1)
    assert int(r.nodes.sum()) == code.numel()
    lv = cc.walk(be, q, lo, hi, leaf_points=8)
    code, vol = torch.cat([l["code"] for l in lv]), torch.cat([l["vol"] for l in lv])
    leaf = (code == OC.OPEN) & (vol <= 8)
    print("leaves, points:", int(leaf.sum()), int(vol[leaf].sum()))
    assert int(leaf.sum()) >= 1


@pytest.mark.parametrize("net", [("5x5", 5), ("20x6", 5)], ids=lambda n: f"{n[0]}-{n[1]}")
def test_budget_brackets_the_brute_force(net):
    q = cc.query("pa")
    lo, hi, pids = cc.boxes()
    w = cc.weights(q, lo, hi)
    want = cc.brute(*net, "pa")
    be = _be(*net)
    prev_open = None
    for budget in (1, 7, 40):
        r = cc.count(be, q, lo, hi, pids, node_budget=budget, leaf_points=8)
        assert np.array_equal(r.fair + r.unfair + r.open, w)
        assert (r.unfair <= want).all() and (want <= r.unfair + r.open).all()
        assert (r.nodes <= budget).all() and (r.nodes >= 1).all()
        if prev_open is not None:
            assert (r.open <= prev_open).all()
        prev_open = r.open
    assert prev_open.sum() > 0 or net != ("5x5", 5)       # 40 nodes still bind somewhere on the hard net


def test_partition_alone_and_slicing_do_not_matter():
    q = cc.query("pa")
    lo, hi, pids = cc.boxes()
    be = _be("5x5", 5)
    for budget in (7, cc.NO_BUDGET):
        base = cc.four(cc.count(be, q, lo, hi, pids, node_budget=budget, leaf_points=8))
        for k in (0, 5, 23):
            alone = cc.four(cc.count(be, q, lo[k:k + 1], hi[k:k + 1], pids[k:k + 1], node_budget=budget, leaf_points=8))
            assert np.array_equal(alone[0], base[k]), (budget, k)
        for slice_nodes in (1, 5, 10 ** 6):
            got = cc.four(cc.count(be, q, lo, hi, pids, node_budget=budget, leaf_points=8, slice_nodes=slice_nodes))
            assert np.array_equal(got, base), (budget, slice_nodes)


@pytest.mark.parametrize("leaf_points, leaves", [(8, 32), (64, 4)])
def test_ambiguous_points_index_and_overflow_paths(leaf_points, leaves):
    q = cc.query("pa")
    lo, hi, pids = cc.ambiguous_box()
    m = rc.ambiguous_net()
    be = Backend(m, "cpu")
    assert int(cc.brute_unfair(m, q, lo, hi)[0]) == 144
    r = cc.count(be, q, lo, hi, pids, leaf_points=leaf_points)
    assert (int(r.unfair[0]), int(r.fair[0]), int(r.open[0])) == (144, 0, 0)
    lv = cc.walk(be, q, lo, hi, leaf_points=leaf_points)
    code, vol = torch.cat([l["code"] for l in lv]), torch.cat([l["vol"] for l in lv])
    assert not ((code != OC.OPEN) & (vol > 1)).any()          # the box test decides nothing larger than a point
    leaf = (code == OC.OPEN) & (vol <= leaf_points)
    assert int(leaf.sum()) == leaves and int(vol[leaf].sum()) == 144
    # fp32 decides none of the points: every one reaches the host
    llo, lhi = torch.cat([l["lo"] for l in lv])[leaf], torch.cat([l["hi"] for l in lv])[leaf]
    values = torch.tensor([[0], [1]])
    pairs = torch.tensor([[0, 1], [1, 0]])
    cert, amb, masks = OC.enum_counts_ref(be, q, llo, lhi, values, pairs)
    assert int(cert.sum()) == 0 and int(amb.sum()) == 144 and all(bool(mk.all()) for mk in masks)
    assert (int(amb.max()) > 32) == (leaf_points == 64)


def test_lattice_decode_order():
    lo = torch.tensor([[1., 0., 0., 2., 3.], [0., 5., 1., 0., 0.]])
    hi = torch.tensor([[2., 2., 1., 2., 5.], [0., 6., 1., 3., 0.]])
    free = [0, 1, 3, 4]                                         # f2 is the PA
    for k in range(2):
        want = list(itertools.product(*[range(int(lo[k, d]), int(hi[k, d]) + 1) for d in free]))
        X = OC.lattice_points_at(lo[k:k + 1], hi[k:k + 1], free, torch.arange(len(want))[None])[0]
        assert X[:, free].long().tolist() == [list(p) for p in want]          # each point once, last dim fastest
        assert (X[:, 2] == lo[k, 2]).all()
    # several leaves at once, arbitrary indices
    idx = torch.tensor([[17, 0, 5], [7, 3, 3]])
    X = OC.lattice_points_at(lo, hi, free, idx)
    for k in range(2):
        want = list(itertools.product(*[range(int(lo[k, d]), int(hi[k, d]) + 1) for d in free]))
        assert X[k][:, free].long().tolist() == [list(want[int(i)]) for i in idx[k]]


def test_measure_certify_end_to_end(tmp_path):
    kw = dict(n_samples=64, max_partitions=8)
    plain = AR.measure_preset("src/GC-age", "GC-1", out_dir=str(tmp_path / "plain"), **kw)
    cert = AR.measure_preset("src/GC-age", "GC-1", out_dir=str(tmp_path / "cert"), certify=True, node_budget=64, **kw)
    new = {"certified_lower", "certified_exact", "count_nodes"}
    assert not new & plain.keys() and plain["certified_upper"] == 1.0
    assert cert.keys() == plain.keys() | new
    assert 0.0 <= cert["certified_lower"] <= cert["certified_upper"] <= 1.0
    assert (tmp_path / "plain" / "rate.csv").read_bytes() == (tmp_path / "cert" / "rate.csv").read_bytes()
    assert not (tmp_path / "plain" / "bounds.csv").exists()
    with open(tmp_path / "plain" / "rate.json") as f:
        assert json.load(f) == plain
    with open(tmp_path / "cert" / "rate.json") as f:
        assert json.load(f) == cert
    assert {k: v for k, v in cert.items() if k not in new | {"certified_upper"}} == \
        {k: v for k, v in plain.items() if k != "certified_upper"}
    with open(tmp_path / "cert" / "bounds.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == AR.BOUNDS_HEADER and len(rows) == 8
    W = U = O = N = 0
    for r in rows:
        w, fa, un, op, nodes = (int(r[k]) for k in ("weight", "fair", "unfair", "open", "nodes"))
        assert fa + un + op == w and 1 <= nodes <= 64
        assert float(r["lower"]) == un / w and float(r["upper"]) == (un + op) / w
        W, U, O, N = W + w, U + un, O + op, N + nodes
    assert cert["certified_lower"] == U / W and cert["certified_upper"] == (U + O) / W
    assert cert["certified_exact"] == (O == 0) and cert["count_nodes"] == N


def test_cli_certify_flags(tmp_path, capsys):
    from fairify_amd import cli

    out = tmp_path / "run"
    cli.main(["measure", "--preset", "src/GC-age", "--model", "GC-1", "--max-partitions", "4", "--samples", "32",
              "--device", "cpu", "--certify", "--node-budget", "16", "--leaf-points", "64", "--out", str(out)])
    printed = json.loads(capsys.readouterr().out)
    with open(out / "rate.json") as f:
        assert json.load(f) == printed
    assert printed["count_nodes"] <= 4 * 16 and printed["certified_lower"] <= printed["certified_upper"]
    with open(out / "bounds.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 4 and all(int(r["nodes"]) <= 16 for r in rows)
    assert sum(int(r["nodes"]) for r in rows) == printed["count_nodes"]


def _toy_grid():
    grid = Grid.reference(rc.DOM, 3)
    return grid, processing_order(grid, seed=0)


def test_consistency_checks():
    q = cc.query("pa")
    grid, order = _toy_grid()
    order = order[:12]
    m = rc.family_net("17x9x4", 2)
    be = Backend(m, "cpu")
    lo, hi = grid.decode(order)
    want = cc.brute_unfair(m, q, torch.from_numpy(lo).float(), torch.from_numpy(hi).float())
    wrong, clean = np.nonzero(want > 0)[0], np.nonzero(want == 0)[0]
    assert wrong.size and clean.size, "the fixture needs a box with and a box without unfair points"
    table = VerdictTable(grid)
    table.set(order, ["unknown"] * len(order))
    out, rows = AR.certify_grid(grid, q, be, order, table, leaf_points=8)
    assert [r[5] for r in rows] == want.tolist() and out["certified_exact"]
    W = sum(r[3] for r in rows)
    assert out["certified_lower"] == out["certified_upper"] == int(want.sum()) / W
    table.set(order[wrong[:1]], ["unsat"])             # marked fair although it holds unfair points
    # without the monitor the partition is trusted: fair = w, not counted
    out, rows = AR.certify_grid(grid, q, be, order, table, leaf_points=8)
    r = rows[wrong[0]]
    assert (r[4], r[5], r[6], r[7]) == (r[3], 0, 0, 0)
    with pytest.raises(AR.SoundnessError) as ei:
        AR.certify_grid(grid, q, be, order, table, leaf_points=8, check_unsat=True)
    err = ei.value
    assert err.grid_id == int(order[wrong[0]])
    blo, bhi = grid.decode(np.array([err.grid_id]))
    assert exact.is_violation(m, err.x[None], err.xp[None])[0]
    assert exact.check_pair_constraints(err.x[None], err.xp[None], blo, bhi, q.pa_idx, q.ra_idx, q.tau)[0]
    # the witness of an UNFAIR node (leaf_points = 1: no enumeration) is confirmed the same way
    with pytest.raises(AR.SoundnessError) as ei:
        AR.certify_grid(grid, q, be, order, table, leaf_points=1, check_unsat=True)
    assert exact.is_violation(m, ei.value.x[None], ei.value.xp[None])[0]
    table = VerdictTable(grid)
    table.set(order, ["unknown"] * len(order))
    table.set(order[clean[:1]], ["sat"])               # marked unfair although no profile flips
    with pytest.raises(RuntimeError, match=str(int(order[clean[0]]))):
        AR.certify_grid(grid, q, be, order, table, leaf_points=8)


def test_witness_boxes():
    q = cc.query("pa")
    lo, hi, pids = cc.boxes()
    m = rc.family_net("5x5", 5)
    want = cc.brute("5x5", 5, "pa")
    mask = np.zeros(24, bool)
    mask[::2] = True
    for leaf_points in (1, 8):
        r = cc.count(Backend(m, "cpu"), q, lo, hi, pids, leaf_points=leaf_points, witness_for=mask)
        assert sorted(r.witness) == [k for k in range(24) if mask[k] and want[k] > 0]
        for k, (blo, bhi) in r.witness.items():
            assert (blo >= lo[k].numpy()).all() and (bhi <= hi[k].numpy()).all()
            x, xp = witness_pair(m, q, blo, bhi)
            assert exact.is_violation(m, x[None], xp[None])[0]
            assert exact.check_pair_constraints(x[None], xp[None], lo[k:k + 1].numpy().astype(np.int64),
                                                hi[k:k + 1].numpy().astype(np.int64), q.pa_idx, q.ra_idx, q.tau)[0]


def test_refusals():
    lo, hi, pids = cc.boxes()
    be = _be("8x6", 0)
    with pytest.raises(ValueError, match="leaf_points"):
        count_partitions(be, cc.query("pa"), lo, hi, pids, 64, 65537)
    with pytest.raises(ValueError, match="launch-shape limit"):
        count_partitions(be, rc.query(("f2",), ("f0", "f1"), 3), lo, hi, pids, 64, 8)
    from fairify_amd.models.mlp import random_mlp
    from fairify_amd.spec import Domain, Feature, Query

    # 32 free dims of 4 values each: 2^64 non-PA points
    dom = Domain("wide", tuple(Feature(f"f{i}", 0, 3) for i in range(33)))
    q = Query(pa=("f0",), ra=(), tau=0).resolve(dom)
    with pytest.raises(ValueError, match="2\\^62"):
        count_partitions(Backend(random_mlp(33, [4], seed=0), "cpu"), q, torch.zeros(1, 33), torch.full((1, 33), 3.0),
                         torch.arange(1), 64, 8)
