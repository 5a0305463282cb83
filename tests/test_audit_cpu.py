"""Audit of real individuals, CPU tier: the resolved flip masks equal an independent brute force bit
for bit on every toy case, do not depend on batch or order, the summary and the verdict cross-check
follow their definitions, and the command runs on the Adult rows and on a CSV."""
import csv
import json

import numpy as np
import pytest
import torch

from fairify_amd.analysis import audit as AA
from fairify_amd.analysis.hybrid import VerdictTable
from fairify_amd.analysis.rate import SoundnessError
from fairify_amd.engine import exact
from fairify_amd.engine.audit import audit_rows, witness
from fairify_amd.ops import audit as A
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import Grid

import audit_cases as AC
import rate_cases as C


@pytest.mark.parametrize("name", list(AC.CASES))
def test_matches_brute_force_and_pinned_counts(name):
    _, _, _, _, V, flagged, negative, ambiguous = AC.CASES[name]
    m, q, X = AC.case(name)
    r = AC.cpu_audit(name)
    want, sx = AC.brute(name)
    values, _ = A.pa_domain_table(q)
    assert values.shape[0] == V and len(X) == (800 if name == "ambiguous" else 4800)
    assert np.array_equal(r.flip_mask, want)                          # bit for bit
    assert not (r.cert & ~want).any() and not (want & ~r.poss).any()  # cert <= flip <= poss
    has_cert = r.cert != 0
    assert np.array_equal(r.own_sign[has_cert], sx[has_cert]) and (sx[has_cert] != 0).all()
    flag = want != 0
    assert np.array_equal(r.direction, np.where(flag, sx, 0))
    assert not r.ambiguous_bits.any()
    print(f"{name}: flagged {int(flag.sum())}, direction -1 {int((sx[flag] < 0).sum())}, "
          f"ambiguous bits {AC.popcount(r.poss & ~r.cert)}")
    assert int(flag.sum()) == flagged
    assert int((r.direction[flag] < 0).sum()) == negative
    assert AC.popcount(r.poss & ~r.cert) == ambiguous
    if name == "three-values":
        assert set(np.unique(r.own).tolist()) == {0, 1, 2}            # own values 0..2, counterparts up to 5


@pytest.mark.parametrize("name", ["5x5", "two-pa", "relaxed"])
def test_batch_and_order_independence(name):
    m, q, X = AC.case(name)
    be = Backend(m, "cpu")
    full = AC.cpu_audit(name)
    amb = np.nonzero(full.poss & ~full.cert)[0]
    picks = [0, 7, len(X) - 1] + ([int(amb[0])] if amb.size else [])
    for i in picks:
        one = audit_rows(be, q, X[i:i + 1])
        assert one.flip_mask[0] == full.flip_mask[i] and one.direction[0] == full.direction[i]
    sub = audit_rows(be, q, X[100:371])
    assert np.array_equal(sub.flip_mask, full.flip_mask[100:371])
    perm = np.random.default_rng(0).permutation(len(X))
    shuf = audit_rows(be, q, X[perm])
    assert np.array_equal(shuf.flip_mask, full.flip_mask[perm])
    assert np.array_equal(shuf.direction, full.direction[perm])
    assert np.array_equal(shuf.own, full.own[perm])


def test_rows_that_are_not_audited():
    m, q, X = AC.case("three-values")
    be = Backend(m, "cpu")
    X = X[:300].copy()
    X[[3, 150], 3] = [6, -1]                       # PA outside its domain 0..5
    X[10, 0] = 40                                  # a non-PA coordinate outside the box: still audited
    r = audit_rows(be, q, X)
    assert r.own[3] == -1 and r.own[150] == -1 and r.own[10] >= 0
    for arr in (r.cert, r.poss, r.flip_mask, r.direction, r.own_sign, r.ambiguous_bits):
        assert arr[3] == 0 and arr[150] == 0
    want, _ = AC.brute_masks(m, q, X)
    assert np.array_equal(r.flip_mask, want)
    values, _ = A.pa_domain_table(q)
    s = AA.summarize(values, r)
    assert s["pa_out_of_domain"] == 2 and s["audited"] == 298 and s["rows"] == 300
    with pytest.raises(ValueError, match="encoded integers"):
        audit_rows(be, q, X.astype(np.float64) + np.eye(300, 5)[:, ::-1] * 0.5)
    with pytest.raises(ValueError, match="launch-shape limit"):
        A.pa_domain_table(C.query(("f2",), ("f0", "f1"), 3))          # 49 offset vectors


def test_resolve_false_leaves_the_ambiguous_bits():
    m, q, X = AC.case("5x5")
    r = audit_rows(Backend(m, "cpu"), q, X, resolve=False)
    full = AC.cpu_audit("5x5")
    assert np.array_equal(r.ambiguous_bits, r.poss & ~r.cert) and AC.popcount(r.ambiguous_bits) == 10
    assert np.array_equal(r.flip_mask, r.cert)
    assert not (r.cert & ~full.flip_mask).any() and not (full.flip_mask & ~r.poss).any()
    assert ((r.direction != 0) == (r.cert != 0)).all()


def test_reference_masks_definition():
    """``audit_masks_ref`` against plain loops over its own point bounds, in small chunks."""
    m, q, X = AC.case("two-pa")
    X = X[:160]
    be = Backend(m, "cpu")
    values, pairs = A.pa_domain_table(q)
    own = A.own_index(q, X, values)
    args = (torch.from_numpy(own), torch.from_numpy(values), torch.from_numpy(pairs))
    cert, poss, sign = (t.numpy() for t in A.audit_masks_ref(be, q, torch.from_numpy(X).float(), *args, sub=7))
    allowed = {(int(a), int(b)) for a, b in pairs}
    for i in range(0, 160, 9):
        l, u = (float(t[0]) for t in be.point_bounds(torch.from_numpy(X[i:i + 1]).float()))
        c = p = 0
        for w in range(values.shape[0]):
            if (int(own[i]), w) not in allowed:
                continue
            xp = X[i].copy()
            xp[list(q.pa_idx)] = values[w]
            lp, up = (float(t[0]) for t in be.point_bounds(torch.from_numpy(xp[None]).float()))
            c |= int((u < 0 < lp) or (l > 0 > up)) << w
            p |= int((l < 0 < up) or (u > 0 > lp)) << w
        assert (int(cert.view(np.uint32)[i]), int(poss.view(np.uint32)[i])) == (c, p)
        assert sign[i] == (-1 if u < 0 else 1 if l > 0 else 0)


def test_summary_arithmetic():
    name = "two-pa"
    _, q, _ = AC.case(name)
    r = AC.cpu_audit(name)
    values, _ = A.pa_domain_table(q)
    s = AA.summarize(values, r)
    V = values.shape[0]
    assert s["audited"] == 4800 and s["flagged"] == 2586 and s["rate"] == 2586 / 4800
    assert sum(g["n"] for g in s["groups"]) == s["audited"]
    assert sum(g["flagged"] for g in s["groups"]) == s["flagged"]
    assert s["flagged_negative"] == 1916 and s["flagged_negative"] + s["flagged_positive"] == s["flagged"]
    for v, g in enumerate(s["groups"]):
        sel = r.own == v
        assert g["value"] == values[v].tolist() and g["n"] == int(sel.sum())
        assert g["flagged"] == int((r.flip_mask[sel] != 0).sum())
        assert g["flagged_negative"] + g["flagged_positive"] == g["flagged"]
        for w in range(V):
            assert s["matrix"][v][w] == sum(1 for b in r.flip_mask[sel] if (int(b) >> w) & 1)
        assert all(s["matrix"][v][w] == 0 for w in range(V) if (values[v] == values[w]).any())
    assert all(isinstance(x, int) for row in s["matrix"] for x in row)
    assert sum(map(sum, s["matrix"])) == AC.popcount(r.flip_mask)


def test_verdict_cross_check():
    m, q, X = AC.case("three-values")
    r = AC.cpu_audit("three-values")
    values, _ = A.pa_domain_table(q)
    grid = Grid.reference(C.DOM, 3)                # f3 = 0..5 is split into 0..2 and 3..5
    ids = grid.encode(X)
    assert (ids >= 0).all()
    low = np.uint32(0b000111)                      # every row has f3 in 0..2: its partition's PA range
    flagged = r.flip_mask != 0
    inside = np.nonzero(flagged & ((r.flip_mask & low) != 0))[0]
    outside = np.nonzero(flagged & ((r.flip_mask & low) == 0))[0]
    assert inside.size and outside.size, "the fixture needs both kinds of flagged rows"
    # a flagged row whose flipped v' all lie outside the partition's PA range: no false alarm
    i = int(outside[0])
    table = VerdictTable(grid)
    table.set(ids[i:i + 1], ["unsat"])
    one =audit_rows(Backend(m, "cpu"), q, X[i:i + 1])
    got_ids, verdict, classes = AA.cross_check(grid, table, q, m, X[i:i + 1], one, values)
    assert got_ids[0] == ids[i] and classes["unsat"] == {"rows": 1, "flagged": 1}
    # a flagged row with a flipped v' inside the range contradicts the UNSAT verdict
    j = int(inside[0])
    table = VerdictTable(grid)
    table.set(ids[j:j + 1], ["unsat"])
    with pytest.raises(SoundnessError) as ei:
        AA.cross_check(grid, table, q, m, X, r, values)
    err = ei.value
    blo, bhi = grid.decode(np.array([err.grid_id]))
    assert table.table[err.grid_id] == 2
    assert exact.is_violation(m, err.x[None], err.xp[None])[0]
    assert exact.check_pair_constraints(err.x[None], err.xp[None], blo, bhi, q.pa_idx, q.ra_idx, q.tau)[0]
    # without verdicts every row is not_attempted; rows outside the grid get id -1
    Y = X[:50].copy()
    Y[0, 0] = 99
    ry = audit_rows(Backend(m, "cpu"), q, Y)
    got_ids, verdict, classes = AA.cross_check(grid, None, q, m, Y, ry, values)
    assert got_ids[0] == -1 and classes["not_attempted"]["rows"] == 50
    assert classes["not_attempted"]["flagged"] == int((ry.flip_mask != 0).sum())


def test_witness_is_the_first_offset():
    m, q, X = AC.case("relaxed")
    r = AC.cpu_audit("relaxed")
    values, _ = A.pa_domain_table(q)
    for i in np.nonzero(r.flip_mask)[0][:20]:
        vp = int(np.log2(int(r.flip_mask[i]) & -int(r.flip_mask[i])))
        x, xp = witness(m, q, X[i], vp)
        assert np.array_equal(x, X[i]) and exact.is_violation(m, x[None], xp[None])[0]
        assert xp[2] == values[vp][0] and abs(int(xp[1]) - int(x[1])) <= 1
        for d in range(int(x[1]) - 1, int(xp[1])):                 # no earlier offset flips
            y = xp.copy()
            y[1] = d
            assert not exact.is_violation(m, x[None], y[None])[0]
    clean = int(np.nonzero(r.poss == 0)[0][0])
    with pytest.raises(ValueError, match="no flipping counterpart"):
        witness(m, q, X[clean], 1 - int(X[clean, 2]))


def test_real_data(adult_data, tmp_path):
    from fairify_amd import presets
    from fairify_amd.data import tabular
    from fairify_amd.models.zoo import get_model
    from fairify_amd.repair.retrain import load_pairs

    pairs = tmp_path / "pairs.npz"
    out = AA.audit_preset("src/AC-sex", "AC-3", max_rows=4096, out_dir=str(tmp_path), pairs_out=str(pairs))
    assert out["source"]["synthetic"] is False and out["rows"] == 4096
    with open(tmp_path / "audit.csv") as fp:
        table = list(csv.DictReader(fp))
    assert len(table) == 4096
    with open(tmp_path / "audit.json") as fp:
        assert json.load(fp) == out
    ds = tabular.load("adult")
    X = np.concatenate([ds.X_train, ds.X_test])[:4096].astype(np.int64)
    m = get_model("AC-3", weights="zoo")
    q = presets.get("src/AC-sex").resolved()
    want, sx = AC.brute_masks(m, q, X)
    print(f"AC-3 on 4096 Adult rows: flagged {int((want != 0).sum())}")
    assert out["flagged"] == int((want != 0).sum()) and out["audited"] == 4096
    assert [int(r["flip_mask"]) for r in table] == want.tolist()
    assert [int(r["sex"]) for r in table] == X[:, 8].tolist()
    Xp, y = load_pairs(str(pairs), 13, 8)
    assert y is None and Xp.shape == (2 * out["flagged"], 13)
    x, xp = Xp[0::2].astype(np.int64), Xp[1::2].astype(np.int64)
    assert np.array_equal(x, X[want != 0]) and exact.is_violation(m, x, xp).all()
    assert (x[:, 8] != xp[:, 8]).all() and np.array_equal(np.delete(x, 8, 1), np.delete(xp, 8, 1))


def test_cli_round_trip(tmp_path, capsys):
    from fairify_amd import cli, presets
    from fairify_amd.data import tabular

    dom = presets.get("src/GC-age").domain()
    ds = tabular.synthetic(dom, n=300, seed=3)
    path = tmp_path / "rows.csv"
    df = ds.df.copy()
    df.insert(0, "note", "x")                       # columns the domain does not name are ignored
    df.to_csv(path, index=False)
    out = tmp_path / "run"
    cli.main(["audit", "--preset", "src/GC-age", "--model", "GC-1", "--data", str(path), "--max-rows", "256",
              "--device", "cpu", "--out", str(out), "--pairs-out", str(tmp_path / "p.npz")])
    printed = json.loads(capsys.readouterr().out)
    with open(out / "audit.json") as fp:
        assert json.load(fp) == printed
    assert printed["rows"] == 256 and printed["audited"] == 256 and printed["source"]["data"] == str(path)
    with open(out / "audit.csv") as fp:
        rows = list(csv.DictReader(fp))
    assert len(rows) == 256 and sum(int(r["flagged"]) for r in rows) == printed["flagged"]
    z = np.load(tmp_path / "p.npz")
    assert z["x"].shape == (printed["flagged"], dom.n) and z["xp"].shape == z["x"].shape
    bad = tmp_path / "bad.csv"
    df.drop(columns=["age"]).to_csv(bad, index=False)
    with pytest.raises(ValueError, match="lacks"):
        cli.main(["audit", "--preset", "src/GC-age", "--model", "GC-1", "--data", str(bad), "--device", "cpu"])
