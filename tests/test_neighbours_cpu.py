"""Single-attribute neighbourhoods, CPU tier: the neighbour table follows its definition, the resolved
bits equal an independent oracle bit for bit at every radius, counts / nearest / classes follow from
them, nothing depends on chunking, batch or order, and the command writes consistent files without
touching the audit's own."""
import csv
import json

import numpy as np
import pytest
import torch

from fairify_amd.analysis import audit as AA
from fairify_amd.analysis.rate import SoundnessError
from fairify_amd.engine import exact
from fairify_amd.engine.audit import audit_rows
from fairify_amd.engine.neighbours import audit_neighbours, exposure
from fairify_amd.ops import audit as A
from fairify_amd.ops import neighbours as NB
from fairify_amd.ops.backend import Backend

import audit_cases as AC
import neighbour_cases as NC
import rate_cases as C


def test_table_construction():
    q = C.query()
    t = NB.neighbour_table(q)
    assert (t.M, t.W) == (28, 1) and t.abs.all()
    assert t.dim.tolist() == [0] * 7 + [1] * 8 + [3] * 6 + [4] * 7
    assert t.off.tolist() == list(range(7)) + list(range(8)) + list(range(6)) + list(range(7))
    assert t.radius.tolist() == [NB.FULL, NB.FULL, 0, NB.FULL, NB.FULL]
    t = NB.neighbour_table(q, 2)
    assert t.M == 16 and not t.abs.any()
    assert t.dim.tolist() == [0] * 4 + [1] * 4 + [3] * 4 + [4] * 4 and t.off.tolist() == [-2, -1, 1, 2] * 4
    # mixed: f0 relative, f1 left out, f3 a radius that covers its range (absolute), f4 full by default
    t = NB.neighbour_table(q, {"f0": 1, "f1": 0, "f3": 5})
    assert t.dim.tolist() == [0, 0] + [3] * 6 + [4] * 7
    assert t.off.tolist() == [-1, 1] + list(range(6)) + list(range(7))
    assert t.abs.tolist() == [0, 0] + [1] * 13 and t.radius.tolist() == [1, 0, 0, 5, NB.FULL]
    assert NB.neighbour_table(q, {"*": 1, "f4": "full"}).M == 6 + 7
    assert NB.neighbour_table(C.query(("f2", "f4"))).M == 21
    assert NB.neighbour_table(NC.wide_query(10)).M == 32 and NB.neighbour_table(NC.wide_query(20)).W == 2
    assert NB.neighbour_table(NC.wide_query(4074)).M == 4096
    with pytest.raises(ValueError, match="radius"):
        NB.neighbour_table(NC.wide_query(4075))
    assert NB.neighbour_table(NC.wide_query(4075), {"f0": 3}).M == 6 + 21
    for bad in ({"f9": 1}, {"f2": 1}, {"f0": -1}, {"f0": "wide"}, [1, 2]):
        with pytest.raises(ValueError):
            NB.neighbour_table(q, bad)


@pytest.mark.parametrize("radius", [None, 1, 2])
@pytest.mark.parametrize("name", list(NC.CASES))
def test_matches_oracle(name, radius):
    m, q, X = NC.case(name)
    flag, valid, delta, own, feat = NC.oracle_case(name, radius)
    r = NC.cpu_result(name, radius)
    M = flag.shape[1]
    assert r.table.M == M and r.flag.shape == (600, (M + 31) // 32) and r.flag.dtype == np.uint32
    assert np.array_equal(r.table.dim, feat)
    got, cert, poss = NC.bits(r.flag, M), NC.bits(r.cert, M), NC.bits(r.poss, M)
    assert np.array_equal(got, flag)                                   # bit for bit
    assert not (cert & ~got).any() and not (got & ~poss).any()         # cert <= flag <= poss
    assert not (poss & ~valid).any()                                   # invalid bits are 0
    assert all(NC.padding_clear(w, M) for w in (r.flag, r.cert, r.poss))
    Z, v = NB.neighbour_rows(q, X, r.table)
    assert np.array_equal(v, valid)
    assert r.ambiguous == int((poss & ~cert).sum()) and r.ambiguous_left == 0 and not r.fused
    ex = exposure(r, X, own)
    count, nearest = NC.oracle_exposure(q, flag, delta, own, feat)
    assert np.array_equal(ex.count, count) and np.array_equal(ex.nearest, nearest)
    cls = NC.classes(own, np.ones(600, bool), count)
    for c, got_c in (("flagged", ex.flagged), ("exposed", ex.exposed), ("robust", ex.robust)):
        assert np.array_equal(got_c, cls == c)
    print(f"{name} r={radius}: M {M}, flagged/exposed/robust "
          f"{[int((cls == c).sum()) for c in ('flagged', 'exposed', 'robust')]}, flagged neighbours {int(flag.sum())}, "
          f"ambiguous {r.ambiguous}")
    if radius is None:
        _, _, _, _, M_pin, classes, neighbours = NC.CASES[name]
        assert M == M_pin and tuple(int((cls == c).sum()) for c in ("flagged", "exposed", "robust")) == classes
        assert int(flag.sum()) == neighbours and r.ambiguous == NC.CPU_AMBIGUOUS.get(name, 0)


@pytest.mark.parametrize("name", ["5x5", "relaxed"])
def test_flag_is_the_audit_of_the_materialised_neighbours(name):
    m, q, X = NC.case(name)
    r = NC.cpu_result(name)
    Z, valid = NB.neighbour_rows(q, X, r.table)
    assert Z.shape == (600, r.table.M, 5)
    flat = audit_rows(Backend(m, "cpu"), q, Z.reshape(-1, 5))
    assert np.array_equal(NC.bits(r.flag, r.table.M), (flat.flip_mask != 0).reshape(600, -1) & valid)


def test_rows_outside_the_domain():
    m, q, X = NC.case("three-values")
    X = X[:120].copy()
    X[[3, 50], 3] = [6, -1]                        # PA outside its domain: not audited, all zeros
    X[10, 0] = 40                                  # non-PA coordinates outside their range: still audited
    X[11, 1] = -3
    X[12, 4] = 9
    be = Backend(m, "cpu")
    for radii, spec in (({}, None), ({0: 2, 1: 3, 4: 2}, {"f0": 2, "f1": 3, "f4": 2})):
        flag, valid, delta, own, feat = NC.oracle(m, q, X, radii)
        r = audit_neighbours(be, q, X, radii=spec)
        M = r.table.M
        assert np.array_equal(NC.bits(r.flag, M), flag)
        for w in (r.cert, r.poss, r.flag):
            assert not w[[3, 50]].any()
        assert (r.own[[3, 50]] == -1).all() and (r.own[[10, 11, 12]] >= 0).all()
        _, v = NB.neighbour_rows(q, X, r.table)
        assert np.array_equal(v, valid)
        f0 = feat == 0
        if spec is None:
            # the overwritten feature brings row 10 back into the range: all 7 values are neighbours;
            # through another feature the row keeps its f0 = 40 and is decided there
            assert valid[10, f0].all() and valid[10, feat == 1].sum() == 7
        else:
            assert not valid[10, f0].any()         # 40 - 2 is still outside 0..6
            assert valid[11, feat == 1].tolist() == [False, False, False, False, False, True]   # -3 + 3 = 0
            assert valid[12, feat == 4].tolist() == [False, False, False, False]                # 9 - 2 = 7 > 6
        ex = exposure(r, X, own)
        count, nearest = NC.oracle_exposure(q, flag, delta, own, feat)
        assert np.array_equal(ex.count, count) and np.array_equal(ex.nearest, nearest)
        audited = r.own >= 0
        cls = NC.classes(own, audited, count)
        assert not (ex.flagged | ex.exposed | ex.robust)[[3, 50]].any()
        for c, got_c in (("flagged", ex.flagged), ("exposed", ex.exposed), ("robust", ex.robust)):
            assert np.array_equal(got_c, cls == c)


def test_nearest_tie_rule():
    m, q, X = NC.case("relaxed")
    r = NC.cpu_result("relaxed")
    flag, valid, delta, own, feat = NC.oracle_case("relaxed")
    ex = exposure(r, X, own)
    ties = 0
    for i in range(600):
        for k in (0, 1, 3, 4):
            d = delta[i, (feat == k) & flag[i]]
            if d.size and (np.abs(d) == np.abs(d).min()).sum() == 2:
                ties += 1
                assert ex.nearest[i, k] == -np.abs(d).min()
            if d.size:
                assert abs(ex.nearest[i, k]) == np.abs(d).min() and ex.nearest[i, k] in d
            else:
                assert ex.nearest[i, k] == 0 and ex.count[i, k] == 0
    assert ties > 0, "the fixture needs a tie"


@pytest.mark.parametrize("name", ["5x5", "two-pa"])
def test_chunk_order_and_batch_independence(name):
    m, q, X = NC.case(name)
    be = Backend(m, "cpu")
    full = NC.cpu_result(name)
    t = full.table
    values, pairs = A.pa_domain_table(q)
    own = A.own_index(q, X, values)
    args = (torch.from_numpy(own[:100]), torch.from_numpy(values), torch.from_numpy(pairs), t)
    for sub in (1 << 20, 7):
        cert, poss = NB.neighbour_masks_ref(be, q, torch.from_numpy(X[:100]), *args, sub=sub)
        assert np.array_equal(cert.numpy().view(np.uint32), full.cert[:100])
        assert np.array_equal(poss.numpy().view(np.uint32), full.poss[:100])
    amb = np.nonzero((full.poss & ~full.cert).any(axis=1))[0]
    for i in [0, 7, 599] + ([int(amb[0])] if amb.size else []):
        one = audit_neighbours(be, q, X[i:i + 1])
        assert np.array_equal(one.flag[0], full.flag[i])
    sub = audit_neighbours(be, q, X[100:371])
    assert np.array_equal(sub.flag, full.flag[100:371])
    perm = np.random.default_rng(0).permutation(600)
    shuf = audit_neighbours(be, q, X[perm])
    assert np.array_equal(shuf.flag, full.flag[perm]) and np.array_equal(shuf.own, full.own[perm])
    if name == "5x5":
        assert amb.size
        raw = audit_neighbours(be, q, X, resolve=False)
        assert np.array_equal(raw.flag, raw.cert) and raw.ambiguous_left == raw.ambiguous == 13


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


def test_real_data(adult_data, tmp_path):
    plain, nb = tmp_path / "plain", tmp_path / "nb"
    want = AA.audit_preset("src/AC-sex", "AC-3", max_rows=256, out_dir=str(plain))
    out = AA.audit_preset("src/AC-sex", "AC-3", max_rows=256, out_dir=str(nb), neighbours=True)
    for name in ("audit.csv", "audit.json"):
        assert _read(plain / name) == _read(nb / name)                 # byte-identical
    assert not (plain / "neighbours.csv").exists()
    s = out.pop("neighbours")
    assert out == want
    with open(nb / "neighbours.json") as fp:
        assert json.load(fp) == s
    assert s["M"] == 343 and s["audited"] == 256 and s["ambiguous_left"] == 0
    assert s["flagged"] == want["flagged"] and s["flagged"] + s["exposed"] + s["robust"] == s["audited"]
    assert set(s["radii"].values()) == {"full"} and "sex" not in s["radii"] and len(s["radii"]) == 12
    assert sum(f["flagged_neighbours"] for f in s["features"].values()) == s["flagged_neighbours"]
    assert 0 < s["flagged_neighbours"] <= s["valid_neighbours"] == 256 * (343 - 12)
    with open(nb / "neighbours.csv") as fp:
        table = list(csv.DictReader(fp))
    assert len(table) == 256
    assert sum(r["class"] == "exposed" for r in table) == s["exposed"]
    assert sum(r["class"] == "robust" for r in table) == s["robust"]
    assert sum(int(r["flagged"]) for r in table) == s["flagged"]
    assert sum(int(r["flagged_neighbours"]) for r in table) == s["flagged_neighbours"]
    for r in table[:64]:
        counts = [int(v) for k, v in r.items() if k.endswith("_count")]
        assert sum(counts) == int(r["flagged_neighbours"]) and len(counts) == 12
        assert all((int(r[k[:-6] + "_nearest"]) != 0) == (int(v) > 0) for k, v in r.items() if k.endswith("_count"))
    print(f"AC-3 on 256 Adult rows: {s['flagged']} flagged, {s['exposed']} exposed, {s['robust']} robust")


def _rows_csv(tmp_path, n, seed=3):
    from fairify_amd import presets
    from fairify_amd.data import tabular

    dom = presets.get("src/GC-age").domain()
    path = tmp_path / "rows.csv"
    tabular.synthetic(dom, n=n, seed=seed).df.to_csv(path, index=False)
    return dom, path


def test_cli_on_a_csv(tmp_path, capsys):
    from fairify_amd import cli

    dom, path = _rows_csv(tmp_path, 96)
    base = ["audit", "--preset", "src/GC-age", "--model", "GC-1", "--data", str(path), "--device", "cpu"]
    with pytest.raises(ValueError, match="radius"):                    # credit_amount is too wide for full
        cli.main(base + ["--neighbours"])
    capsys.readouterr()
    cli.main(base + ["--out", str(tmp_path / "plain")])
    capsys.readouterr()
    cli.main(base + ["--out", str(tmp_path / "nb"), "--neighbours", "--radius", "2", "--radius-of", "month=full",
                     "--radius-of", "credit_amount=3"])
    printed = json.loads(capsys.readouterr().out)
    for name in ("audit.csv", "audit.json"):
        assert _read(tmp_path / "plain" / name) == _read(tmp_path / "nb" / name)
    s = printed["neighbours"]
    with open(tmp_path / "nb" / "neighbours.json") as fp:
        assert json.load(fp) == s
    assert s["radii"]["month"] == "full" and s["radii"]["credit_amount"] == 3 and s["radii"]["purpose"] == 2
    assert "age" not in s["radii"]
    assert s["flagged"] + s["exposed"] + s["robust"] == s["audited"] == 96 and s["ambiguous_left"] == 0
    with open(tmp_path / "nb" / "neighbours.csv") as fp:
        rows = list(csv.DictReader(fp))
    assert len(rows) == 96 and [r["class"] for r in rows].count("exposed") == s["exposed"]
    assert {"month_count", "month_nearest", "credit_amount_count"} <= set(rows[0]) and "age_count" not in rows[0]


def test_doctored_verdicts_raise(tmp_path):
    """Rows that are not flagged themselves but have flagged neighbours, under a verdict table that
    calls every partition UNSAT: the contradiction comes from a neighbour."""
    from fairify_amd import presets
    from fairify_amd.models.zoo import get_model

    dom, path = _rows_csv(tmp_path, 256)
    kw = dict(data=str(path), neighbours=True, radius=2, out_dir=str(tmp_path / "a"))
    AA.audit_preset("src/GC-age", "GC-1", **kw)
    with open(tmp_path / "a" / "neighbours.csv") as fp:
        cls = [r["class"] for r in csv.DictReader(fp)]
    exposed = [i for i, c in enumerate(cls) if c == "exposed"]
    assert exposed, "the fixture needs exposed rows"
    import pandas as pd

    sub = tmp_path / "exposed.csv"
    pd.read_csv(path).iloc[exposed].to_csv(sub, index=False)
    pre = presets.get("src/GC-age")
    grid = pre.grid(seed=0)
    res = tmp_path / "results"
    res.mkdir()
    with open(res / "GC-1.csv", "w", newline="") as fp:
        wr = csv.writer(fp)
        wr.writerow(["Partition_ID", "Verification"])
        for p in range(grid.full_size):
            wr.writerow([p + 1, "unsat"])
    kw.update(data=str(sub), results=str(res), out_dir=None)
    # the rows themselves pass the cross-check
    out = AA.audit_preset("src/GC-age", "GC-1", data=str(sub), results=str(res))
    assert out["flagged"] == 0 and out["verdicts"]["unsat"]["rows"] > 0
    with pytest.raises(SoundnessError) as ei:
        AA.audit_preset("src/GC-age", "GC-1", **kw)
    err = ei.value
    m = get_model("GC-1", weights="zoo")
    assert exact.is_violation(m, err.x[None], err.xp[None])[0]
    X = pd.read_csv(sub)[dom.names].to_numpy()
    assert not (X == err.x[None]).all(axis=1).any()                    # x is a neighbour, not a row
    assert ((X != err.x[None]).sum(axis=1) == 1).any()                 # one attribute away from one
