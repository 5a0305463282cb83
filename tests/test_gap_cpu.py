"""Certified score gap, CPU tier: gap_partitions against a brute force written with plain loops
(tests/gap_cases.py) -- containment, witness, width of closed partitions, budget, independence --,
the node bound along a descent, and the `gap` command."""
import csv
import functools
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import count_cases as cc
import gap_cases as gc
import rate_cases as rc
from fairify_amd.analysis import gap as AG
from fairify_amd.analysis import rate as AR
from fairify_amd.analysis.hybrid import V_UNKNOWN, V_UNSAT
from fairify_amd.engine import exact
from fairify_amd.engine.gap import gap_partitions
from fairify_amd.engine.search import pa_table
from fairify_amd.ops import count as OC
from fairify_amd.ops import gap as OG
from fairify_amd.ops.backend import Backend

NO_BUDGET = 10 ** 6


@functools.lru_cache(maxsize=None)
def _be(name, k):
    return Backend(gc.family_net(name, k), "cpu")


@functools.lru_cache(maxsize=None)
def _run(name, k, kind, tol, leaf_points):
    lo, hi, pids = gc.boxes(kind)
    return gap_partitions(_be(name, k), gc.query(kind), lo, hi, pids, tol, NO_BUDGET, leaf_points)


@functools.lru_cache(maxsize=None)
def _widths(name, k, kind):
    lo, hi, _ = gc.boxes(kind)
    q = gc.query(kind)
    return [gc.point_width(_be(name, k), q, lo[p], hi[p]) for p in range(lo.shape[0])]


@pytest.mark.parametrize("kind", gc.KINDS)
@pytest.mark.parametrize("name,k", cc.NETS)
def test_containment_witness_and_width(name, k, kind):
    q = gc.query(kind)
    lo, hi, _ = gc.boxes(kind)
    lo_np, hi_np = lo.numpy().astype(np.int64), hi.numpy().astype(np.int64)
    want, _ = gc.brute(name, k, kind)
    m = gc.family_net(name, k)
    w = _widths(name, k, kind)
    for tol in (0.0, 0.01):
        for leaf_points in (1, 8, 64):
            r = _run(name, k, kind, tol, leaf_points)
            assert r.closed.all()
            for p in range(25):
                tag = (name, k, kind, tol, leaf_points, p)
                assert gc.brackets(r.gap_lo[p], want[p], r.gap_hi[p]), tag
                assert exact.check_pair_constraints(r.x[p:p + 1], r.xp[p:p + 1], lo_np[p:p + 1], hi_np[p:p + 1],
                                                    q.pa_idx, q.ra_idx, q.tau)[0], tag
                got = abs(exact.exact_logit_fraction(m, r.x[p]) - exact.exact_logit_fraction(m, r.xp[p]))
                assert got >= Fraction(float(r.gap_lo[p])), tag
                assert r.gap_hi[p] - r.gap_lo[p] <= tol + 2 * w[p], (tag, r.gap_hi[p] - r.gap_lo[p], w[p])


@pytest.mark.parametrize("budget", (1, 3, 16))
@pytest.mark.parametrize("name,k,kind", (("8x6", 5, "pa"), ("17x9x4", 5, "relaxed")))
def test_budget(name, k, kind, budget):
    q = gc.query(kind)
    lo, hi, pids = gc.boxes(kind)
    want, _ = gc.brute(name, k, kind)
    r = gap_partitions(_be(name, k), q, lo[24:], hi[24:], pids[24:], 0.0, budget, 8)
    assert not r.closed[0] and r.nodes[0] <= budget
    assert gc.brackets(r.gap_lo[0], want[24], r.gap_hi[0])
    if budget == 1:
        assert r.gap_hi[0] < math.inf, "the frozen children carry the root's bound"


@pytest.mark.parametrize("kind", ("pa", "relaxed", "two_pa"))
def test_independence(kind):
    name, k = "20x6", 5
    q = gc.query(kind)
    lo, hi, pids = gc.boxes(kind)
    be = _be(name, k)

    def rows(r):
        return [(r.gap_lo[p], r.gap_hi[p], bool(r.closed[p]), int(r.nodes[p]), r.x[p].tolist(), r.xp[p].tolist())
                for p in range(len(r.gap_lo))]

    for budget in (NO_BUDGET, 16):
        base = rows(gap_partitions(be, q, lo, hi, pids, 0.01, budget, 8))
        rev = torch.arange(24, -1, -1)
        assert rows(gap_partitions(be, q, lo[rev], hi[rev], pids[rev], 0.01, budget, 8)) == base[::-1]
        for p in (0, 7, 24):
            assert rows(gap_partitions(be, q, lo[p:p + 1], hi[p:p + 1], pids[p:p + 1], 0.01, budget, 8)) == [base[p]]
    sel = torch.tensor([0, 1, 2, 3, 24])
    base = rows(gap_partitions(be, q, lo[sel], hi[sel], pids[sel], 0.01, NO_BUDGET, 64))
    for sn in (1, 7):
        assert rows(gap_partitions(be, q, lo[sel], hi[sel], pids[sel], 0.01, NO_BUDGET, 64, slice_nodes=sn)) == base


def _descent(be, q, lo, hi, leaf_points, max_levels=5):
    """A cc.walk-style descent with the gap search's own split (no incumbent: nothing is pruned)."""
    values, pairs = pa_table(q, lo.numpy().astype(np.int64), hi.numpy().astype(np.int64))
    vt, pt = torch.from_numpy(values), torch.from_numpy(pairs)
    score = OC.split_scores(be.mlp)
    plo, phi, part = lo.float().clone(), hi.float().clone(), torch.zeros(lo.shape[0], dtype=torch.int64)
    inc = torch.full((1,), -math.inf, dtype=torch.float64)
    out = []
    for _ in range(max_levels):
        if not plo.shape[0]:
            break
        nb = OG.node_ub_ref(be, q, plo, phi, vt, pt)
        out.append((plo, phi, nb))
        _, _, kids, _ = OG.level_ref(q, plo, phi, part, nb.ub, nb.c, inc, 0.0, leaf_points, score)
        plo, phi, part = kids
    return vt, pt, out


@pytest.mark.parametrize("name,k,kind", (("8x6", 5, "pa"), ("17x9x4", 5, "relaxed"), ("20x6", 5, "three_valued")))
def test_node_bound(name, k, kind):
    q = gc.query(kind)
    m = gc.family_net(name, k)
    be = _be(name, k)
    lo, hi, _ = gc.boxes(kind)
    gc.brute(name, k, kind)                     # fills the logit cache of the net
    vt, pt, levels = _descent(be, q, lo[24:], hi[24:], 8)
    V = vt.shape[0]
    seen = 0
    for plo, phi, nb in levels:
        rx, rp = OG.node_forms(be, q, plo, phi, vt)
        lb, ub = rx.out_lb.view(-1, V).double(), rx.out_ub.view(-1, V).double()
        lbp, ubp = rp.out_lb.view(-1, V).double(), rp.out_ub.view(-1, V).double()
        for j in range(plo.shape[0]):
            want, _ = gc.brute_gap(m, q, plo[j], phi[j], gc._logits(name, k))
            assert Fraction(float(nb.ub[j])) >= want, (name, kind, j)
            # never above the interval difference (rounded up to fp32 as the bound itself is)
            iv = max(max(float(ubp[j, b] - lb[j, a]), float(ub[j, a] - lbp[j, b])) for a, b in pt.tolist())
            assert float(nb.ub[j]) <= float(OG.round_up32(torch.tensor([iv * (1 + 1e-12) + 1e-300], dtype=torch.float64))[0])
            # the candidate is a pair of the node
            x, xp = nb.cand_x[j].numpy().astype(np.int64), nb.cand_xp[j].numpy().astype(np.int64)
            assert exact.check_pair_constraints(x[None], xp[None], plo[j:j + 1].numpy().astype(np.int64),
                                                phi[j:j + 1].numpy().astype(np.int64), q.pa_idx, q.ra_idx, q.tau)[0]
            seen += 1
    assert seen >= 31


def test_nan_form_prunes_nothing():
    q = gc.query("pa")
    be = _be("8x6", 5)
    lo, hi, _ = gc.boxes("pa")
    values, pairs = pa_table(q, lo.numpy().astype(np.int64), hi.numpy().astype(np.int64))
    vt, pt = torch.from_numpy(values), torch.from_numpy(pairs)
    rx, _ = OG.node_forms(be, q, lo, hi, vt)
    rx.Lc = rx.Lc.clone()
    rx.Lc[0, 0] = math.nan                      # node 0, PA row 0: a NaN coefficient
    rx.out_lb = rx.out_lb.clone()
    rx.out_lb[0] = math.nan
    rx.out_ub = rx.out_ub.clone()
    rx.out_ub[0] = math.nan
    nb = OG.node_ub_from(q, lo, hi, vt, pt, rx, rx)
    assert nb.ub[0] == math.inf and torch.isfinite(nb.ub[1:]).all()
    inc = torch.full((25,), 1e30, dtype=torch.float64)
    code, _, _, _ = OG.level_ref(q, lo, hi, torch.arange(25), nb.ub, nb.c, inc, 0.0, 8, OC.split_scores(be.mlp))
    assert code[0] != OG.PRUNED and (code[1:] == OG.PRUNED).all()


def test_enum_reference_against_brute():
    q = gc.query("relaxed")
    name, k = "8x6", 5
    m, be = gc.family_net(name, k), _be(name, k)
    lo, hi, _ = gc.boxes("relaxed", whole=False)
    values, pairs = pa_table(q, lo.numpy().astype(np.int64), hi.numpy().astype(np.int64))
    l_lo, l_hi, a_s, a_p, a_e = OG.enum_gap_ref(be, q, lo, hi, torch.from_numpy(values), torch.from_numpy(pairs), sub=300)
    want, _ = gc.brute(name, k, "relaxed")
    x, xp = OG.witness_rows(q, lo.numpy(), hi.numpy(), values, pairs, a_s.numpy(), a_p.numpy(), a_e.numpy())
    for p in range(24):
        assert gc.brackets(l_lo[p], want[p], l_hi[p])
        got = abs(exact.exact_logit_fraction(m, x[p]) - exact.exact_logit_fraction(m, xp[p]))
        assert got >= Fraction(float(l_lo[p]))
        assert float(l_hi[p]) - float(l_lo[p]) <= 2 * gc.point_width(be, q, lo[p], hi[p])


def test_screened_oracle_is_the_plain_one():
    for name, k, kind in (("8x6", 5, "relaxed"), ("5x5", 5, "three_valued")):
        m, q = gc.family_net(name, k), gc.query(kind)
        lo, hi, _ = gc.boxes(kind)
        want, _ = gc.brute(name, k, kind)
        for p in (0, 6, 10, 23, 24):
            assert gc.screened_gap(m, q, lo[p], hi[p])[0] == want[p]


def test_gpu_tier_leaves_separate_their_two_best():
    """The leaves of tests/test_gap_gpu.py: at most 1 % have the reference's two best cert values
    within the comparison tolerance (there the arguments are not compared)."""
    leaves = close = 0
    for name, k in (("8x6", 5), ("20x6", 5), ("70x6", 0), ("150x6", 0), ("17x9x4", 5), ("5x5", 5), ("in20", 0)):
        for kind in ("pa", "relaxed", "three_valued", "two_ra"):
            m, q, lo, hi = gc.leaf_case(name, k, kind)
            be = Backend(m, "cpu")
            values, pairs = pa_table(q, lo[:1].numpy().astype(np.int64), hi[:1].numpy().astype(np.int64))
            table = gc.cert_table(be, q, lo, hi, torch.from_numpy(values), torch.from_numpy(pairs))
            assert [t.numel() for t in table] == [v * pairs.shape[0] * OG.offset_vectors(q).shape[0]
                                                  for v in gc.LEAF_VOLUMES]
            for j in range(lo.shape[0]):
                leaves += 1
                close += gc.top_two_within(table[j], gc.value_tolerance(be, q, lo[j], hi[j]))
    assert leaves == 252 and close <= leaves // 100, (leaves, close)


def test_enum_reference_on_a_nan_net():
    """Every bound NaN: nothing is certified (-inf, the first key as the argument), nothing excluded."""
    m = rc.ambiguous_net()
    m.weights[1][0, 0] = np.nan
    q = gc.query("pa")
    lo, hi, _ = gc.boxes("pa", whole=False)
    values, pairs = pa_table(q, lo.numpy().astype(np.int64), hi.numpy().astype(np.int64))
    l_lo, l_hi, a_s, a_p, a_e = OG.enum_gap_ref(Backend(m, "cpu"), q, lo[:3], hi[:3], torch.from_numpy(values),
                                                torch.from_numpy(pairs))
    assert (l_lo == -math.inf).all() and (l_hi == math.inf).all()
    assert a_s.tolist() == a_p.tolist() == a_e.tolist() == [0, 0, 0]


def test_refusals():
    lo, hi, pids = gc.boxes()
    be = _be("8x6", 0)
    with pytest.raises(ValueError, match="leaf_points"):
        gap_partitions(be, gc.query("pa"), lo, hi, pids, 0.01, 64, 65537)
    with pytest.raises(ValueError, match="tol"):
        gap_partitions(be, gc.query("pa"), lo, hi, pids, -1.0, 64, 8)
    with pytest.raises(ValueError, match="launch-shape limit"):
        gap_partitions(be, rc.query(ra=("f0", "f1", "f3", "f4"), tau=1), lo, hi, pids, 0.01, 64, 8)


# ---- the command ------------------------------------------------------------------------------

def test_command_on_a_stored_preset(tmp_path):
    kw = dict(max_partitions=6, node_budget=32, leaf_points=64)
    a = AG.gap_preset("src/GC-age", "GC-1", device="cpu", out_dir=str(tmp_path / "a"), **kw)
    b = AG.gap_preset("src/GC-age", "GC-1", device="cpu", out_dir=str(tmp_path / "b"), **kw)
    assert a == b
    for f in ("gap.csv", "gap.json"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    with open(tmp_path / "a" / "gap.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == AG.GAP_HEADER and len(rows) == 6
    with open(tmp_path / "a" / "gap.json") as f:
        js = json.load(f)
    assert js["gap_lo"] == max(float(r["gap_lo"]) for r in rows)
    assert js["gap_hi"] == max(float(r["gap_hi"]) for r in rows)
    assert rows[js["argmax_index"] - 1]["gap_lo"] == repr(js["gap_lo"])
    assert js["nodes"] == sum(int(r["nodes"]) for r in rows) and all(int(r["nodes"]) <= 32 for r in rows)
    assert js["closed_partitions"] + js["frozen_partitions"] == 6
    assert js["closed_partitions"] == sum(int(r["closed"]) for r in rows)
    assert 0.0 <= js["witness"]["prob_gap"] <= js["prob_gap_upper"] <= 1.0
    assert js["prob_gap_upper"] == min(1.0, js["gap_hi"] / 4)
    assert all(0.0 <= float(r["gap_lo"]) <= float(r["gap_hi"]) for r in rows)
    # the witness columns: a pair of the partition, its exact signs, its exact gap at least gap_lo
    from fairify_amd import presets
    from fairify_amd.models.zoo import get_model

    pre = presets.get("src/GC-age")
    grid, q, m = pre.grid(seed=0), pre.resolved(), get_model("GC-1", weights="zoo", seed=0)
    for r in rows:
        x, xp = (np.array(r[c].split(), np.int64) for c in ("x", "xp"))
        blo, bhi = grid.decode(np.array([int(r["grid_id"])]))
        assert exact.check_pair_constraints(x[None], xp[None], blo, bhi, q.pa_idx, q.ra_idx, q.tau)[0]
        assert (int(r["sign_x"]), int(r["sign_xp"])) == (exact.exact_signs(m, x[None])[0], exact.exact_signs(m, xp[None])[0])
        got = abs(exact.exact_logit_fraction(m, x) - exact.exact_logit_fraction(m, xp))
        assert got >= Fraction(float(r["gap_lo"]))


def test_command_line(tmp_path, capsys):
    from fairify_amd import cli

    cli.main(["gap", "--preset", "src/GC-age", "--model", "GC-1", "--max-partitions", "2", "--node-budget", "8",
              "--device", "cpu", "--out", str(tmp_path)])
    printed = json.loads(capsys.readouterr().out)
    assert printed["partitions"] == 2 and printed["nodes"] <= 16 and (tmp_path / "gap.csv").exists()


def test_soundness_monitor():
    q = gc.query("pa")
    name, k = "8x6", 5
    m, be = gc.family_net(name, k), _be(name, k)
    lo, hi, _ = gc.boxes("pa", whole=False)
    _, args = gc.brute(name, k, "pa")
    # the brute-force arg-max pairs of toy boxes 6, 10 and 23 flip sign (fp64 is enough to see it)
    for p in (6, 10, 23):
        x, xp = args[p]
        zx = float(be.forward(torch.tensor(x[None], dtype=torch.float64).float()).double()[0])
        zxp = float(be.forward(torch.tensor(xp[None], dtype=torch.float64).float()).double()[0])
        assert zx * zxp < 0 and exact.is_violation(m, x[None], xp[None])[0], p

    class ToyGrid:
        """The 24 toy boxes as a grid: decode only."""
        def decode(self, ids):
            return lo.numpy().astype(np.int64)[ids], hi.numpy().astype(np.int64)[ids]

    class Table:
        def __init__(self, codes):
            self.table = np.asarray(codes, np.int8)

    order = np.arange(24)
    codes = np.full(24, V_UNKNOWN, np.int8)
    out = AG.gap_grid(ToyGrid(), q, be, order, Table(codes), 0.01, NO_BUDGET, 8)
    assert (out[7] * out[8] < 0)[[6, 10, 23]].all(), "the search's witnesses flip there too"
    codes[10] = V_UNSAT
    with pytest.raises(AR.SoundnessError) as ei:
        AG.gap_grid(ToyGrid(), q, be, order, Table(codes), 0.01, NO_BUDGET, 8)
    err = ei.value
    assert err.grid_id == 10 and exact.is_violation(m, err.x[None], err.xp[None])[0]
    assert (err.x == args[10][0]).all() and (err.xp == args[10][1]).all()
    # a fair net's table raises nothing
    fair = _be("8x6", 0)
    assert cc.TOTALS[("8x6", 0)] == (0, 0)
    AG.gap_grid(ToyGrid(), q, fair, order, Table(np.full(24, V_UNSAT, np.int8)), 0.01, NO_BUDGET, 8)
