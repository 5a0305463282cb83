"""Certified score gap, GPU tier: the leaf-enumeration kernel (csrc/gap.hip) against exact
arithmetic and against the reference for every tile count, its independence of the launch shape,
gap_partitions end to end on the fused and the composed path, and the `gap` command against the CPU."""
import csv
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import gap_cases as gc
from fairify_amd.engine import exact
from fairify_amd.engine.gap import gap_partitions
from fairify_amd.engine.search import pa_table
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import count as OC
from fairify_amd.ops import gap as OG
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

# TM = 1, 2, 7, 10, 2 (three layers), 1 (zero bias), 4 (two input tiles)
ENUM_NETS = (("8x6", 5), ("20x6", 5), ("70x6", 0), ("150x6", 0), ("17x9x4", 5), ("5x5", 5), ("in20", 0))
ENUM_KINDS = ("pa", "relaxed", "three_valued", "two_ra")
NO_BUDGET = 10 ** 6


def _tables(q, lo, hi, dev):
    values, pairs = pa_table(q, lo[:1].numpy().astype(np.int64), hi[:1].numpy().astype(np.int64))
    return values, pairs, torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)


def _enum(be, q, lo, hi, vt, pt, **kw):
    from fairify_amd.ops import hip

    out = hip.gap_enum(be, q, lo.to(be.device), hi.to(be.device), vt, pt, **kw)
    assert out is not None, "the kernel must cover this shape"
    return [t.cpu() for t in out]


@pytest.mark.parametrize("kind", ENUM_KINDS)
@pytest.mark.parametrize("name,k", ENUM_NETS)
def test_enum_kernel_against_exact_arithmetic(cuda, name, k, kind):
    m, q, lo, hi = gc.leaf_case(name, k, kind)
    be = Backend(m, cuda)
    assert be.hip
    values, pairs, vt, pt = _tables(q, lo, hi, cuda)
    l_lo, l_hi, a_s, a_p, a_e = _enum(be, q, lo, hi, vt, pt)
    x, xp = OG.witness_rows(q, lo.numpy(), hi.numpy(), values, pairs, a_s.numpy(), a_p.numpy(), a_e.numpy())
    lo_np, hi_np = lo.numpy().astype(np.int64), hi.numpy().astype(np.int64)
    for j, vol in enumerate(gc.LEAF_VOLUMES):
        want, _ = gc.screened_gap(m, q, lo[j], hi[j])
        w = gc.point_width(be, q, lo[j], hi[j])
        print(name, kind, vol, float(l_lo[j]), float(want), float(l_hi[j]), "2w", 2 * w)
        assert gc.brackets(l_lo[j], want, l_hi[j]), (name, kind, vol)
        assert exact.check_pair_constraints(x[j:j + 1], xp[j:j + 1], lo_np[j:j + 1], hi_np[j:j + 1], q.pa_idx, q.ra_idx,
                                            q.tau)[0]
        got = abs(exact.exact_logit_fraction(m, x[j]) - exact.exact_logit_fraction(m, xp[j]))
        assert got >= Fraction(float(l_lo[j])), (name, kind, vol)
        assert float(l_hi[j]) - float(l_lo[j]) <= 2 * w, (name, kind, vol)


def test_enum_kernel_matches_reference(cuda):
    """Values within the point kernel's tolerance of the reference on the same leaves, arguments
    equal except where the reference's two best cert values lie within that tolerance (at most 1 % of
    the leaves; tests/test_gap_cpu.py checks the cap on the CPU reference)."""
    leaves = excepted = 0
    for name, k in ENUM_NETS:
        for kind in ENUM_KINDS:
            m, q, lo, hi = gc.leaf_case(name, k, kind)
            be = Backend(m, cuda)
            _, _, vt, pt = _tables(q, lo, hi, cuda)
            got = _enum(be, q, lo, hi, vt, pt)
            ref = [t.cpu() for t in OG.enum_gap_ref(be, q, lo.to(cuda), hi.to(cuda), vt, pt)]
            table = gc.cert_table(be, q, lo.to(cuda), hi.to(cuda), vt, pt)
            for j in range(lo.shape[0]):
                tol = gc.value_tolerance(be, q, lo[j], hi[j])
                assert abs(float(got[0][j]) - float(ref[0][j])) <= tol, (name, kind, j)
                assert abs(float(got[1][j]) - float(ref[1][j])) <= tol, (name, kind, j)
                leaves += 1
                if gc.top_two_within(table[j], tol):
                    excepted += 1
                    continue
                assert [int(t[j]) for t in got[2:]] == [int(t[j]) for t in ref[2:]], (name, kind, j)
    print("leaves", leaves, "excepted", excepted)
    assert excepted <= leaves // 100


@pytest.mark.parametrize("name,k,kind", (("20x6", 5, "relaxed"), ("70x6", 0, "three_valued"), ("in20", 0, "pa")))
def test_enum_outputs_do_not_depend_on_the_launch(cuda, name, k, kind):
    m, q, lo, hi = gc.leaf_case(name, k, kind)
    be = Backend(m, cuda)
    _, _, vt, pt = _tables(q, lo, hi, cuda)
    L = lo.shape[0]
    base = _enum(be, q, lo, hi, vt, pt, blocks=L)

    def same(a, b):
        return all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(a, b))

    for blocks in (1, 2):
        assert same(_enum(be, q, lo, hi, vt, pt, blocks=blocks), base)
    rev = torch.arange(L - 1, -1, -1)
    assert same(_enum(be, q, lo[rev], hi[rev], vt, pt), [t[rev] for t in base])
    for j in (0, 4, L - 1):                                                # alone in its launch
        assert same(_enum(be, q, lo[j:j + 1], hi[j:j + 1], vt, pt), [t[j:j + 1] for t in base])
    over = _enum(be, q, lo, hi, vt, pt, max_vol=64)                       # leaves over the bound are flagged
    vol = np.array(gc.LEAF_VOLUMES)
    assert (over[2].numpy()[vol > 64] == -2).all() and same([t[vol <= 64] for t in over], [t[vol <= 64] for t in base])


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("name,k,kind", (("8x6", 5, "pa"), ("17x9x4", 5, "relaxed"), ("20x6", 5, "three_valued"),
                                         ("70x6", 0, "pa")))
def test_end_to_end(cuda, monkeypatch, name, k, kind, fused):
    monkeypatch.setenv("FAIRIFY_GAP_FUSED", "1" if fused else "0")
    q = gc.query(kind)
    m = gc.family_net(name, k)
    be = Backend(m, cuda)
    lo, hi, pids = gc.boxes(kind)
    sel = torch.tensor([0, 6, 10, 23, 24])
    lo, hi, pids = lo[sel], hi[sel], pids[sel]
    lo_np, hi_np = lo.numpy().astype(np.int64), hi.numpy().astype(np.int64)
    want = [gc.screened_gap(m, q, lo[p], hi[p])[0] for p in range(5)]
    w = [gc.point_width(be, q, lo[p], hi[p]) for p in range(5)]
    for tol, leaf_points in ((0.0, 8), (0.01, 64)):
        r = gap_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), tol, NO_BUDGET, leaf_points)
        assert r.closed.all() and bool(r.stats.get("fused_leaves", 0)) == fused
        for p in range(5):
            print(name, kind, fused, tol, p, r.gap_lo[p], float(want[p]), r.gap_hi[p], "w", w[p])
            assert gc.brackets(r.gap_lo[p], want[p], r.gap_hi[p])
            assert r.gap_hi[p] - r.gap_lo[p] <= tol + 2 * w[p]
            assert exact.check_pair_constraints(r.x[p:p + 1], r.xp[p:p + 1], lo_np[p:p + 1], hi_np[p:p + 1], q.pa_idx,
                                                q.ra_idx, q.tau)[0]
        if fused:      # bitwise equal across batchings
            for p in (1, 4):
                one = gap_partitions(be, q, lo[p:p + 1].to(cuda), hi[p:p + 1].to(cuda), pids[p:p + 1].to(cuda), tol,
                                     NO_BUDGET, leaf_points)
                assert (one.gap_lo[0], one.gap_hi[0], one.nodes[0]) == (r.gap_lo[p], r.gap_hi[p], r.nodes[p])
                assert (one.x[0] == r.x[p]).all() and (one.xp[0] == r.xp[p]).all()


@pytest.mark.parametrize("switch", ("1", "0"))
def test_declined_shape_takes_the_composed_path(cuda, monkeypatch, switch):
    from fairify_amd.ops import hip

    monkeypatch.setenv("FAIRIFY_GAP_FUSED", switch)
    q = gc.query("pa")
    m = random_mlp(5, [150, 150], seed=3, bias_scale=0.5)                  # stages more than 64 KB
    be = Backend(m, cuda)
    lo, hi, pids = gc.boxes("pa")
    lo, hi, pids = lo[:3], hi[:3], pids[:3]
    _, _, vt, pt = _tables(q, lo, hi, cuda)
    assert hip.gap_enum(be, q, lo.to(cuda), hi.to(cuda), vt, pt) is None
    r = gap_partitions(be, q, lo.to(cuda), hi.to(cuda), pids.to(cuda), 0.01, NO_BUDGET, 64)
    # switched on, the leaf kernel declines (LDS) while the level kernel covers the five inputs
    assert r.closed.all() and r.stats["leaves"] > 0 and "fused_leaves" not in r.stats
    assert ("fused_levels" in r.stats) == (switch == "1")
    for p in range(3):
        assert gc.brackets(r.gap_lo[p], gc.screened_gap(m, q, lo[p], hi[p])[0], r.gap_hi[p])


def test_wide_inputs_decline_both_kernels(cuda, monkeypatch):
    from fairify_amd.spec import Domain, Feature, Query

    monkeypatch.setenv("FAIRIFY_GAP_FUSED", "1")
    dom = Domain("toy40", tuple(Feature(f"h{i}", 0, 3) for i in range(40)))
    q = Query(pa=("h9",), ra=(), tau=0).resolve(dom)
    m = random_mlp(40, [8], seed=4, bias_scale=0.5)
    be = Backend(m, cuda)
    lo = torch.ones(2, 40)
    hi = lo.clone()
    for d, w in ((3, 3), (20, 2), (39, 3)):
        lo[:, d], hi[:, d] = 0, w
    lo[:, 9], hi[:, 9] = 0, 1
    hi[1, 20] = 1
    r = gap_partitions(be, q, lo.to(cuda), hi.to(cuda), torch.arange(2).to(cuda), 0.0, NO_BUDGET, 4)
    assert r.closed.all() and r.stats["leaves"] > 0 and "fused_leaves" not in r.stats and "fused_levels" not in r.stats
    for p in range(2):
        assert gc.brackets(r.gap_lo[p], gc.screened_gap(m, q, lo[p], hi[p])[0], r.gap_hi[p])


@pytest.mark.parametrize("switch", ("1", "0"))
def test_command_matches_the_cpu(cuda, tmp_path, monkeypatch, switch):
    from fairify_amd.analysis.gap import GAP_HEADER, gap_preset
    from fairify_amd import presets
    from fairify_amd.models.zoo import get_model

    monkeypatch.setenv("FAIRIFY_GAP_FUSED", switch)
    kw = dict(max_partitions=8, node_budget=64, leaf_points=256)
    gpu = gap_preset("src/GC-age", "GC-1", device="cuda:0", out_dir=str(tmp_path / "gpu"), **kw)
    cpu = gap_preset("src/GC-age", "GC-1", device="cpu", out_dir=str(tmp_path / "cpu"), **kw)
    assert gpu.keys() == cpu.keys() and not cpu["fused"] and gpu["fused"] == (switch == "1")
    tabs = []
    for d in ("gpu", "cpu"):
        with open(tmp_path / d / "gap.csv", newline="") as f:
            rows = list(csv.DictReader(f))
        assert list(rows[0]) == GAP_HEADER and len(rows) == 8
        tabs.append(rows)
    m = get_model("GC-1", weights="zoo", seed=0)
    for g, c in zip(*tabs):
        print(g, c)
        for col in GAP_HEADER:
            if col not in ("gap_lo", "gap_hi"):
                assert g[col] == c[col], col
        # the float columns bracket one value: the two brackets intersect, and each holds its own witness
        assert max(float(g["gap_lo"]), float(c["gap_lo"])) <= min(float(g["gap_hi"]), float(c["gap_hi"]))
        for r in (g, c):
            x, xp = (np.array(r[col].split(), np.int64) for col in ("x", "xp"))
            got = abs(exact.exact_logit_fraction(m, x) - exact.exact_logit_fraction(m, xp))
            assert Fraction(float(r["gap_lo"])) <= got <= Fraction(float(r["gap_hi"]))
    assert presets.get("src/GC-age").resolved().n == 20


# ---- level kernel -----------------------------------------------------------------------------

def _pool(be, q, lo, hi, want):
    """Nodes of every level of a descent without pruning from the root boxes, the first ``want``."""
    R = lo.shape[0]
    values, pairs, vt, pt = _tables(q, lo[:1], hi[:1], be.device)
    score = OC.split_scores(be.mlp).to(be.device)
    plo, phi = lo.to(be.device), hi.to(be.device)
    part = torch.arange(R, device=be.device)
    never = torch.full((R,), -math.inf, dtype=torch.float64, device=be.device)
    los, his, parts, n = [], [], [], 0
    while plo.shape[0] and n < want:
        los.append(plo), his.append(phi), parts.append(part)
        n += plo.shape[0]
        nb = OG.node_ub_ref(be, q, plo, phi, vt, pt)
        _, _, (plo, phi, part), _ = OG.level_ref(q, plo, phi, part, nb.ub, nb.c, never, 0.0, 4, score)
    return torch.cat(los)[:want], torch.cat(his)[:want], torch.cat(parts)[:want], vt, pt, score


@pytest.mark.parametrize("kind", ("pa", "relaxed", "three_valued"))
@pytest.mark.parametrize("name,k", (("8x6", 5), ("17x9x4", 5), ("in20", 0)))
def test_level_kernel_matches_reference(cuda, name, k, kind):
    from fairify_amd.ops import hip

    if name == "in20":                  # 20 inputs: the lane + 16 half of the group; roots: the nine leaf boxes
        m, q, rlo, rhi = gc.leaf_case(name, k, kind)
    else:
        m, q = gc.family_net(name, k), gc.query(kind)
        rlo, rhi, _ = gc.boxes(kind)
    R = rlo.shape[0]
    be = Backend(m, cuda)
    for N in (1, 63, 64, 65, 1000):
        lo, hi, part, vt, pt, score = _pool(be, q, rlo, rhi, N)
        assert lo.shape[0] == N
        rx, rp = OG.node_forms(be, q, lo, hi, vt)
        ref = OG.node_ub_from(q, lo, hi, vt, pt, rx, rp)
        # incumbents at midpoints between neighbouring sorted reference ubs: one ulp cannot flip a code
        u = torch.unique(ref.ub.double())
        inc = torch.empty(R, dtype=torch.float64, device=cuda)
        for p in range(R):
            i = min(int((0.2 + 0.6 * p / (R - 1)) * (u.numel() - 1)), max(u.numel() - 2, 0))
            inc[p] = (u[i] + u[i + 1]) / 2 if u.numel() > 1 else u[0] - 1.0
        leaf_points = 8
        code, dim, kids, lvs = OG.level_ref(q, lo, hi, part, ref.ub, ref.c, inc, 0.0, leaf_points, score)
        r = hip.gap_level(be, q, lo, hi, part.to(torch.int32), rx, rp, vt, pt, inc, score, leaf_points)
        assert r is not None
        ulp = (torch.nextafter(ref.ub, torch.full_like(ref.ub, math.inf)) - ref.ub).abs()
        assert bool(((r["ub"] - ref.ub).abs() <= ulp).all()), (name, kind, N)
        assert torch.equal(r["code"], code) and torch.equal(r["pair"].long(), ref.pair)
        assert torch.equal(r["orient"].long(), ref.orient)
        assert torch.equal(r["c"], ref.c) and torch.equal(r["cand_x"], ref.cand_x) and torch.equal(r["cand_xp"], ref.cand_xp)
        inner = code == OG.INNER
        assert torch.equal(r["sdim"].long()[inner], dim[inner])
        nk, nl, lost = (int(v) for v in r["counters"].cpu())
        assert (nk, nl, lost) == (kids[0].shape[0], lvs[0].shape[0], 0), "capacity overflow is reported in counters[2]"
        clo, chi, cpart, cub, ckey = (t[:nk] for t in r["kids"])
        ko = torch.argsort(ckey)
        assert torch.equal(ckey[ko], (2 * torch.nonzero(inner).flatten()).repeat_interleave(2).int()
                           + torch.tensor([0, 1], device=cuda, dtype=torch.int32).repeat(nk // 2))
        assert torch.equal(clo[ko], kids[0]) and torch.equal(chi[ko], kids[1]) and torch.equal(cpart[ko].long(), kids[2])
        assert torch.equal(cub[ko], r["ub"][inner].repeat_interleave(2))
        llo, lhi, lpart, lkey = (t[:nl] for t in r["leaves"])
        lo_ = torch.argsort(lkey)
        assert torch.equal(llo[lo_], lvs[0]) and torch.equal(lhi[lo_], lvs[1]) and torch.equal(lpart[lo_].long(), lvs[2])
        assert len(set(code.tolist())) == 3 or N < 1000, "the large pool should hold all three codes"
