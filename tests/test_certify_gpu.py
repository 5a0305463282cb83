"""The pair-certificate kernels (csrc/certify.hip) on a real MI355X against the float64 oracle of
tests/certify_cases.py: every kernel instance (fused / eval + pick, 16 / 32 register dims), lane-group
and workgroup edges, the pick outputs as properties of the kernel's own choice, the NaN rule, the
fields only the native BaB runtime sets, and soundness by lattice enumeration."""
import copy
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import certify_cases as cc
from fairify_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

OUTS = ("score", "open", "split_dim", "cand_x", "cand_xp", "cand_v", "cand_o", "scores", "leaf")


def run(s, **kw):
    """hip.pair_certify of case ``s`` -> its outputs as numpy arrays."""
    from fairify_amd.ops import hip

    dec, x = hip.pair_certify(s.be, *cc.certify_args(s), full=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dec.open_, x["open_u8"] != 0)
    r = dict(score=dec.score, open=x["open_u8"], split_dim=dec.split_dim, cand_x=dec.cand_x, cand_xp=dec.cand_xp,
             cand_v=dec.cand_v, cand_o=dec.cand_orient, scores=x["scores"], leaf=x["leaf"], gmin=x["gmin"],
             tstar=x["tstar"])
    return SimpleNamespace(**{k: v.cpu().numpy() for k, v in r.items()})


def same(a, b, rows=slice(None), keys=OUTS):
    """Bitwise equality of the outputs ``keys`` on ``rows`` (NaN compares equal to itself)."""
    return all(np.array_equal(getattr(a, k)[rows], getattr(b, k)[rows], equal_nan=True) for k in keys)


_CASES = {}


def solved(name, dev):
    """Case, oracle (from the forms the kernel reads) and kernel outputs of a MATRIX case, once per process."""
    if name not in _CASES:
        s = cc.build(cc.MATRIX[name], dev)
        assert s.be.hip
        _CASES[name] = (s, cc.oracle(s), run(s))
    return _CASES[name]


def repeated(s, k: int):
    t = copy.copy(s)
    t.pairs = s.pairs.repeat(k, 1)
    return t


# ---------------------------------------------------------------------------------------------- A
def check_scores(s, o, r):
    score = r.score.astype(np.float64)
    low, up = cc.node_values(o, 0.0), cc.node_values(o, cc.K)
    k = cc.smallest_k(o, np.minimum(score, up))
    print(f"Nn {o.Nn} Q {o.Q}: open {np.mean(r.open != 0):.2f}, largest k {k.max():.4f} (allowed {cc.K:.4f})")
    assert np.all(score >= low)                       # one-sided: never below the exact value
    assert np.array_equal(r.open != 0, r.score > 0)
    assert np.all(score <= up)
    assert np.all(r.score[o.imp.all(1)] == -1.0)
    if o.Q > 4:                                       # the two-kernel path leaves every pair's value behind
        g = r.gmin.astype(np.float64)
        assert np.all(g >= cc.pair_values(o, 0.0)) and np.all(g <= cc.pair_values(o, cc.K))
        assert np.all((r.tstar >= 0) & (r.tstar <= 1))
        assert np.array_equal(r.score, r.gmin.max(1))


@pytest.mark.parametrize("name", list(cc.MATRIX))
def test_score_against_oracle(cuda, name):
    """score >= max_q min_t g64(t) with no tolerance (the kernel value never undercuts the exact one, so
    every node the oracle leaves open is open), open == (score > 0), and score <= max_q min_t (g64 + K marg)
    with K = 2 x 1.0265 = 2.053: 1.0265 is the largest k of the fp32 CPU reference over the same cases
    (tests/test_certify_cpu.py); the kernels need 1.029 at most.  Nodes with every pair excluded by the
    sign bounds score exactly -1."""
    check_scores(*solved(name, cuda))


@pytest.mark.parametrize("npairs", [3, None])
def test_exact_forms(cuda, npairs):
    """Forms that fp32 evaluates without rounding (cc.exact_case; Q = 3 fused, Q = 132 two-kernel): the
    score is the exact objective plus the whole margin, PA magnitudes summed term by term."""
    s = cc.exact_case(npairs, device=cuda)
    want, tol = cc.exact_bounds(s)
    assert np.all(np.abs(run(s).score.astype(np.float64) - want) <= tol)


# ---------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("name", ["f16_q4_n257", "f32_q4_n65"])
def test_fused_equals_two_kernel(cuda, name):
    """The same relaxed two-pair data through the fused kernel (Q = 4) and, with the pair list three
    times over (Q = 12), through eval + pick: both keep the first maximum in orientation-major order, so
    a duplicate never wins and every output is bitwise the same."""
    s, _, a = solved(name, cuda)
    b = run(repeated(s, 3))
    assert np.any(a.score == -1.0)          # ties between the entries of a node take part
    assert np.all(b.cand_v < 2)
    assert same(a, b, keys=[k for k in OUTS if k != "cand_v"]) and np.array_equal(a.cand_v % 2, b.cand_v % 2)


# ---------------------------------------------------------------------------------------------- C
def check_picks(s, o, r, ra=(), tau=0.0, smear=False):
    """The pick outputs as properties of the kernel's own choice (cand_v, cand_o)."""
    n0, Pp, pa, sh, u = o.n0, o.Pp, o.pa, o.sh, cc.UNIT
    free = np.array([i not in pa for i in range(n0)])
    values, pairs = s.values.cpu().numpy(), s.pairs.cpu().numpy()
    low = cc.node_values(o, 0.0)
    plo_v, pup_v = cc.pair_values(o, 0.0), cc.pair_values(o, cc.K)
    wx, wxp = o.xhi - o.xlo, o.xphi - o.xplo
    for n in range(o.Nn):
        q, ori = int(r.cand_v[n]), int(r.cand_o[n])
        assert 0 <= q < Pp and 0 <= ori < o.Q // Pp
        qq = ori * Pp + q
        score = float(r.score[n])
        # the choice is a near-argmax, and the score is the chosen pair's value
        assert plo_v[n, qq] <= score <= pup_v[n, qq] and pup_v[n, qq] >= low[n]
        sc = r.scores[n].astype(np.float64)
        assert int(r.split_dim[n]) == int(np.argmax(sc[:n0] if smear else sc))
        dead_x = ~free | (wx[n] <= 0)
        live_p = free & ~sh & (wxp[n] > 0)
        assert np.all(sc[:n0][dead_x] == -1.0) and np.all(sc[n0:][~live_p] == -1.0)
        assert int(r.leaf[n]) == int(not np.any(free & (wx[n] > 0)) and not np.any(live_p))
        cx, cp = r.cand_x[n].astype(np.float64), r.cand_xp[n].astype(np.float64)
        assert np.all((cx == o.xlo[n]) | (cx == o.xhi[n]) | ~free)
        assert np.all((cp == cx) | ~(free & sh))
        un = free & ~sh
        if len(ra):
            assert np.all(np.abs(cp - cx)[list(ra)] <= tau)
            assert np.all((cp >= o.xplo[n]) & (cp <= o.xphi[n]) | ~un)
        else:
            assert np.all((cp == o.xplo[n]) | (cp == o.xphi[n]) | ~un)
        assert np.array_equal(cx[pa], values[pairs[q, 0]]) and np.array_equal(cp[pa], values[pairs[q, 1]])
        # some near-optimal t explains the split scores and makes the candidate pair a maximiser
        Ac, Bc, A0, B0 = o.Ac[n, qq], o.Bc[n, qq], o.A0[n, qq], o.B0[n, qq]
        nt = int(np.sum(~np.isnan(o.ts[n, qq])))
        near = [0] if o.imp[n, qq] else [j for j in range(nt) if o.g[n, qq, j] <= score]
        ok = False
        for j in near:
            t, g, marg = o.ts[n, qq, j], o.g[n, qq, j], o.marg[n, qq, j]
            cs, ta, tb = t * Ac + (1 - t) * Bc, t * Ac, (1 - t) * Bc
            ex = np.where(sh, np.abs(cs), np.abs(ta)) * wx[n] + 1e-9 * wx[n]
            exp_ = np.abs(tb) * wxp[n] + 1e-9 * wxp[n]
            # relative to the dim's coefficient magnitudes: the rounding of the kernel's fp32 t enters
            # through both, and at the breakpoint of dim i the two terms of its coef(t) cancel
            tol_x = 2 * n0 * u * ((np.abs(Ac) + np.where(sh, np.abs(Bc), 0.0)) * wx[n] + 1e-9 * wx[n])
            tol_p = 2 * n0 * u * (np.abs(Bc) * wxp[n] + 1e-9 * wxp[n])
            fit = np.all(np.abs(sc[n0:] - exp_)[live_p] <= tol_p[live_p])
            if not smear:
                fit = fit and np.all(np.abs(sc[:n0] - ex)[~dead_x] <= tol_x[~dead_x])
            if len(ra) == 0:
                obj = np.where(sh, cs * cx, ta * cx + tb * cp).sum() + t * A0 + (1 - t) * B0
                fit = fit and obj >= g - cc.K * marg
            if fit:
                ok = True
                break
        assert ok, f"node {n}: no near-optimal t explains scores / candidate"


@pytest.mark.parametrize("name", list(cc.MATRIX))
def test_pick_properties(cuda, name):
    """cand_v / cand_o is a near-argmax (the oracle's value of the chosen pair brackets the score and
    reaches the oracle's maximum within the tolerance of A); split_dim is the first argmax of the
    kernel's own scores row; -1 on PA, zero-width and, in the x' half, shared dims; the other entries are
    |coef(t)| x width + 1e-9 width for a near-optimal oracle t, to 2 n0 unit relative to the terms of
    coef(t); leaf exactly for single lattice points; candidates are box vertices with the pair's PA
    values that reach g64(t) within the tolerance of A."""
    check_picks(*solved(name, cuda))


@pytest.mark.parametrize("name", ["f16_q2_n63", "f32_q4_n65", "t32_q12_n63", "t32_q6_n1"])
def test_pick_with_ra_and_tau(cuda, name):
    """With the RA dims and tau passed the candidate x' stays within tau of x and inside the x' box;
    nothing else changes."""
    s, o, base = solved(name, cuda)
    c = s.case
    r = run(s, ra=c.ra, tau=float(c.tau))
    assert same(base, r, keys=[k for k in OUTS if k != "cand_xp"])
    check_picks(s, o, r, ra=c.ra, tau=c.tau)
    other = [i for i in range(c.n0) if i not in c.ra]
    assert np.array_equal(base.cand_xp[:, other], r.cand_xp[:, other])
    assert np.any(base.cand_xp != r.cand_xp) or c.Nn == 1        # the clip moved some candidate


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("Nn", [1, 65])
def test_all_leaf_batch(cuda, Nn):
    s = cc.build(cc.Case(5, (6, 4), (2,), (), 0, Nn, 12, 0.0, npairs=2, wmax=0), cuda)
    o, r = cc.oracle(s), run(s)
    check_scores(s, o, r)
    check_picks(s, o, r)
    assert np.all(r.leaf == 1) and np.all(r.scores == -1.0) and np.all(r.split_dim == 0)


@pytest.mark.parametrize("name", ["f16_q3_n65", "t32_q20_n257"])
def test_equal_coefficients_on_a_shared_dim(cuda, name):
    """res_x is res_xp and the A and B coefficients of shared dim 1 are equal (the breakpoint's
    denominator is 0): that dim has no breakpoint, the values stay finite and within the oracle's bounds."""
    s = copy.copy(solved(name, cuda)[0])
    res = dataclasses.replace(s.res_x, Lc=s.res_x.Lc.clone(), Uc=s.res_x.Uc.clone())
    res.Lc[:, 1], res.Uc[:, 1] = -0.375, 0.375
    s.res_x = s.res_xp = res
    o, r = cc.oracle(s), run(s)
    assert np.all(o.Ac[:, :, 1] == o.Bc[:, :, 1]) and np.all(np.isfinite(r.score))
    check_scores(s, o, r)
    check_picks(s, o, r)


@pytest.mark.parametrize("rep", [1, 3])
def test_nan_keeps_the_node_open(cuda, rep):
    """NaN in one pair's form: the node stays open on the fused path (Q = 2) and on the two-kernel path
    (the pair list three times over, Q = 6), and every other node of its lane group and workgroup is
    bitwise what it is without the NaN."""
    s = repeated(cc.build(cc.NAN_CASE, cuda), rep)
    base = run(s)
    n = cc.nan_target(s, base.open)
    r = run(cc.with_nan(s, n))
    assert base.open[n] == 0 and r.open[n] == 1 and r.score[n] == np.inf
    assert same(base, r, rows=np.arange(s.case.Nn) != n)


def test_no_nodes(cuda):
    s = copy.copy(solved("f16_q3_n65", cuda)[0])
    for k in ("lo", "hi", "plo", "phi"):
        setattr(s, k, getattr(s, k)[:0])
    cut = {f.name: getattr(s.res_x, f.name) for f in dataclasses.fields(s.res_x)}
    cut = {k: (v[:0] if torch.is_tensor(v) else None) for k, v in cut.items()}
    s.res_x = s.res_xp = ref.BoundResult(**cut)
    r = run(s)
    assert r.score.shape == (0,) and r.cand_x.shape == (0, 16) and r.scores.shape == (0, 32) and r.open.shape == (0,)


def test_wide_input_falls_back(cuda):
    """n0 = 33: the kernels hold at most 32 dims, the launcher refuses on the host before any launch, and
    Backend.pair_certify takes ops/reference.py on the device tensors."""
    from fairify_amd.ops import hip
    from fairify_amd.ops.backend import Backend

    s = cc.build(cc.Case(33, (8, 6), (2,), (), 0, 9, 30, 0.0))
    want = s.be.pair_certify(*cc.certify_args(s))
    for k in ("lo", "hi", "plo", "phi", "values", "pairs", "pa", "shared"):
        setattr(s, k, getattr(s, k).to(cuda))
    res = {f.name: getattr(s.res_x, f.name) for f in dataclasses.fields(s.res_x)}
    s.res_x = s.res_xp = ref.BoundResult(**{k: (v.to(cuda) if torch.is_tensor(v) else None) for k, v in res.items()})
    s.be = Backend(s.m, cuda)
    assert s.be.hip
    got = s.be.pair_certify(*cc.certify_args(s))
    direct = ref.pair_certify(*cc.certify_args(s), unit=s.be.unit)
    for f in dataclasses.fields(ref.PairDecision):
        assert torch.equal(getattr(got, f.name), getattr(direct, f.name))
    assert torch.allclose(got.score.cpu(), want.score, rtol=1e-5, atol=1e-5)
    clear = want.score.abs() > 1e-4
    assert torch.equal(got.open_.cpu()[clear], want.open_[clear])
    with pytest.raises(RuntimeError, match="-4"):
        hip.pair_certify(s.be, *cc.certify_args(s))


# ---------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("name", ["f16_q4_n257", "t32_q20_n257"])
def test_status_filter(cuda, name):
    """Nodes of partitions that are neither RUNNING (3) nor STOPPING (4) report open = 0 and score =
    -inf; all the others are bitwise the run without a status (fused and two-kernel path)."""
    s, _, base = solved(name, cuda)
    Nn = s.case.Nn
    status = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int8, device=cuda)
    part = (torch.arange(Nn, device=cuda) * 7 % 5).to(torch.int32)
    r = run(s, status=status, part=part)
    live = np.isin(status.cpu().numpy()[part.cpu().numpy()], (3, 4))
    assert live.any() and (~live).any()
    assert np.all(r.open[~live] == 0) and np.all(r.score[~live] == -np.inf)
    assert same(base, r, rows=live)


@pytest.mark.parametrize("name", ["f16_q4_n257", "t16_q132_n65", "f32_q4_n65"])
def test_skip_closed(cuda, name):
    """skip_closed over outputs pre-filled with a sentinel: a closed node writes open, score and leaf = 0
    and nothing else; an open node is bitwise the skip_closed = 0 run."""
    s, _, base = solved(name, cuda)
    r = run(s, skip_closed=True, prefill=7)
    op = base.open != 0
    assert op.any() and (~op).any()
    assert same(base, r, rows=op)
    assert np.all(r.open[~op] == 0) and np.array_equal(r.score[~op], base.score[~op]) and np.all(r.leaf[~op] == 0)
    for k in ("split_dim", "cand_x", "cand_xp", "cand_v", "cand_o", "scores"):
        assert np.all(getattr(r, k)[~op] == 7), k


def smear_inputs(s, n1, dev):
    """Layer bounds [Nn*V, n1 + 3] (three more columns than layer 0 is wide) with about half of the
    neurons unstable and exact zeros among the bounds, and first-layer weights [n0, n1]."""
    g = torch.Generator().manual_seed(n1)
    R = s.case.Nn * s.values.shape[0]
    lb = torch.randint(-2, 2, (R, n1 + 3), generator=g).float() * torch.rand(R, n1 + 3, generator=g)
    ub = lb + torch.randint(0, 3, (R, n1 + 3), generator=g).float() * torch.rand(R, n1 + 3, generator=g)
    W0 = torch.randn(s.case.n0, n1, generator=g)
    return lb.to(dev), ub.to(dev), W0.to(dev)


@pytest.mark.parametrize("n0", [13, 20])
@pytest.mark.parametrize("n1", [5, 32, 33, 100])
def test_smear_scores(cuda, n0, n1):
    """First-layer smear (non-relaxed): the x half of the scores is width_i x the sum over the node's V
    rows and the neurons j with lay_lb < 0 < lay_ub of |W0[i, j]|, + 1e-9 width_i, to 2 V n1 unit
    relative (fp32 sums of at most V n1 non-negative terms); -1 on PA and zero-width dims; split_dim
    their first argmax.  n1 below, at and past the 32-neuron mask word; rows with even and odd counts
    of unstable neurons (fetched two at a time)."""
    from fairify_amd.ops import hip

    s = cc.build(cc.Case(n0, (8, 6), (2,), (), 0, 65, 50 + n0, 0.0, npairs=2), cuda)
    o = cc.oracle(s)
    V = s.values.shape[0]
    lb, ub, W0 = smear_inputs(s, n1, cuda)
    base = run(s)
    r = run(s, smear=True, lay_lb=lb, lay_ub=ub, W0T=hip.smear_w0t(W0))
    assert same(base, r, keys=[k for k in OUTS if k not in ("scores", "split_dim")])
    assert np.array_equal(base.scores[:, n0:], r.scores[:, n0:])
    uns = ((lb < 0) & (ub > 0))[:, :n1].cpu().numpy()
    cnt = uns.sum(1)
    assert np.any(cnt % 2 == 0) and np.any(cnt % 2 == 1) and np.any(lb.cpu().numpy()[:, :n1] == 0)
    aw = np.abs(W0.cpu().numpy().astype(np.float64))                       # [n0, n1]
    acc = (uns.reshape(65, V, n1).sum(1).astype(np.float64)[:, None, :] * aw[None]).sum(2)     # [Nn, n0]
    wx = o.xhi - o.xlo
    want = acc * wx + 1e-9 * wx
    dead = (wx <= 0) | np.isin(np.arange(n0), o.pa)[None]
    want[dead] = -1.0
    got = r.scores[:, :n0].astype(np.float64)
    assert np.all(got[dead] == -1.0)
    assert np.all(np.abs(got - want)[~dead] <= 2 * V * n1 * cc.UNIT * want[~dead])
    assert np.array_equal(r.split_dim, np.argmax(r.scores[:, :n0], axis=1))
    check_picks(s, o, r, smear=True)


def test_smear_leaves_relaxed_queries_alone(cuda):
    """smear = 1 on a relaxed query (RA dims passed, nra != 0) keeps the certificate's split scores."""
    from fairify_amd.ops import hip

    s, _, _ = solved("f16_q2_n63", cuda)
    c = s.case
    lb, ub, W0 = smear_inputs(s, 33, cuda)
    a = run(s, ra=c.ra, tau=float(c.tau))
    b = run(s, ra=c.ra, tau=float(c.tau), smear=True, lay_lb=lb, lay_ub=ub, W0T=hip.smear_w0t(W0))
    assert same(a, b)


def test_wrapper_rejects_bad_runtime_fields(cuda, monkeypatch):
    """Host-side checks: nothing mis-shaped reaches a launch, and the binding still rejects unknown keys
    (before it launches anything)."""
    from fairify_amd.ops import ext, hip

    s, _, _ = solved("f16_q3_n65", cuda)
    lb, ub, W0 = smear_inputs(s, 8, cuda)
    with pytest.raises(ValueError):
        run(s, status=torch.zeros(2, dtype=torch.int8, device=cuda))
    with pytest.raises(ValueError):
        run(s, status=torch.zeros(2, dtype=torch.int8, device=cuda),
            part=torch.full((s.case.Nn,), 2, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError):
        run(s, smear=True, lay_lb=lb[:-1], lay_ub=ub, W0T=hip.smear_w0t(W0))
    with pytest.raises(ValueError):
        run(s, smear=True, lay_lb=lb, lay_ub=ub, W0T=hip.smear_w0t(W0)[:, :8])
    with pytest.raises(ValueError):
        run(s, ra=(16,), tau=1.0)
    real = ext().certify
    monkeypatch.setattr(hip, "ext", lambda: SimpleNamespace(certify=lambda **kw: real(**kw, skip_close=1)))
    with pytest.raises(TypeError, match="unexpected keyword argument 'skip_close'"):
        run(s)


# ---------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("shape", list(cc.SOUND_SHAPES))
def test_kernel_closes_no_violating_node(cuda, shape):
    """Soundness by enumeration through the kernels: no closed node holds a lattice pair of opposite
    float64 logit signs; at least 10 % of the nodes are closed and at least 10 % hold a violation."""
    closed, viol = [], []
    for c, truth in zip(cc.sound_cases(shape), cc.sound_truth(shape)):
        s = cc.build(c, cuda)
        closed.append(run(s, ra=c.ra, tau=float(c.tau)).open == 0)
        viol.append(truth)
    closed, viol = np.concatenate(closed), np.concatenate(viol)
    print(f"{shape}: closed {closed.mean():.3f} violating {viol.mean():.3f} of {closed.size} nodes")
    assert not np.any(closed & viol)
    assert closed.mean() >= 0.10 and viol.mean() >= 0.10
