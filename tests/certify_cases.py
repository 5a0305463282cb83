"""Shared inputs of the pair-certificate tests (tests/test_certify_cpu.py, tests/test_certify_gpu.py):
a case builder (random net, integer node boxes, PA table, symbolic row bounds) and a numpy float64
oracle of the certificate written with plain loops, independently of ops/reference.py.

Feature i of every case ranges over 0..TOY[i % 5] (the toy domain of tests/test_bab_gpu.py for
n0 = 5).  A node holds the whole range of its PA dims; its x' box is its x box widened by tau on the
RA dims.  Pairs are the ordered pairs of different PA assignments."""
import functools
import itertools
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops.backend import Backend

TOY = (3, 4, 2, 4, 5)
UNIT = 2.0 ** -24


class Case(NamedTuple):
    n0: int
    hidden: Tuple[int, ...]
    pa: Tuple[int, ...]
    ra: Tuple[int, ...]
    tau: int
    Nn: int
    seed: int
    bias: float = 0.0
    npairs: Optional[int] = None      # keep the first npairs pairs (an odd count: idle lanes)
    wmax: int = 3                     # box widths 0..wmax per dim

    @property
    def relaxed(self) -> bool:
        return bool(self.ra)


def frange(i: int) -> int:
    return TOY[i % 5]


def rows(lo, hi, values, pa):
    """Node boxes [N, n] -> node-major rows [N*V, n] with the PA dims set to assignment v
    (BaBSolver._rows)."""
    N, n = lo.shape
    V = values.shape[0]
    rlo = lo[:, None, :].expand(N, V, n).clone()
    rhi = hi[:, None, :].expand(N, V, n).clone()
    vv = values.to(lo.dtype)[None, :, :].expand(N, V, values.shape[1])
    rlo[:, :, pa] = vv
    rhi[:, :, pa] = vv
    return rlo.reshape(N * V, n), rhi.reshape(N * V, n)


def inputs(c: Case):
    """Net, boxes and PA table of a case (CPU tensors, no bounds yet)."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    rng = torch.tensor([float(frange(i)) for i in range(c.n0)])
    lo = torch.stack([torch.randint(0, frange(i) + 1, (c.Nn,), generator=g) for i in range(c.n0)], 1).float()
    hi = torch.minimum(lo + torch.randint(0, c.wmax + 1, (c.Nn, c.n0), generator=g).float(), rng[None])
    pa = torch.tensor(list(c.pa), dtype=torch.long)
    lo[:, pa] = 0
    hi[:, pa] = rng[pa]
    plo, phi = lo.clone(), hi.clone()
    for r in c.ra:
        plo[:, r] -= c.tau
        phi[:, r] += c.tau
    vals = np.array(list(itertools.product(*[range(frange(p) + 1) for p in c.pa])), np.int64)
    prs = np.array([(i, j) for i in range(len(vals)) for j in range(len(vals)) if i != j], np.int64)
    if c.npairs is not None:
        prs = prs[:c.npairs]
    shared = torch.ones(c.n0, dtype=torch.bool)
    shared[list(c.ra)] = False
    m = random_mlp(c.n0, list(c.hidden), seed=300 + c.seed, bias_scale=c.bias)
    return SimpleNamespace(case=c, m=m, lo=lo, hi=hi, plo=plo, phi=phi, values=torch.from_numpy(vals),
                           pairs=torch.from_numpy(prs), pa=pa, shared=shared, relaxed=c.relaxed)


def build(c: Case, device="cpu"):
    """:func:`inputs` moved to ``device`` with the symbolic bounds of the Nn * V rows."""
    s = inputs(c)
    s.be = Backend(s.m, device)
    for k in ("lo", "hi", "plo", "phi", "values", "pairs", "pa", "shared"):
        setattr(s, k, getattr(s, k).to(device))
    s.res_x = s.be.bounds(*rows(s.lo, s.hi, s.values, s.pa), mode="symbolic")
    s.res_xp = s.be.bounds(*rows(s.plo, s.phi, s.values, s.pa), mode="symbolic") if c.relaxed else s.res_x
    return s


def certify_args(s):
    """Positional arguments of Backend.pair_certify / hip.pair_certify after the backend."""
    return (s.res_x, s.res_xp, s.lo, s.hi, s.plo, s.phi, s.pairs, s.values, s.pa, s.shared, s.relaxed)


# The shape matrix of the kernel tests.  Kernel instance = (fused | eval + pick) x (NM 16 | 32); every
# instance runs with Nn = 1 and with an Nn that leaves its last workgroup partial.  Q = pairs x
# orientations: 1..4 fused (lane groups of 1, 2, 4, 4), above that the two-kernel path.
MATRIX = {
    # fused, NM = 16
    "f16_q1_n1": Case(5, (6, 4), (2,), (), 0, 1, 40, 0.0, npairs=1),
    "f16_q2_n63": Case(13, (8, 6), (12,), (0,), 2, 63, 60, 0.5, npairs=1),        # PA at n0 - 1
    "f16_q3_n65": Case(16, (8, 6), (7,), (), 0, 65, 91, 0.0, npairs=3),
    "f16_q4_n257": Case(5, (6, 4), (2,), (3,), 1, 257, 3, 0.5, npairs=2),
    # fused, NM = 32
    "f32_q3_n1": Case(17, (8, 6), (2,), (), 0, 1, 4, 0.0, npairs=3),
    "f32_q4_n65": Case(32, (8, 6), (31,), (5,), 1, 65, 111, 0.0, npairs=2),        # PA at the masks' top bit
    "f32_q1_n64": Case(20, (8, 6), (2,), (), 0, 64, 6, 0.5, npairs=1),
    # eval + pick, NM = 16
    "t16_q132_n65": Case(5, (6, 4), (2, 0), (), 0, 65, 7, 0.0),                    # two PAs, 12 assignments
    "t16_q5_n1": Case(16, (8, 6), (4,), (), 0, 1, 8, 0.5, npairs=5),
    # eval + pick, NM = 32
    "t32_q20_n257": Case(17, (8, 6), (4,), (), 0, 257, 9, 0.5, npairs=20),
    "t32_q6_n1": Case(32, (8, 6), (31, 2), (0,), 1, 1, 41, 0.0, npairs=3),
    "t32_q12_n63": Case(20, (8, 6), (2,), (1,), 2, 63, 11, 0.0),
}


# The NaN-rule tests: a zero-bias net with nodes that the certificate closes although the sign bounds
# of the rows of their first pair exclude nothing (most closed nodes are closed by the sign bounds alone)
NAN_CASE = Case(5, (6, 4), (2,), (), 0, 64, 35, 0.0, npairs=2)


def nan_target(s, open_) -> int:
    """A closed node of ``s`` whose pair 0 is evaluated (not excluded by the sign bounds)."""
    return int(np.nonzero(~np.asarray(open_, bool) & ~oracle(s).imp[:, 0])[0][0])


def with_nan(s, n: int):
    """``s`` with NaN in one coefficient of the lower form of node n's row of pair 0's first assignment."""
    import copy
    import dataclasses

    t = copy.copy(s)
    t.res_x = dataclasses.replace(s.res_x, Lc=s.res_x.Lc.clone())
    t.res_x.Lc[n * s.values.shape[0] + int(s.pairs[0, 0]), 1] = float("nan")
    t.res_xp = t.res_x if s.res_xp is s.res_x else s.res_xp
    return t


# Upper side of the score checks: score <= max_q min_t (g64(t) + K marg(t)).  K_REF is the largest k the
# fp32 CPU reference needs over MATRIX (tests/test_certify_cpu.py measures and bounds it: the margin
# itself, k = 1, plus the rounding it covers); the kernels get twice that.
K_REF = 1.0265
K = 2 * K_REF


def exact_case(npairs: Optional[int], Nn: int = 65, seed: int = 20, device="cpu"):
    """Hand-made forms whose objective fp32 evaluates without rounding: two PAs (dims 2 and 0, the
    terms 3 v2 - 2 v0 cancel for some assignments), small integer coefficients whose A and B parts
    have the same sign on every dim (no breakpoint inside (0, 1): t is 0 or 1), integer constants,
    errors of 1/4.  The certificate value is then the exact objective plus the margin, up to the
    rounding of the two additions of the margin terms."""
    from fairify_amd.ops import reference as ref

    s = inputs(Case(5, (6, 4), (2, 0), (), 0, Nn, seed, 0.0, npairs=npairs))
    g = torch.Generator().manual_seed(seed)
    R = Nn * s.values.shape[0]
    sign = torch.tensor([1., -1., 1., -1., 1.])

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    Lc, Uc = -sign * ints(0, 7, R, 5), sign * ints(0, 7, R, 5)
    for C in (Lc, Uc):
        C[:, 2], C[:, 0] = 3.0, -2.0
    quarter = torch.full((R,), 0.25)
    res = ref.BoundResult(out_lb=-torch.ones(R), out_ub=torch.ones(R), Lc=Lc, L0=ints(-8, 8, R), Le=quarter,
                          Uc=Uc, U0=ints(-8, 8, R), Ue=quarter.clone())
    for k in ("lo", "hi", "plo", "phi", "values", "pairs", "pa", "shared"):
        setattr(s, k, getattr(s, k).to(device))
    for k in ("out_lb", "out_ub", "Lc", "L0", "Le", "Uc", "U0", "Ue"):
        setattr(res, k, getattr(res, k).to(device))
    s.be = Backend(s.m, device)
    s.res_x = s.res_xp = res
    return s


def exact_bounds(s):
    """(expected score, tolerance) [Nn] of :func:`exact_case`: the oracle value with the margin once,
    and 2 unit |value| (the two additions) + 8 unit max margin (the margin's own arithmetic)."""
    o_ = oracle(s)
    f = node_values(o_, 1.0)
    return f, 2 * UNIT * np.abs(f) + 8 * UNIT * np.nanmax(o_.marg, axis=(1, 2))


# ------------------------------------------------------------------------------------------- oracle
def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def g64(Ac, A0, Bc, B0, sh, xl, xh, pl, ph, t):
    """The margin-free objective max_{x, x'} t A(x) + (1 - t) B(x') at every t of the array ``t``:
    shared dims carry the combined coefficient on x, the others x and x' separately."""
    t = np.asarray(t, np.float64)[:, None]
    cs = t * Ac + (1 - t) * Bc
    vs = np.maximum(cs * xl, cs * xh)
    ca, cb = t * Ac, (1 - t) * Bc
    vu = np.maximum(ca * xl, ca * xh) + np.maximum(cb * pl, cb * ph)
    return np.where(sh, vs, vu).sum(1) + t[:, 0] * A0 + (1 - t[:, 0]) * B0


def oracle(s, unit: float = UNIT):
    """fp64 certificate of every (node, pair, orientation) from the fp32 forms and boxes of ``s``.

    Arrays indexed [n, qq] with qq = orientation * Pp + pair (the kernels' order): ``imp`` (excluded
    by the rows' sign bounds), the signed folded forms ``Ac, A0, Bc, B0`` (PA coefficients zeroed),
    ``magA, magB``, and padded to T = n0 + 2 candidates with NaN: ``ts`` (0, 1 and the exact
    breakpoints of the shared dims inside (0, 1)), ``g`` = g64(ts) and ``marg`` =
    gamma(2 n0 + 4) (t magA + (1 - t) magB) + 8 unit (magA + magB)."""
    fx = {k: _f64(getattr(s.res_x, a)) for k, a in (("Lc", "Lc"), ("L0", "L0"), ("Le", "Le"), ("Uc", "Uc"),
                                                     ("U0", "U0"), ("Ue", "Ue"), ("olb", "out_lb"), ("oub", "out_ub"))}
    fp = {k: _f64(getattr(s.res_xp, a)) for k, a in (("Lc", "Lc"), ("L0", "L0"), ("Le", "Le"), ("Uc", "Uc"),
                                                      ("U0", "U0"), ("Ue", "Ue"), ("olb", "out_lb"), ("oub", "out_ub"))}
    xlo, xhi, xplo, xphi = (_f64(t) for t in (s.lo, s.hi, s.plo, s.phi))
    pairs, values = s.pairs.cpu().numpy(), s.values.cpu().numpy().astype(np.float64)
    pa = [int(i) for i in s.pa.cpu().numpy()]
    sh = s.shared.cpu().numpy().astype(bool)
    Nn, n0 = xlo.shape
    V, Pp = values.shape[0], pairs.shape[0]
    norient = 2 if s.relaxed else 1
    Q, T = Pp * norient, n0 + 2
    ku = (2 * n0 + 4 + 2) * unit
    gam = ku / (1 - ku)
    o_ = SimpleNamespace(Nn=Nn, n0=n0, Pp=Pp, Q=Q, sh=sh, pa=pa, unit=unit,
                         imp=np.zeros((Nn, Q), bool), Ac=np.zeros((Nn, Q, n0)), Bc=np.zeros((Nn, Q, n0)),
                         A0=np.zeros((Nn, Q)), B0=np.zeros((Nn, Q)), magA=np.zeros((Nn, Q)), magB=np.zeros((Nn, Q)),
                         ts=np.full((Nn, Q, T), np.nan), g=np.full((Nn, Q, T), np.nan),
                         marg=np.full((Nn, Q, T), np.nan), xlo=xlo, xhi=xhi, xplo=xplo, xphi=xphi)

    def fold(C, c0, v):
        C = C.copy()
        terms = C[pa] * values[v]
        C[pa] = 0.0
        return C, c0 + terms.sum(), np.abs(terms).sum()

    for n in range(Nn):
        xl, xh, pl, ph = xlo[n], xhi[n], xplo[n], xphi[n]
        mx, mxp = np.maximum(np.abs(xl), np.abs(xh)), np.maximum(np.abs(pl), np.abs(ph))
        for qq in range(Q):
            o, q = divmod(qq, Pp)
            vi, vj = int(pairs[q, 0]), int(pairs[q, 1])
            ri, rj = n * V + vi, n * V + vj
            if o == 0:      # t (-(L_v(x) - eL)) + (1 - t) (U_v'(x') + eU)
                imp = fx["olb"][ri] >= 0 or fp["oub"][rj] <= 0
                Ac, A0, fA = fold(fx["Lc"][ri], fx["L0"][ri] - fx["Le"][ri], vi)
                Ac, A0 = -Ac, -A0
                Bc, B0, fB = fold(fp["Uc"][rj], fp["U0"][rj] + fp["Ue"][rj], vj)
            else:           # t (U_v(x) + eU) + (1 - t) (-(L_v'(x') - eL))
                imp = fx["oub"][ri] <= 0 or fp["olb"][rj] >= 0
                Ac, A0, fA = fold(fx["Uc"][ri], fx["U0"][ri] + fx["Ue"][ri], vi)
                Bc, B0, fB = fold(fp["Lc"][rj], fp["L0"][rj] - fp["Le"][rj], vj)
                Bc, B0 = -Bc, -B0
            magA = (np.abs(Ac) * mx).sum() + abs(A0) + fA
            magB = (np.abs(Bc) * mxp).sum() + abs(B0) + fB
            ts = [0.0, 1.0]
            for i in range(n0):
                if sh[i] and i not in pa and Ac[i] != Bc[i]:
                    t = -Bc[i] / (Ac[i] - Bc[i])
                    if 0.0 < t < 1.0:
                        ts.append(t)
            ts = np.array(ts)
            k = len(ts)
            o_.imp[n, qq] = imp
            o_.Ac[n, qq], o_.A0[n, qq], o_.Bc[n, qq], o_.B0[n, qq] = Ac, A0, Bc, B0
            o_.magA[n, qq], o_.magB[n, qq] = magA, magB
            o_.ts[n, qq, :k] = ts
            o_.g[n, qq, :k] = g64(Ac, A0, Bc, B0, sh, xl, xh, pl, ph, ts)
            o_.marg[n, qq, :k] = gam * (ts * magA + (1 - ts) * magB) + 8 * unit * (magA + magB)
    return o_


def pair_values(o_, k: float = 0.0):
    """min_t (g64(t) + k marg(t)) per (node, pair, orientation), -1 where ``imp``: [Nn, Q].  NaN forms
    give NaN."""
    v = np.where(np.isnan(o_.ts), np.inf, o_.g + k * o_.marg)
    return np.where(o_.imp, -1.0, v.min(-1))


def node_values(o_, k: float = 0.0):
    """max over (pair, orientation) of :func:`pair_values`: [Nn] (-inf without pairs)."""
    pv = pair_values(o_, k)
    return pv.max(1) if pv.shape[1] else np.full(pv.shape[0], -np.inf)


def smallest_k(o_, score, hi: float = 64.0, iters: int = 50):
    """Per node the smallest k with node_values(k) >= score (bisection; node_values grows with k)."""
    score = np.asarray(score, np.float64)
    lo_k, hi_k = np.zeros(o_.Nn), np.full(o_.Nn, hi)
    assert np.all(node_values(o_, hi) >= score), "score above the oracle at k = %g" % hi
    for _ in range(iters):
        mid = 0.5 * (lo_k + hi_k)
        ok = _node_values_vec(o_, mid) >= score
        hi_k = np.where(ok, mid, hi_k)
        lo_k = np.where(ok, lo_k, mid)
    return hi_k


def _node_values_vec(o_, k):
    """node_values with one k per node."""
    v = np.where(np.isnan(o_.ts), np.inf, o_.g + k[:, None, None] * o_.marg)
    return np.where(o_.imp, -1.0, v.min(-1)).max(1)


# ------------------------------------------------------------------------------------- enumeration
def forward64(m, x):
    """The logit of integer points x [R, n0] in float64."""
    h = np.asarray(x, np.float64)
    L = len(m.weights)
    for l, (w, b) in enumerate(zip(m.weights, m.biases)):
        h = h @ w.astype(np.float64) + b.astype(np.float64)
        if l < L - 1:
            h = np.maximum(h, 0.0)
    return h[:, 0]


def violating_nodes(s) -> np.ndarray:
    """bool [Nn]: the node holds a lattice pair (x, x') with x in the x box, shared dims equal,
    |x_r - x'_r| <= tau on the RA dims, PA assignments a pair of ``s.pairs``, and logits of
    opposite strict signs in float64."""
    c = s.case
    lo, hi = s.lo.cpu().numpy().astype(np.int64), s.hi.cpu().numpy().astype(np.int64)
    values, pairs = s.values.cpu().numpy(), s.pairs.cpu().numpy()
    pa, free = list(c.pa), [d for d in range(c.n0) if d not in c.pa]
    offs = list(itertools.product(range(-c.tau, c.tau + 1), repeat=len(c.ra))) if c.ra else [()]
    out = np.zeros(c.Nn, bool)
    for n in range(c.Nn):
        pts = np.array(list(itertools.product(*[range(lo[n, d], hi[n, d] + 1) for d in free])), np.int64)
        X = np.zeros((len(pts), len(values), c.n0), np.int64)
        X[:, :, free] = pts[:, None, :]
        X[:, :, pa] = values[None, :, :]
        zx = forward64(s.m, X.reshape(-1, c.n0)).reshape(len(pts), len(values))
        for e in offs:
            Xp = X.copy()
            for d, off in zip(c.ra, e):
                Xp[:, :, d] += off
            zp = forward64(s.m, Xp.reshape(-1, c.n0)).reshape(len(pts), len(values)) if c.ra else zx
            if np.any(zx[:, pairs[:, 0]] * zp[:, pairs[:, 1]] < 0):
                out[n] = True
                break
    return out


# the three query shapes of the soundness tests on the toy domain (n0 = 5): one PA, two PAs
# (12 assignments, 132 ordered pairs), one PA with an RA dim and tau = 1; per shape four nets
SOUND_SHAPES = {"one_pa": dict(pa=(2,), ra=(), tau=0), "two_pa": dict(pa=(2, 0), ra=(), tau=0),
                "pa_ra": dict(pa=(2,), ra=(3,), tau=1)}
SOUND_NETS = ((0, 0.0), (1, 0.5), (2, 0.0), (3, 0.5))


def sound_cases(shape: str, Nn: int = 64):
    kw = SOUND_SHAPES[shape]
    return [Case(5, (6, 4), kw["pa"], kw["ra"], kw["tau"], Nn, seed, bias) for seed, bias in SOUND_NETS]


@functools.lru_cache(maxsize=None)
def sound_truth(shape: str, Nn: int = 64):
    """Per net of :func:`sound_cases`: the violating-node mask (cached per process)."""
    return [violating_nodes(inputs(c)) for c in sound_cases(shape, Nn)]
