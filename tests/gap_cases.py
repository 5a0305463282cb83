"""Shared inputs of the score-gap tests (tests/test_gap_cpu.py, tests/test_gap_gpu.py): the toy
domain, boxes, nets and query kinds of tests/rate_cases.py / tests/count_cases.py, the whole-domain
box, the ten-tile family, a 20-input net, and a brute-force largest gap written independently of
engine/gap.py."""
import functools
import itertools
from fractions import Fraction

import numpy as np
import torch

import count_cases as cc
import rate_cases as rc
from fairify_amd.engine import exact
from fairify_amd.models.mlp import random_mlp
from fairify_amd.spec import Domain, Feature, Query

WHOLE = (torch.zeros(1, 5), torch.tensor([[6., 7., 1., 5., 6.]]))      # 2 352 non-PA points (PA f2)
KINDS = ("pa", "relaxed", "two_pa", "three_valued")


def family_net(name: str, k: int):
    if name == "150x6":                  # the ten-tile kernel instance (1 650 weights)
        return random_mlp(5, [150, 6], seed=100 + k, bias_scale=0.5)
    return rc.family_net(name, k)


def query(kind: str):
    if kind == "two_ra":                 # two RA dims with tau = 1: nine offset vectors
        return rc.query(ra=("f1", "f4"), tau=1)
    return cc.query(kind)


def boxes(kind: str = "pa", whole: bool = True):
    """The 24 toy boxes and (``whole``) the whole-domain box as row 24."""
    lo, hi, _ = cc.boxes(kind)
    if whole:
        lo, hi = torch.cat([lo, WHOLE[0]]), torch.cat([hi, WHOLE[1]])
    return lo, hi, torch.arange(lo.shape[0])


# the 20-input net: 17 dims degenerate, dims 3, 9 (PA) and 18, 19 free; exercises the second input tile
DOM20 = Domain("toy20", tuple(Feature(f"g{i}", 0, 7) for i in range(20)))


def net20():
    return random_mlp(20, [50], seed=120, bias_scale=0.5)


def box20(w3=3, w18=3, w19=3):
    g = torch.Generator().manual_seed(3)
    lo = torch.randint(0, 8, (1, 20), generator=g).float()
    hi = lo.clone()
    for d, w in ((3, w3), (18, w18), (19, w19)):
        lo[0, d], hi[0, d] = 0, w
    lo[0, 9], hi[0, 9] = 0, 1
    return lo, hi


def offsets(q):
    if q.ra_idx and q.tau > 0:
        return list(itertools.product(range(-q.tau, q.tau + 1), repeat=len(q.ra_idx)))
    return [()]


def brute_gap(m, q, lo, hi, cache=None):
    """Exact largest gap of one box ``lo, hi`` [n]: (Fraction, x, x') by plain loops over the non-PA
    points, the PA assignments, the ordered all-differ pairs and the unclipped RA offsets.
    ``cache``: exact logits by row, shared between the boxes of one net."""
    lo_np, hi_np = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
    n = lo_np.shape[0]
    free = [d for d in range(n) if d not in q.pa_idx]
    vals = list(itertools.product(*[range(lo_np[d], hi_np[d] + 1) for d in q.pa_idx]))
    best, arg = Fraction(0), None
    cache = {} if cache is None else cache

    def logit(row):
        if row not in cache:
            cache[row] = exact.exact_logit_fraction(m, row)
        return cache[row]

    for pt in itertools.product(*[range(lo_np[d], hi_np[d] + 1) for d in free]):
        base = [0] * n
        for d, v in zip(free, pt):
            base[d] = int(v)
        for val in vals:
            x = list(base)
            for d, v in zip(q.pa_idx, val):
                x[d] = int(v)
            fx = logit(tuple(x))
            for wal in vals:
                if not all(a != b for a, b in zip(val, wal)):
                    continue
                for e in offsets(q):
                    xp = list(base)
                    for d, v in zip(q.pa_idx, wal):
                        xp[d] = int(v)
                    for d, o in zip(q.ra_idx, e):
                        xp[d] += int(o)
                    g = abs(fx - logit(tuple(xp)))
                    if arg is None or g > best:
                        best, arg = g, (np.array(x, np.int64), np.array(xp, np.int64))
    return best, arg


def pair_rows(q, lo, hi):
    """Every (x, x') the query relates inside the box ``lo, hi`` [n], in the order (point, pair,
    offset): int64 [M, n] each, with the point index, pair index and offset index of each row."""
    lo_np, hi_np = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
    n = lo_np.shape[0]
    free = [d for d in range(n) if d not in q.pa_idx]
    vals = list(itertools.product(*[range(lo_np[d], hi_np[d] + 1) for d in q.pa_idx]))
    prs = [(a, b) for a in range(len(vals)) for b in range(len(vals)) if all(u != v for u, v in zip(vals[a], vals[b]))]
    X, XP, key = [], [], []
    for s, pt in enumerate(itertools.product(*[range(lo_np[d], hi_np[d] + 1) for d in free])):
        base = lo_np.copy()
        base[free] = pt
        for p, (a, b) in enumerate(prs):
            for e, off in enumerate(offsets(q)):
                x, xp = base.copy(), base.copy()
                x[list(q.pa_idx)] = vals[a]
                xp[list(q.pa_idx)] = vals[b]
                for d, o in zip(q.ra_idx, off):
                    xp[d] += o
                X.append(x)
                XP.append(xp)
                key.append((s, p, e))
    return np.array(X, np.int64), np.array(XP, np.int64), key


def screened_gap(m, q, lo, hi):
    """Exact largest gap of one box as :func:`brute_gap`, for the wider nets: every pair is evaluated
    in fp64 with its rigorous rounding bound (``exact.logits_with_error``), and the pairs that the
    bound cannot rule out as the maximum -- a handful -- are decided with ``exact_logit_fraction``."""
    X, XP, _ = pair_rows(q, lo, hi)
    rows, inv = np.unique(np.concatenate([X, XP]), axis=0, return_inverse=True)
    z, e = exact.logits_with_error(m, rows)
    inv = inv.reshape(-1)
    ix, ixp = inv[:len(X)], inv[len(X):]
    g, err = np.abs(z[ix] - z[ixp]), (e[ix] + e[ixp]) * 1.0001 + 1e-300
    cand = np.nonzero(g + err >= (g - err).max())[0]
    best, arg = Fraction(-1), None
    cache = {}

    def logit(i):
        if i not in cache:
            cache[i] = exact.exact_logit_fraction(m, rows[i])
        return cache[i]

    for c in cand:
        v = abs(logit(ix[c]) - logit(ixp[c]))
        if v > best:
            best, arg = v, (X[c], XP[c])
    return best, arg


# leaf volumes of the enumeration-kernel tests as widths over the (up to four) varying dims
LEAF_WIDTHS4 = {1: (1, 1, 1, 1), 15: (3, 5, 1, 1), 16: (4, 4, 1, 1), 17: (17, 1, 1, 1), 63: (7, 3, 3, 1),
                64: (4, 4, 4, 1), 65: (5, 13, 1, 1), 256: (4, 4, 4, 4), 2352: (7, 8, 6, 7)}
LEAF_WIDTHS3 = {1: (1, 1, 1), 15: (3, 5, 1), 16: (4, 4, 1), 17: (17, 1, 1), 63: (7, 3, 3), 64: (4, 4, 4),
                65: (5, 13, 1), 256: (4, 8, 8), 2352: (7, 8, 42)}
LEAF_VOLUMES = tuple(LEAF_WIDTHS4)


# Where a leaf's box starts on its varying dims.  A leaf at the origin (pattern 0) whose two best cert
# values lie within twice the comparison tolerance in the CPU reference -- two points that differ in
# a dim the logit hardly feels -- is moved to the first pattern that separates them, so that the
# kernel's argument can be compared with the reference's (tests/test_gap_cpu.py checks the cap).
LEAF_STARTS = ((0, 0, 0, 0), (1, 0, 2, 1), (2, 1, 0, 3), (0, 3, 1, 2), (3, 2, 1, 0), (1, 1, 1, 1), (4, 0, 3, 1))
LEAF_MOVED = {("8x6", "pa"): {15: 1, 16: 1, 17: 1, 65: 2}, ("8x6", "relaxed"): {17: 1}, ("20x6", "pa"): {63: 1},
              ("20x6", "relaxed"): {63: 1, 2352: 2}, ("70x6", "relaxed"): {65: 2}, ("70x6", "three_valued"): {17: 1},
              ("150x6", "three_valued"): {15: 1}, ("17x9x4", "pa"): {15: 1}, ("5x5", "pa"): {65: 6},
              ("5x5", "relaxed"): {65: 4, 2352: 4}, ("5x5", "two_ra"): {65: 4}, ("in20", "pa"): {2352: 1},
              ("in20", "relaxed"): {15: 1}, ("in20", "two_ra"): {2352: 2}}


def leaf_boxes(q, base, vary, pa_hi: int, moved=None):
    """One leaf per volume of ``LEAF_VOLUMES``: the row ``base`` [n] with the dims ``vary`` that are not
    protected widened to the volume's widths, from the start pattern ``moved[volume]`` (default 0),
    and the PA dims set to ``0..pa_hi``."""
    dims = [d for d in vary if d not in q.pa_idx]
    table = LEAF_WIDTHS4 if len(dims) >= 4 else LEAF_WIDTHS3
    lo = torch.tensor([list(base)] * len(LEAF_VOLUMES), dtype=torch.float32)
    hi = lo.clone()
    for r, vol in enumerate(LEAF_VOLUMES):
        start = LEAF_STARTS[(moved or {}).get(vol, 0)]
        for d, w, s in zip(dims, table[vol], start):
            lo[r, d], hi[r, d] = s, s + w - 1
        for d in q.pa_idx:
            lo[r, d], hi[r, d] = 0, pa_hi
    return lo, hi


def leaf_case(name: str, k: int, kind: str):
    """(net, query, leaf boxes lo / hi) of one enumeration-kernel case; ``name`` "in20": the 20-input net."""
    pa_hi = 2 if kind == "three_valued" else 1
    if name == "in20":
        names = dict(pa=dict(pa=("g9",)), relaxed=dict(pa=("g9",), ra=("g18",), tau=1), three_valued=dict(pa=("g3",)),
                     two_ra=dict(pa=("g9",), ra=("g18", "g19"), tau=1))[kind]
        q = Query(**{"ra": (), "tau": 0, **names}).resolve(DOM20)
        base = box20()[0][0].tolist()
        return net20(), q, *leaf_boxes(q, base, (3, 9, 18, 19), pa_hi, LEAF_MOVED.get((name, kind)))
    q = query(kind)
    return family_net(name, k), q, *leaf_boxes(q, (1, 2, 0, 1, 3), (0, 1, 2, 3, 4), pa_hi, LEAF_MOVED.get((name, kind)))


def cert_table(be, q, lo, hi, values, pairs):
    """Per leaf the reference's ``cert`` of every (point, pair, offset), flattened in that order
    (a list of fp64 tensors on the backend's device)."""
    from fairify_amd.ops import count as OC
    from fairify_amd.ops import gap as OG
    from fairify_amd.ops.rate import profile_rows

    free = OC.free_dims(q)
    vol = OC.volumes(lo, hi, free)
    vi, vj = pairs[:, 0], pairs[:, 1]
    n, V = lo.shape[1], values.shape[0]
    out = []
    for k in range(lo.shape[0]):
        X = OC.lattice_points_at(lo[k:k + 1], hi[k:k + 1], free, torch.arange(int(vol[k]), device=lo.device)[None])[0]
        XV, XP = profile_rows(q, X, values)
        lx, ux = (t.view(-1, 1, V) for t in be.point_bounds(XV.reshape(-1, n)))
        lxp, uxp = (t.view(X.shape[0], -1, V) for t in be.point_bounds(XP.reshape(-1, n))) if q.relaxed else (lx, ux)
        cert, _ = OG.cert_poss(lx[:, :, vi], ux[:, :, vi], lxp[:, :, vj], uxp[:, :, vj])
        out.append(cert.permute(0, 2, 1).reshape(-1))
    return out


def value_tolerance(be, q, lo, hi) -> float:
    """The comparison tolerance of tests/test_symbolic_kernel_gpu.py:test_point_kernel_matches_reference
    for the same arithmetic, ``1e-4 (1 + max |z|)`` over the leaf's rows."""
    X, XP, _ = pair_rows(q, lo, hi)
    z, _ = exact.logits_with_error(be.mlp, np.unique(np.concatenate([X, XP]), axis=0))
    return 1e-4 * (1.0 + float(np.abs(z).max()))


def top_two_within(cert: torch.Tensor, tol: float) -> bool:
    """Whether the two largest distinct values of a leaf's ``cert`` table lie within ``tol``."""
    top = cert.max()
    rest = cert[cert < top]
    return bool(rest.numel()) and float(top - rest.max()) <= tol


@functools.lru_cache(maxsize=None)
def _logits(name: str, k: int) -> dict:
    return {}


@functools.lru_cache(maxsize=None)
def brute(name: str, k: int, kind: str):
    """Brute-force gaps (floats rounded to nearest; compare with :func:`brackets`) of family net
    (name, k) on the 25 boxes, and the arg-max pairs (cached per process)."""
    lo, hi, _ = boxes(kind)
    m = family_net(name, k)
    q = query(kind)
    out = [brute_gap(m, q, lo[p], hi[p], _logits(name, k)) for p in range(lo.shape[0])]
    return [g for g, _ in out], [a for _, a in out]


def brackets(lo_f: float, g: Fraction, hi_f: float) -> bool:
    return Fraction(float(lo_f)) <= g <= Fraction(float(hi_f))


def point_width(be, q, lo, hi) -> float:
    """The widest ``ub - lb`` of the backend's point bounds over every row of the box (all PA
    assignments, RA offsets included)."""
    lo_np, hi_np = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
    n = lo_np.shape[0]
    free = [d for d in range(n) if d not in q.pa_idx]
    vals = list(itertools.product(*[range(lo_np[d], hi_np[d] + 1) for d in q.pa_idx]))
    rows = set()
    for pt in itertools.product(*[range(lo_np[d], hi_np[d] + 1) for d in free]):
        base = [0] * n
        for d, v in zip(free, pt):
            base[d] = int(v)
        for val in vals:
            for e in offsets(q):
                r = list(base)
                for d, v in zip(q.pa_idx, val):
                    r[d] = int(v)
                for d, o in zip(q.ra_idx, e):
                    r[d] += int(o)
                rows.add(tuple(r))
    X = torch.tensor(sorted(rows), dtype=torch.float32, device=be.device)
    lb, ub = be.point_bounds(X)
    return float((ub.double() - lb.double()).max())
