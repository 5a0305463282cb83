"""Certified score gap between counterparts: the node bound, the level rule and the leaf enumeration.

For a partition box ``B``, the PA assignments ``values`` [V, npa] and ordered all-differ ``pairs``
[Pp, 2] of ``engine/search.pa_table`` and the RA offset vectors ``e`` of ``ops/rate.offset_vectors``
(unclipped, ``|e_r| <= tau``; only ``e = 0`` for a PA-only query):

    g(x, v, v', e) = | N(x[PA<-v]) - N((x + e)[PA<-v']) |      x a non-PA lattice point of B
    G(B)           = max g            (0 if there is no pair)

in units of the logit.  A branch-and-bound over the non-PA lattice (``engine/gap.py``) brackets
``gap_lo <= G(B) <= gap_hi``; a node is an integer sub-box as in ``ops/count.py``.

* node bound (:func:`node_ub_ref`): the node rows are ``ops/count.node_rows`` bounded with
  ``Backend.bounds(mode="symbolic", crown=True)``.  For a pair ``(v, v')`` orientation A is
  ``U_v'(x') + Ue' - L_v(x) + Le`` with the PA terms folded into the constant, the coefficient
  ``c_d = Uc'_d - Lc_d`` maximised over ``[lo_d, hi_d]`` on a shared dim and ``tau |Uc'_d|`` added on
  an RA dim (``x'_d = x_d + e_d``); orientation B swaps the roles (``U_v(x) - L_v'(x')``).  The sum
  runs in fp64 (the forms are fp32, the products exact) plus ``gamma(2 n0 + 8, FP64_UNIT)`` times the
  summed magnitudes of the terms.  The pair's bound is the smaller of that and the interval bound
  (``ub' - lb`` resp. ``ub - lb'``), a NaN counts as +inf; the node's ``ub`` is the largest over pairs
  and orientations (lowest pair, then A, on ties), rounded up to fp32.  The candidate is the
  maximising corner of the best pair: ``hi_d`` where ``c_d >= 0`` else ``lo_d``, ``e_d = +-tau`` by
  the sign of the counterpart's coefficient.
* level rule (:func:`level_ref`): ``ub <= inc_start + tol`` is PRUNED (a NaN or infinite ``ub`` never
  is), an open node of at most ``leaf_points`` points a LEAF, any other is halved along the free dim
  of the largest fp32 product ``|c_d| (hi_d - lo_d)`` (lowest ``d`` on ties; the ``s_d`` rule of
  ``ops/count.split_scores`` if every product is 0).
* leaf enumeration (:func:`enum_gap_ref`): per point (``ops/count.lattice_points_at``), pair and
  offset, from the rigorous point bounds: ``cert = max(lb' - ub, lb - ub')``, ``poss = max(ub' - lb,
  ub - lb')``, each subtraction in fp64 and widened outward by ``gamma(1, FP64_UNIT)`` of the
  operands' magnitudes (fp32 arithmetic would add about ``4e-7 |logit|`` to every leaf's width);
  per leaf ``leaf_lo = max cert`` with its argument (lowest point, then pair, then offset on ties)
  and ``leaf_hi = max poss``.

This module is the reference (any backend); the enumeration kernel is csrc/gap.hip
(``ops/hip.py:gap_enum``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import count as C
from . import reference as ref
from .rate import offset_vectors, profile_rows

PRUNED, LEAF, INNER = 0, 1, 2


@dataclass
class NodeBound:
    ub: torch.Tensor          # [N] fp32 upper bound of the node's largest gap
    pair: torch.Tensor        # [N] int64 best pair (-1: no pair)
    orient: torch.Tensor      # [N] int64 0: A, 1: B
    c: torch.Tensor           # [N, n] fp32 coefficients of the best pair (0 on PA dims)
    cand_x: torch.Tensor      # [N, n] fp32 candidate x (the maximising corner)
    cand_xp: torch.Tensor     # [N, n] fp32 its counterpart


def round_up32(v: torch.Tensor) -> torch.Tensor:
    """fp64 -> fp32 rounded up: cast, then one step up unless the cast did not round down."""
    f = v.to(torch.float32)
    up = torch.nextafter(f, torch.full_like(f, math.inf))
    return torch.where(f.double() < v, up, f)


def _first_argmax(x: torch.Tensor) -> torch.Tensor:
    """Index of the first maximum along dim 1 of ``x`` [N, K] (K >= 1, no NaN)."""
    K = x.shape[1]
    ar = torch.arange(K, device=x.device)[None].expand_as(x)
    m = x.max(dim=1, keepdim=True).values
    return torch.where(x == m, ar, torch.full_like(ar, K)).min(dim=1).values.clamp(max=K - 1)


def cert_poss(lx, ux, lxp, uxp):
    """(cert, poss) fp64 of broadcastable rigorous fp32 bounds of ``x`` and ``x'``: a certain lower
    and a possible upper value of ``|N(x) - N(x')|``.  The subtractions run in fp64 (exact for fp32
    operands up to an exponent gap of 29 bits) and are widened by ``gamma(1, FP64_UNIT)`` of the
    operands' magnitudes.  A NaN gives -inf / +inf."""
    g = ref.gamma(1, ref.FP64_UNIT)
    lx, ux, lxp, uxp = (t.double() for t in (lx, ux, lxp, uxp))

    def lo_(a, b):
        return (a - b) - g * (a.abs() + b.abs())

    def hi_(a, b):
        return (a - b) + g * (a.abs() + b.abs())

    cert = torch.maximum(lo_(lxp, ux), lo_(lx, uxp))
    poss = torch.maximum(hi_(uxp, lx), hi_(ux, lxp))
    cert = torch.where(cert.isnan(), torch.full_like(cert, -math.inf), cert)
    poss = torch.where(poss.isnan(), torch.full_like(poss, math.inf), poss)
    return cert, poss


def node_forms(be, q, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor):
    """Bound results of the nodes' x rows and counterpart rows (the same object when not relaxed)."""
    rlo, rhi, plo, phi = C.node_rows(q, lo.to(torch.float32), hi.to(torch.float32), values)
    fold = tuple(q.pa_idx)
    rx = be.bounds(rlo, rhi, mode="symbolic", crown=True, fold=fold)
    rp = be.bounds(plo, phi, mode="symbolic", crown=True, fold=fold) if q.relaxed else rx
    return rx, rp


def node_ub_from(q, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor, rx, rp) -> NodeBound:
    """The node bound from the bound results ``rx`` / ``rp`` of the node rows [N V]."""
    lo, hi = lo.to(torch.float32), hi.to(torch.float32)
    N, n = lo.shape
    V, Pp = values.shape[0], pairs.shape[0]
    dev = lo.device
    if Pp == 0 or N == 0:
        z = torch.zeros(N, dtype=torch.float32, device=dev)
        return NodeBound(z, torch.full((N,), -1, dtype=torch.int64, device=dev),
                         torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, n, device=dev), lo.clone(), lo.clone())
    pa = torch.tensor(list(q.pa_idx), dtype=torch.long, device=dev)
    is_pa = torch.zeros(n, dtype=torch.bool, device=dev)
    is_pa[pa] = True
    is_ra = torch.zeros(n, dtype=torch.bool, device=dev)
    tau = 0.0
    if q.relaxed:
        is_ra[torch.tensor(list(q.ra_idx), dtype=torch.long, device=dev)] = True
        tau = float(q.tau)
    vi, vj = pairs[:, 0].to(dev), pairs[:, 1].to(dev)
    vals = values.to(dev, torch.float64)
    lo64, hi64 = lo.double()[:, None, :], hi.double()[:, None, :]
    m64 = torch.maximum(lo64.abs(), hi64.abs())
    gam = ref.gamma(2 * n + 8, ref.FP64_UNIT)
    g1 = ref.gamma(1, ref.FP64_UNIT)

    def rows(r, idx):
        f = lambda t: t.view(N, V, -1)[:, idx]                                       # noqa: E731
        return (f(r.Lc), f(r.L0)[..., 0], f(r.Le)[..., 0], f(r.Uc), f(r.U0)[..., 0], f(r.Ue)[..., 0],
                f(r.out_lb)[..., 0], f(r.out_ub)[..., 0])

    Lc, L0, Le, Uc, U0, Ue, lb, ub = rows(rx, vi)
    Lcp, L0p, Lep, Ucp, U0p, Uep, lbp, ubp = rows(rp, vj)

    def orient(cU, u0, ue, vu, cL, l0, le, vl, cpart, iu, il):
        # max of U(.) + ue - L(.) + le over the node: cU / cL [N, Pp, n] fp32, vu / vl the PA rows
        a, b = cU.double(), cL.double()
        c = a - b
        free = torch.maximum(c * lo64, c * hi64).masked_fill(is_pa, 0.0)
        mfree = ((a.abs() + b.abs()) * m64).masked_fill(is_pa, 0.0)
        pu = a[:, :, pa] * vals[vu][None]
        pl = b[:, :, pa] * vals[vl][None]
        rterm = (tau * cpart.double().abs()).masked_fill(~is_ra, 0.0)
        val = free.sum(-1) + rterm.sum(-1) + pu.sum(-1) - pl.sum(-1) + u0.double() + ue.double() - l0.double() + le.double()
        mag = mfree.sum(-1) + rterm.sum(-1) + pu.abs().sum(-1) + pl.abs().sum(-1) + u0.double().abs() \
            + ue.double().abs() + l0.double().abs() + le.double().abs()
        form = val + gam * mag
        iv = (iu.double() - il.double()) + g1 * (iu.double().abs() + il.double().abs())
        form = torch.where(form.isnan(), torch.full_like(form, math.inf), form)
        iv = torch.where(iv.isnan(), torch.full_like(iv, math.inf), iv)
        return torch.minimum(form, iv), (cU - cL).masked_fill(is_pa, 0.0)

    bA, cA = orient(Ucp, U0p, Uep, vj, Lc, L0, Le, vi, Ucp, ubp, lb)
    bB, cB = orient(Uc, U0, Ue, vi, Lcp, L0p, Lep, vj, Lcp, ub, lbp)
    both = torch.stack([bA, bB], dim=2).reshape(N, 2 * Pp)                          # pair-major, A before B
    k = _first_argmax(both)
    ar = torch.arange(N, device=dev)
    p, o = k // 2, k % 2
    c = torch.where((o == 0)[:, None], cA[ar, p], cB[ar, p])
    sgn = torch.where((o == 0)[:, None], Ucp[ar, p] >= 0, Lcp[ar, p] <= 0)
    x = torch.where(c >= 0, hi, lo)
    xp = x + torch.where(sgn, tau, -tau) * is_ra.to(torch.float32)
    x[:, pa] = values.to(dev, torch.float32)[vi[p]]
    xp[:, pa] = values.to(dev, torch.float32)[vj[p]]
    return NodeBound(round_up32(both[ar, k]), p, o, c, x, xp)


def node_ub_ref(be, q, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor) -> NodeBound:
    """Upper bound of the largest gap inside each node box ``lo, hi`` [N, n], its best pair and
    orientation, the pair's fp32 coefficients and the candidate rows."""
    rx, rp = node_forms(be, q, lo, hi, values)
    return node_ub_from(q, lo, hi, values, pairs, rx, rp)


def level_ref(q, lo: torch.Tensor, hi: torch.Tensor, part: torch.Tensor, ub: torch.Tensor, c: torch.Tensor,
              inc_start: torch.Tensor, tol: float, leaf_points: int, score: torch.Tensor):
    """Level step over nodes [N, n]: (codes [N] uint8 PRUNED / LEAF / INNER, split dims [N] int64,
    children ``(clo, chi, cpart)`` -- node order, two per INNER node --, leaves ``(llo, lhi, lpart)``).
    ``inc_start`` [P] fp64: the partitions' incumbents at the start of the level."""
    N, n = lo.shape
    dev = lo.device
    free = C.free_dims(q)
    f = torch.as_tensor(free, dtype=torch.long, device=dev)
    vol = C.volumes(lo, hi, free)
    pruned = ub.double() <= inc_start.to(dev, torch.float64)[part.long()] + float(tol)
    w = (hi[:, f] - lo[:, f]).to(torch.float32)
    prod = c.to(torch.float32)[:, f].abs() * w
    prod = torch.where(prod.isnan(), torch.zeros_like(prod), prod)
    neg = torch.full_like(prod, -1.0)
    prod = torch.where(w > 0, prod, neg)
    ssc = torch.where(w > 0, w * score.to(dev, torch.float32)[f][None], neg)
    sc = torch.where((prod > 0).any(dim=1, keepdim=True), prod, ssc)
    dim = f[_first_argmax(sc)] if N and len(free) else torch.zeros(N, dtype=torch.long, device=dev)
    can = (w > 0).any(dim=1)
    leaf = ~pruned & ((vol <= int(leaf_points)) | ~can)
    inner = ~pruned & ~leaf
    code = torch.full((N,), PRUNED, dtype=torch.uint8, device=dev)
    code[leaf] = LEAF
    code[inner] = INNER
    clo, chi = C.halves(lo[inner], hi[inner], dim[inner])
    return code, dim, (clo, chi, part[inner].repeat_interleave(2)), (lo[leaf], hi[leaf], part[leaf])


def enum_gap_ref(be, q, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor,
                 sub: int = 16384):
    """Reference enumeration of ``L`` leaves: (``leaf_lo`` [L] fp64, ``leaf_hi`` [L] fp64, ``arg_s``,
    ``arg_pair``, ``arg_e`` [L] int32: the argument of ``leaf_lo``)."""
    L, n = lo.shape
    dev = lo.device
    free = C.free_dims(q)
    vol = C.volumes(lo, hi, free).cpu().numpy()
    if L and int(vol.max()) > C.MAX_LEAF_POINTS:
        raise ValueError(f"gap: a leaf of {int(vol.max())} points exceeds the limit of {C.MAX_LEAF_POINTS}")
    V, Pp = values.shape[0], pairs.shape[0]
    E = offset_vectors(q).shape[0]
    leaf_lo = torch.zeros(L, dtype=torch.float64, device=dev)
    leaf_hi = torch.zeros(L, dtype=torch.float64, device=dev)
    arg = torch.full((3, L), -1, dtype=torch.int32, device=dev)
    if Pp == 0:
        return leaf_lo, leaf_hi, arg[0], arg[1], arg[2]
    vi, vj = pairs[:, 0].to(dev), pairs[:, 1].to(dev)
    K = Pp * E
    k0 = 0
    while k0 < L:                               # leaves batched up to ``sub`` points per forward
        k1, pts = k0 + 1, int(vol[k0])
        while k1 < L and pts + int(vol[k1]) <= sub:
            pts += int(vol[k1])
            k1 += 1
        vt = torch.from_numpy(vol[k0:k1]).to(dev)
        lid = torch.repeat_interleave(torch.arange(k1 - k0, device=dev), vt)          # leaf of each point
        s = torch.arange(pts, device=dev) - torch.repeat_interleave(vt.cumsum(0) - vt, vt)
        X = C.lattice_points_at(lo[k0:k1][lid].to(torch.float32), hi[k0:k1][lid].to(torch.float32), free, s[:, None])[:, 0]
        XV, XP = profile_rows(q, X, values)
        lx, ux = be.point_bounds(XV.reshape(-1, n))
        lx, ux = lx.view(pts, 1, V), ux.view(pts, 1, V)
        if q.relaxed:
            lxp, uxp = be.point_bounds(XP.reshape(-1, n))
            lxp, uxp = lxp.view(pts, E, V), uxp.view(pts, E, V)
        else:
            lxp, uxp = lx, ux
        cert, poss = cert_poss(lx[:, :, vi], ux[:, :, vi], lxp[:, :, vj], uxp[:, :, vj])   # [pts, E, Pp]
        cert = cert.permute(0, 2, 1).reshape(-1)                                     # key order (s, pair, e)
        kid = lid.repeat_interleave(K)
        top = torch.full((k1 - k0,), -math.inf, dtype=cert.dtype, device=dev).scatter_reduce(0, kid, cert, "amax")
        key = s.repeat_interleave(K) * K + torch.arange(K, device=dev).repeat(pts)
        big = torch.full((k1 - k0,), 2 ** 62, dtype=torch.int64, device=dev)
        first = big.scatter_reduce(0, kid, torch.where(cert == top[kid], key, big[kid]), "amin")
        leaf_lo[k0:k1] = top
        leaf_hi[k0:k1] = torch.full((k1 - k0,), -math.inf, dtype=poss.dtype, device=dev).scatter_reduce(
            0, kid, poss.reshape(-1), "amax")
        arg[0, k0:k1] = (first // K).to(torch.int32)
        arg[1, k0:k1] = ((first % K) // E).to(torch.int32)
        arg[2, k0:k1] = (first % E).to(torch.int32)
        k0 = k1
    return leaf_lo, leaf_hi, arg[0], arg[1], arg[2]


def witness_rows(q, lo: np.ndarray, hi: np.ndarray, values: np.ndarray, pairs: np.ndarray, s, pair, e):
    """Arguments ``(s, pair, e)`` [M] of the boxes ``lo, hi`` [M, n] (int64) -> rows ``x, x'`` [M, n] int64."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    s, pair, e = (np.asarray(t, np.int64).reshape(-1) for t in (s, pair, e))
    X = C.lattice_points_at(torch.from_numpy(lo), torch.from_numpy(hi), C.free_dims(q),
                            torch.from_numpy(s)[:, None])[:, 0].numpy()
    x, xp = X.copy(), X.copy()
    pa = list(q.pa_idx)
    x[:, pa] = values[pairs[pair, 0]]
    xp[:, pa] = values[pairs[pair, 1]]
    if q.relaxed:
        xp[:, list(q.ra_idx)] += offset_vectors(q)[e]
    return x, xp
