"""Counting branch-and-bound: the node rows, the box test, the split and the leaf enumeration.

A *node* is an integer sub-box ``lo, hi`` [n] (float32, integral) of a partition; its PA dims keep
the partition's PA range, its volume is ``prod_{d not in PA} (hi_d - lo_d + 1)`` (int64).

* box test: the node's ``x`` rows are its box with the PA dims pinned to each ``values[v]``, the
  counterpart rows the same rows (PA-only query) or those rows with every RA dim widened by
  ``tau`` on both sides.  With ``[l, u]`` / ``[l', u']`` the logit intervals of the rows
  (``Backend.bounds(mode="symbolic", crown=True)``), a node is UNFAIR if some pair ``(v, v')`` has
  ``u_v < 0 < l'_v'`` or ``l_v > 0 > u'_v'`` (every lattice point flips, with offset 0), FAIR if
  no pair has ``l_v < 0 < u'_v'`` or ``u_v > 0 > l'_v'`` (no lattice point flips with any
  offset: the widened box contains every shifted point), OPEN otherwise -- the four comparisons
  of ``ops/rate.classify`` over boxes;
* split: along the non-PA dim with ``hi_d > lo_d`` of the largest fp32 product
  ``(hi_d - lo_d) * s_d`` (lowest ``d`` on ties), ``s_d = sum_j |W_0[d, j]|``, into
  ``[lo_d, m]`` and ``[m + 1, hi_d]`` with ``m = lo_d + floor((hi_d - lo_d) / 2)``;
* enumeration: point ``s`` in ``[0, vol)`` of a leaf is the mixed-radix decode over the non-PA
  dims in increasing dim order, last dim fastest, classified like a rate profile
  (``ops/rate.rate_flags_ref``).

This module is the reference (any backend); the kernels are csrc/count.hip (``ops/hip.py``:
``count_rows``, ``count_level``, ``count_enum``).
"""
from __future__ import annotations

import numpy as np
import torch

from .rate import rate_flags_ref

OPEN, FAIR, UNFAIR = 0, 1, 2
MAX_LEAF_POINTS = 65536   # launch-shape limit of fa_count_enum_kernel (FA_COUNT_MAX_VOL)


def free_dims(q):
    """The non-PA dims, increasing."""
    return [d for d in range(q.n) if d not in q.pa_idx]


def split_scores(mlp) -> torch.Tensor:
    """``s_d = sum_j |W_0[d, j]|`` [n0]: summed in fp64, cast to fp32 once."""
    return torch.from_numpy(np.abs(np.asarray(mlp.weights[0], np.float64)).sum(axis=1).astype(np.float32))


def volumes(lo: torch.Tensor, hi: torch.Tensor, free) -> torch.Tensor:
    """Non-PA lattice points of boxes [N, n]: int64 [N]."""
    f = torch.as_tensor(list(free), dtype=torch.long, device=lo.device)
    return ((hi[:, f] - lo[:, f]).to(torch.int64) + 1).prod(dim=1)


def node_rows(q, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor):
    """Node boxes [N, n] -> node-major ``x`` rows ``rlo, rhi`` [N V, n] and counterpart rows
    ``plo, phi`` [N V, n] (the x rows themselves for a PA-only query)."""
    N, n = lo.shape
    V = values.shape[0]
    pa = torch.tensor(list(q.pa_idx), device=lo.device, dtype=torch.long)
    rlo = lo[:, None, :].expand(N, V, n).clone()
    rhi = hi[:, None, :].expand(N, V, n).clone()
    vv = values.to(lo.dtype)[None].expand(N, V, -1)
    rlo[:, :, pa] = vv
    rhi[:, :, pa] = vv
    rlo, rhi = rlo.reshape(N * V, n), rhi.reshape(N * V, n)
    if not q.relaxed:
        return rlo, rhi, rlo, rhi
    ra = torch.tensor(list(q.ra_idx), device=lo.device, dtype=torch.long)
    plo, phi = rlo.clone(), rhi.clone()
    plo[:, ra] -= float(q.tau)
    phi[:, ra] += float(q.tau)
    return rlo, rhi, plo, phi


def box_codes_ref(lx, ux, lxp, uxp, pairs: torch.Tensor) -> torch.Tensor:
    """Class codes [N] uint8 (OPEN / FAIR / UNFAIR) from the x-row bounds [N, V], the
    counterpart-row bounds [N, V] and ``pairs`` [Pp, 2]."""
    vi, vj = pairs[:, 0], pairs[:, 1]
    li, ui = lx[:, vi], ux[:, vi]
    lj, uj = lxp[:, vj], uxp[:, vj]
    unfair = (((ui < 0) & (lj > 0)) | ((li > 0) & (uj < 0))).any(dim=1)
    poss = (((li < 0) & (uj > 0)) | ((ui > 0) & (lj < 0))).any(dim=1)
    code = torch.full((lx.shape[0],), FAIR, dtype=torch.uint8, device=lx.device)
    code[poss] = OPEN
    code[unfair] = UNFAIR
    return code


def split_ref(lo: torch.Tensor, hi: torch.Tensor, free, score: torch.Tensor):
    """Halve nodes [N, n] (each with a non-PA dim of width > 0): (split dims [N], child boxes
    ``clo, chi`` [2 N, n]: node k's children are rows 2k, 2k + 1)."""
    N, n = lo.shape
    f = torch.as_tensor(list(free), dtype=torch.long, device=lo.device)
    w = (hi[:, f] - lo[:, f]).to(torch.float32)
    sc = w * score.to(lo.device, torch.float32)[f][None]
    sc = torch.where(w > 0, sc, torch.full_like(sc, -1.0))
    dim = f[sc.argmax(dim=1)] if N else torch.zeros(0, dtype=torch.long, device=lo.device)
    return (dim,) + halves(lo, hi, dim)


def halves(lo: torch.Tensor, hi: torch.Tensor, dim: torch.Tensor):
    """Child boxes ``clo, chi`` [2 N, n] of nodes [N, n] halved along ``dim`` [N] (int64): node k's
    children are rows 2k, 2k + 1."""
    N, n = lo.shape
    ar = torch.arange(N, device=lo.device)
    l, h = lo[ar, dim], hi[ar, dim]
    m = l + torch.floor((h - l) / 2)
    clo = lo[:, None, :].expand(N, 2, n).clone()
    chi = hi[:, None, :].expand(N, 2, n).clone()
    chi[ar, 0, dim] = m
    clo[ar, 1, dim] = m + 1
    return clo.reshape(2 * N, n), chi.reshape(2 * N, n)


def lattice_points_at(lo: torch.Tensor, hi: torch.Tensor, free, idx: torch.Tensor) -> torch.Tensor:
    """Points ``idx`` [L, K] (int64) of the boxes ``lo, hi`` [L, n]: [L, K, n] in ``lo``'s dtype.
    The PA dims carry ``lo``; the digits of an index run over the non-PA dims, last dim fastest."""
    L, n = lo.shape
    X = lo[:, None, :].expand(L, idx.shape[1], n).clone()
    rest = idx.to(torch.int64).clone()
    for d in reversed(list(free)):
        w = ((hi[:, d] - lo[:, d]).to(torch.int64) + 1)[:, None]
        X[:, :, d] = lo[:, d, None] + (rest % w).to(lo.dtype)
        rest = rest // w
    return X


def enum_counts_ref(be, q, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor,
                    sub: int = 16384):
    """Reference enumeration of ``L`` leaves: (certain points [L] int32, ambiguous points [L]
    int32, a list of the leaves' ambiguous masks, bool [vol_k] each)."""
    L = lo.shape[0]
    dev = lo.device
    free = free_dims(q)
    vol = volumes(lo, hi, free).cpu().numpy()
    if L and int(vol.max()) > MAX_LEAF_POINTS:
        raise ValueError(f"count: a leaf of {int(vol.max())} points exceeds the limit of {MAX_LEAF_POINTS}")
    cert = torch.zeros(L, dtype=torch.int32, device=dev)
    amb = torch.zeros(L, dtype=torch.int32, device=dev)
    masks = []
    k0 = 0
    while k0 < L:                               # leaves batched up to ``sub`` points per forward
        k1, pts = k0 + 1, int(vol[k0])
        while k1 < L and pts + int(vol[k1]) <= sub:
            pts += int(vol[k1])
            k1 += 1
        X = torch.cat([lattice_points_at(lo[k:k + 1], hi[k:k + 1], free,
                                         torch.arange(int(vol[k]), device=dev)[None])[0] for k in range(k0, k1)])
        c, p = rate_flags_ref(be, q, X, values, pairs)
        a = p & ~c
        o = 0
        for k in range(k0, k1):
            v = int(vol[k])
            cert[k] = int(c[o:o + v].sum())
            amb[k] = int(a[o:o + v].sum())
            masks.append(a[o:o + v].clone())
            o += v
        k0 = k1
    return cert, amb, masks
