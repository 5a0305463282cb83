"""Single-attribute neighbourhood of real individuals: rigorous per-(row, neighbour) bits on the
device, exact resolution of what fp32 cannot decide on the host.

``audit_neighbours`` decides, for every row of a table of individuals and every entry of the
neighbour table (``ops/neighbours.py``: the row with ONE non-protected attribute set to another
value of its domain, within a radius), whether that neighbour is a discriminated individual in
``engine/audit.py``'s sense: some counterpart of the neighbour flips the sign of its logit strictly.
The rigorous point bounds settle almost every bit; the ambiguous bits ``poss & ~cert`` are decided
with ``exact.exact_signs`` in one vectorised pass, so ``flag`` is a function of (network, query,
row, radii) only.  ``exposure`` turns the bits into per-feature counts, the nearest flagged value
and the row classes *flagged* / *exposed* / *robust*.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import audit as A
from ..ops import neighbours as NB
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from . import exact
from .audit import counterparts


@dataclass
class NeighbourResult:
    table: NB.NeighbourTable
    own: np.ndarray                       # [N] int32      index into the PA-domain table, -1: not audited
    cert: np.ndarray                      # [N, W] uint32  bit j: neighbour j is certainly flagged
    poss: np.ndarray                      # [N, W] uint32  bit j: possibly flagged
    flag: np.ndarray                      # [N, W] uint32  exact bits (with resolve), else cert
    ambiguous: int                        # bits the rigorous bounds left undecided
    ambiguous_left: int                   # of those, bits still undecided (0 with resolve)
    fused: bool = False                   # the bits came from the fused kernel


@dataclass
class Exposure:
    count: np.ndarray                     # [N, n] int64  flagged neighbours through feature k
    nearest: np.ndarray                   # [N, n] int64  signed delta of the nearest one (0: none)
    flagged: np.ndarray                   # [N] bool      the row itself is flagged
    exposed: np.ndarray                   # [N] bool      not flagged, some neighbour is
    robust: np.ndarray                    # [N] bool      audited, neither


def device_words(be: Backend, q: ResolvedQuery, X: np.ndarray, own: np.ndarray, values: np.ndarray,
                 pairs: np.ndarray, table: NB.NeighbourTable):
    """(cert, poss uint32 [N, W], fused): the fused kernel when ``be.hip``, it is not switched off
    (``FAIRIFY_NEIGHBOURS_FUSED=0``) and it covers the shape, otherwise the reference / composed path."""
    dev = be.device
    Xt = torch.from_numpy(X).to(dev)
    ot = torch.from_numpy(own).to(dev)
    vt, pt = torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)
    out = None
    if be.hip:
        from ..ops import hip

        if hip.neighbours_fused():
            out = hip.neighbour_masks(be, q, Xt.to(torch.float32), ot, vt, pt, table)
    fused = out is not None
    if out is None:
        out = NB.neighbour_masks_ref(be, q, Xt, ot, vt, pt, table)
    cert, poss = (np.ascontiguousarray(t.cpu().numpy()) for t in out)
    return cert.view(np.uint32), poss.view(np.uint32), fused


def _popcount(words: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def audit_neighbours(be: Backend, q: ResolvedQuery, X, radii=None, resolve: bool = True) -> NeighbourResult:
    """Decide every single-attribute neighbour of rows ``X`` [N, n] (integral) under ``radii``
    (``ops/neighbours.radius_array``).  With ``resolve`` the ambiguous bits are decided exactly and
    ``flag`` is exact; without, ``flag = cert`` and the exact bits lie between ``cert`` and ``poss``."""
    X = A.integral_rows(X)
    if X.shape[1] != q.n:
        raise ValueError(f"neighbours: rows have {X.shape[1]} columns, the domain {q.n}")
    table = radii if isinstance(radii, NB.NeighbourTable) else NB.neighbour_table(q, radii)
    values, pairs = A.pa_domain_table(q)
    V = values.shape[0]
    own = A.own_index(q, X, values)
    cert, poss, fused = device_words(be, q, X, own, values, pairs, table)
    flag = cert.copy()
    ambw = poss & ~cert
    some = np.nonzero(ambw.any(axis=1))[0]                          # the few rows with an ambiguous bit
    sub, js = np.nonzero(NB.unpack_bits(ambw[some], table.M))
    ambiguous = left = int(len(js))
    if resolve and ambiguous:
        rows = some[sub]                                            # K ambiguous (row, neighbour) bits
        Z = X[rows].copy()                                          # their neighbours, materialised
        d = table.dim[js].astype(np.int64)
        Z[np.arange(len(rows)), d] = np.where(table.abs[js] != 0, table.off[js].astype(np.int64),
                                              Z[np.arange(len(rows)), d] + table.off[js])
        allowed = np.zeros((V, V), dtype=bool)
        allowed[pairs[:, 0], pairs[:, 1]] = True
        k, vp = np.nonzero(allowed[own[rows]])                      # every (bit, allowed v') combination
        s_z = exact.exact_signs(be.mlp, Z)
        XP = counterparts(q, Z[k], vp, values)                      # [K', E, n]
        s_cp = exact.exact_signs(be.mlp, XP.reshape(-1, X.shape[1])).reshape(len(k), -1)
        hit = np.zeros(len(rows), dtype=bool)
        np.logical_or.at(hit, k, (s_z[k][:, None] * s_cp < 0).any(axis=1))
        np.bitwise_or.at(flag, (rows[hit], js[hit] // 32), np.uint32(1) << (js[hit] % 32).astype(np.uint32))
        left = 0
    return NeighbourResult(table=table, own=own, cert=cert, poss=poss, flag=flag, ambiguous=ambiguous,
                           ambiguous_left=left, fused=fused)


def exposure(res: NeighbourResult, X, own_flagged) -> Exposure:
    """Per row and feature the flagged neighbours and the signed delta ``c - x_k`` of the nearest one
    (on a tie the negative delta; 0: none), and the row classes given ``own_flagged`` [N], the rows
    ``engine.audit.audit_rows`` flags themselves."""
    X = A.integral_rows(X)
    N, n = X.shape
    t = res.table
    bits = NB.unpack_bits(res.flag, t.M)
    delta = NB.deltas(X, t)
    count = np.zeros((N, n), dtype=np.int64)
    nearest = np.zeros((N, n), dtype=np.int64)
    none = np.iinfo(np.int64).max
    for k in np.unique(t.dim):
        cols = np.nonzero(t.dim == k)[0]
        b, dl = bits[:, cols], delta[:, cols]
        count[:, k] = b.sum(axis=1)
        key = np.where(b, 2 * np.abs(dl) + (dl > 0), none)          # smallest |delta|, the negative one first
        best = key.argmin(axis=1)
        nearest[:, k] = np.where(b.any(axis=1), dl[np.arange(N), best], 0)
    audited = res.own >= 0
    flagged = np.asarray(own_flagged, dtype=bool) & audited
    any_nb = count.sum(axis=1) > 0
    return Exposure(count=count, nearest=nearest, flagged=flagged, exposed=audited & ~flagged & any_nb,
                    robust=audited & ~flagged & ~any_nb)
