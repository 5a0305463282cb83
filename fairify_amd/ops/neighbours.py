"""Single-attribute neighbourhood of real individuals: the neighbour table, the materialised
neighbours and the rigorous per-(row, neighbour) bits.

For a resolved query ``q``, integral rows ``X`` [N, n] and a radius ``r_k`` per non-PA feature
(*full* or an integer >= 0; 0 leaves the feature out) -- docs/DESIGN.md 5g:

* the neighbour of row ``x`` through a non-PA feature ``k`` and a value ``c`` is ``z = x`` with
  ``z_k := c``; it is valid when ``lo_k <= c <= hi_k`` (the domain range), ``c != x_k`` and
  ``|c - x_k| <= r_k``.  A row coordinate outside its range is allowed;
* the neighbour table, built once per call and ordered by feature, then by value or offset, has one
  entry ``(dim, off, abs)`` per candidate: a feature whose radius is full or ``>= hi_k - lo_k`` gets
  the absolute entries ``c = lo_k .. hi_k``, any other feature the relative entries
  ``c = x_k + off``, ``off = -r_k .. r_k`` without 0.  ``M`` entries, ``W = ceil(M / 32)`` words;
* bit ``j % 32`` of word ``j / 32`` of ``cert`` / ``poss`` [N, W] is neighbour j of the row: the
  neighbour is valid and ``ops/audit.py``'s cert / poss mask *of the neighbour* (own index, pairs,
  counterparts and bounds exactly those of the audit) has some bit set.  Invalid neighbours, padding
  bits and rows outside the PA domain give 0.

``cert <= exact flag <= poss`` per bit.  This module is the reference on any backend -- on a CUDA
backend it is the composed device path (the audit kernel fed materialised neighbours in chunks); the
fused kernel is ``ops/hip.py:neighbour_masks`` (csrc/neighbours.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import audit as A

MAX_NEIGHBOURS = 4096     # table entries per call
FULL = 2 ** 31 - 1        # a full radius, as the kernel reads it (INT_MAX)
_REF_ROWS = 1 << 17       # materialised neighbour rows per chunk of the reference


@dataclass(frozen=True)
class NeighbourTable:
    dim: np.ndarray       # [M] int32  the overwritten (non-PA) coordinate
    off: np.ndarray       # [M] int32  its new value (abs) or the offset from the row's own (relative)
    abs: np.ndarray       # [M] int32  1: absolute entry
    radius: np.ndarray    # [n] int64  per feature; FULL: full, 0: left out (PA features: 0)
    lo: np.ndarray        # [n] int64  domain range
    hi: np.ndarray

    @property
    def M(self) -> int:
        return int(self.dim.shape[0])

    @property
    def W(self) -> int:
        return (self.M + 31) // 32


def _one_radius(r, what: str) -> int:
    if r is None or (isinstance(r, str) and r.strip().lower() == "full"):
        return FULL
    try:
        v = int(r)
    except (TypeError, ValueError):
        raise ValueError(f"neighbours: radius {r!r} of {what} is neither a non-negative integer nor 'full'")
    if v < 0 or (not isinstance(r, str) and v != r):
        raise ValueError(f"neighbours: radius {r!r} of {what} is neither a non-negative integer nor 'full'")
    return min(v, FULL)


def radius_array(q, radii=None) -> np.ndarray:
    """Per-feature radii [n] int64 (FULL: full; PA features 0).  ``radii``: ``None`` or ``'full'``
    (full everywhere), one integer, a dict ``name -> integer | 'full'`` (with an optional
    ``'*'`` entry for the features it does not name, default full), or a sequence over all n features."""
    dom = q.domain
    n = dom.n
    if isinstance(radii, dict):
        unknown = [k for k in radii if k != "*" and not dom.has(k)]
        if unknown:
            raise ValueError(f"neighbours: radius given for {unknown}, not features of domain {dom.suite}")
        named_pa = [k for k in radii if k != "*" and dom.index(k) in q.pa_idx]
        if named_pa:
            raise ValueError(f"neighbours: {named_pa} are protected attributes and have no radius")
        base = _one_radius(radii.get("*"), "*")
        out = [_one_radius(radii[f.name], f.name) if f.name in radii else base for f in dom.features]
    elif radii is None or isinstance(radii, (str, int, np.integer)):
        out = [_one_radius(radii, "every feature")] * n
    else:
        if len(radii) != n:
            raise ValueError(f"neighbours: {len(radii)} radii for {n} features")
        out = [_one_radius(r if not isinstance(r, np.generic) else r.item(), dom.features[k].name)
               for k, r in enumerate(radii)]
    out = np.array(out, dtype=np.int64)
    out[list(q.pa_idx)] = 0
    return out


def neighbour_table(q, radii=None) -> NeighbourTable:
    """The neighbour table of ``q`` under ``radii`` (see :func:`radius_array`).  More than
    ``MAX_NEIGHBOURS`` entries raise ``ValueError``: give the wide features a radius."""
    rad = radius_array(q, radii)
    lo, hi = q.domain.lo(), q.domain.hi()
    dim, off, ab = [], [], []
    M = 0
    for k in range(q.n):
        r = int(rad[k])
        if r == 0:
            continue
        full = r >= int(hi[k] - lo[k])
        M += int(hi[k] - lo[k] + 1) if full else 2 * r
        if M > MAX_NEIGHBOURS:
            raise ValueError(f"neighbours: more than {MAX_NEIGHBOURS} neighbours per row (at feature "
                             f"{q.domain.features[k].name!r}, range {int(lo[k])}..{int(hi[k])}): give it a radius")
        cs = range(int(lo[k]), int(hi[k]) + 1) if full else [o for o in range(-r, r + 1) if o]
        dim += [k] * len(cs)
        off += list(cs)
        ab += [int(full)] * len(cs)
    return NeighbourTable(dim=np.array(dim, dtype=np.int32), off=np.array(off, dtype=np.int32),
                          abs=np.array(ab, dtype=np.int32), radius=rad, lo=lo, hi=hi)


def neighbour_rows(q, X, table: NeighbourTable) -> Tuple[np.ndarray, np.ndarray]:
    """(Z [N, M, n] int64, valid [N, M] bool): every table entry applied to every row."""
    X = np.asarray(X, dtype=np.int64)
    c, valid = neighbour_values(X, table)
    Z = np.repeat(X[:, None, :], table.M, axis=1)
    Z[:, np.arange(table.M), table.dim.astype(np.int64)] = c
    return Z, valid


def neighbour_values(X, table: NeighbourTable) -> Tuple[np.ndarray, np.ndarray]:
    """(c [N, M] int64, valid [N, M] bool): the new value of every (row, entry) and its validity."""
    X = np.asarray(X, dtype=np.int64)
    d = table.dim.astype(np.int64)
    xk = X[:, d]                                                                      # [N, M]
    c = np.where(table.abs[None] != 0, table.off[None].astype(np.int64), xk + table.off[None])
    valid = (c >= table.lo[d][None]) & (c <= table.hi[d][None]) & (c != xk) & (np.abs(c - xk) <= table.radius[d][None])
    return c, valid


def deltas(X, table: NeighbourTable) -> np.ndarray:
    """``c - x_k`` of every (row, entry): [N, M] int64."""
    X = np.asarray(X, dtype=np.int64)
    xk = X[:, table.dim.astype(np.int64)]
    return np.where(table.abs[None] != 0, table.off[None].astype(np.int64) - xk, table.off[None].astype(np.int64))


def pack_bits(bits: torch.Tensor, W: int) -> torch.Tensor:
    """bool [N, M] -> int32 words [N, W], bit j % 32 of word j / 32."""
    N, M = bits.shape
    full = torch.zeros(N, W * 32, dtype=torch.int64, device=bits.device)
    full[:, :M] = bits.to(torch.int64)
    w = (full.view(N, W, 32) << torch.arange(32, device=bits.device)).sum(dim=2)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bits(words: np.ndarray, M: int) -> np.ndarray:
    """uint32 words [N, W] -> bool [N, M]."""
    words = np.ascontiguousarray(words).view(np.uint32)
    b = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None]) & np.uint32(1)
    return b.reshape(words.shape[0], 32 * words.shape[1])[:, :M].astype(bool)


def neighbour_masks_ref(be, q, X: torch.Tensor, own: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor,
                        table: NeighbourTable, sub: int = 4096):
    """Reference words of rows ``X`` [N, n]: (cert, poss) int32 [N, W] on ``X``'s device.  The
    neighbours are materialised in chunks of at most ``sub`` rows and audited as rows of their own
    (``ops/audit.audit_masks_ref``; on a HIP backend the audit kernel where it covers the shape): a
    bit is set when any bit of the neighbour's mask is set and the neighbour is valid."""
    N, n = X.shape
    M, W = table.M, table.W
    dev = X.device
    cert = torch.zeros(N, W, dtype=torch.int32, device=dev)
    poss = torch.zeros(N, W, dtype=torch.int32, device=dev)
    if not N or not M:
        return cert, poss
    X = X.to(torch.int64)
    own = own.to(dev, torch.int32)
    values, pairs = values.to(dev), pairs.to(dev)
    d = torch.from_numpy(table.dim.astype(np.int64)).to(dev)
    off = torch.from_numpy(table.off.astype(np.int64)).to(dev)
    ab = torch.from_numpy(table.abs != 0).to(dev)
    lo, hi = torch.from_numpy(table.lo).to(dev)[d], torch.from_numpy(table.hi).to(dev)[d]
    rad = torch.from_numpy(table.radius).to(dev)[d]
    audit = A.audit_masks_ref
    if getattr(be, "hip", False):
        from . import hip

        def audit(be_, q_, Z, o, v, p):
            out = hip.audit_masks(be_, q_, Z, o, v, p)
            return out if out is not None else A.audit_masks_ref(be_, q_, Z, o, v, p)
    sub = max(1, min(int(sub), _REF_ROWS // M))
    for s0 in range(0, N, sub):
        sl = slice(s0, min(N, s0 + sub))
        Xc = X[sl]
        m = Xc.shape[0]
        xk = Xc[:, d]                                                                 # [m, M]
        c = torch.where(ab[None], off[None].expand(m, M), xk + off[None])
        valid = (c >= lo[None]) & (c <= hi[None]) & (c != xk) & ((c - xk).abs() <= rad[None])
        Z = Xc[:, None, :].expand(m, M, n).clone()
        Z.scatter_(2, d[None, :, None].expand(m, M, 1), c[:, :, None])
        ce, po, _ = audit(be, q, Z.reshape(-1, n).to(torch.float32), own[sl].repeat_interleave(M), values, pairs)
        cert[sl] = pack_bits((ce.view(m, M) != 0) & valid, W)
        poss[sl] = pack_bits((po.view(m, M) != 0) & valid, W)
    return cert, poss
