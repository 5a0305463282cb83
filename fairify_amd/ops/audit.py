"""Audit of real individuals: the PA-domain table, a row's own index and the rigorous per-row masks.

For a resolved query ``q`` and integral rows ``X`` [N, n] (docs/DESIGN.md 5f):

* the PA table covers the whole PA *domain*: ``values = q.pa_values(domain lo, domain hi)`` [V, npa]
  and ``pairs = q.pa_pairs(values)``, the ordered all-differ pairs;
* ``own[i]`` is the index of row i's PA coordinates in ``values``, -1 when they lie outside the PA
  domain (the row is not audited: all outputs 0);
* the counterparts of row i: for every ``v'`` with ``(own[i], v')`` in ``pairs`` and every RA offset
  vector ``e`` (``ops/rate.offset_vectors``: unclipped, row-major over ``q.ra_idx``; one zero-length
  vector for a PA-only query), the row with PA := ``values[v']`` and RA += ``e``;
* with ``[l, u]`` the rigorous logit bounds (``Backend.point_bounds``) of the own row and
  ``[l', u']`` of a counterpart, bit ``v'`` of ``cert`` is set when some ``e`` has ``u < 0 < l'`` or
  ``l > 0 > u'``, bit ``v'`` of ``poss`` when some ``e`` has ``l < 0 < u'`` or ``u > 0 > l'``, and
  ``own_sign`` is -1 if ``u < 0``, +1 if ``l > 0``, else 0.

``cert <= exact flip <= poss`` per bit: the exact logit lies in ``[l, u]``.  This module is the
reference on any backend -- on a CUDA backend it is the composed device path, built from the
existing point kernel; the fused kernel is ``ops/hip.py:audit_masks`` (csrc/audit.hip).
"""
from __future__ import annotations

import numpy as np
import torch

from .rate import MAX_OFFSETS, offset_vectors, profile_rows

MAX_VALUES = 32       # bits of a mask; launch-shape limit of csrc/audit.hip (FA_RATE_MAX_V)
_REF_ROWS = 1 << 18   # counterpart rows per chunk of the reference


def pa_domain_table(q):
    """(values [V, npa], pairs [Pp, 2]) int64 of the whole PA domain.  More than 32 PA assignments
    or RA offset vectors raise ``ValueError``."""
    values = q.pa_values(q.domain.lo(), q.domain.hi())
    V = values.shape[0]
    if V > MAX_VALUES:
        raise ValueError(f"audit: {V} PA assignments exceed the launch-shape limit of {MAX_VALUES} of this first "
                         f"version")
    offset_vectors(q)                     # the E limit holds on every path
    return values, q.pa_pairs(values)


def integral_rows(X) -> np.ndarray:
    """Rows [N, n] as int64; a non-integral (or non-finite) entry raises ``ValueError``."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"audit: expected rows [N, n], got shape {X.shape}")
    if np.issubdtype(X.dtype, np.integer):
        return X.astype(np.int64)
    Xf = X.astype(np.float64)
    bad = ~(np.isfinite(Xf) & (Xf == np.rint(Xf)))
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise ValueError(f"audit: row {int(r)} column {int(c)} holds {Xf[r, c]!r}: rows must be encoded integers")
    return np.rint(Xf).astype(np.int64)


def own_index(q, X: np.ndarray, values: np.ndarray) -> np.ndarray:
    """Index [N] (int32) of each row's PA coordinates in ``values``; -1 outside the PA domain."""
    X = np.asarray(X, dtype=np.int64)
    eq = np.all(X[:, None, list(q.pa_idx)] == values[None], axis=2)                  # [N, V]
    return np.where(eq.any(axis=1), eq.argmax(axis=1), -1).astype(np.int32)


def _bit_weights(V: int, dev) -> torch.Tensor:
    """int32 bit patterns 1 << v (bit 31 as the sign bit)."""
    w = [(1 << v) - (1 << 32 if v == 31 else 0) for v in range(V)]
    return torch.tensor(w, dtype=torch.int32, device=dev)


def audit_masks_ref(be, q, X: torch.Tensor, own: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor,
                    sub: int = 4096):
    """Reference masks of rows ``X`` [N, n]: (cert int32 [N], poss int32 [N], own_sign int8 [N]) on
    ``X``'s device, in chunks of at most ``sub`` rows: ``ops/rate.profile_rows``, ``be.point_bounds``,
    then the mask arithmetic."""
    E = int(offset_vectors(q).shape[0])
    N, n = X.shape
    V = int(values.shape[0])
    if V > MAX_VALUES:
        raise ValueError(f"audit: {V} PA assignments exceed the launch-shape limit of {MAX_VALUES} of this first "
                         f"version")
    assert E <= MAX_OFFSETS
    dev = X.device
    X = X.to(torch.float32)
    own = own.to(dev, torch.long)
    cert = torch.zeros(N, dtype=torch.int32, device=dev)
    poss = torch.zeros(N, dtype=torch.int32, device=dev)
    sign = torch.zeros(N, dtype=torch.int8, device=dev)
    if not N:
        return cert, poss, sign
    table = torch.zeros(V, V, dtype=torch.bool, device=dev)
    if pairs.shape[0]:
        table[pairs[:, 0].to(dev), pairs[:, 1].to(dev)] = True
    bits = _bit_weights(V, dev)
    values = values.to(dev)
    sub = max(1, min(int(sub), _REF_ROWS // (E * V)))
    for s0 in range(0, N, sub):
        sl = slice(s0, min(N, s0 + sub))
        Xc, oc = X[sl], own[sl]
        m = Xc.shape[0]
        _, XP = profile_rows(q, Xc, values)                                           # [m, E, V, n]
        l, u = be.point_bounds(Xc)
        lp, up = be.point_bounds(XP.reshape(-1, n))
        lp, up = lp.view(m, E, V), up.view(m, E, V)
        l, u = l.view(m, 1, 1), u.view(m, 1, 1)
        ok = table[oc.clamp(min=0)] & (oc >= 0)[:, None]                              # [m, V]
        c = ((((u < 0) & (lp > 0)) | ((l > 0) & (up < 0))).any(dim=1)) & ok
        p = ((((l < 0) & (up > 0)) | ((u > 0) & (lp < 0))).any(dim=1)) & ok
        cert[sl] = (c.to(torch.int32) * bits).sum(dim=1, dtype=torch.int32)
        poss[sl] = (p.to(torch.int32) * bits).sum(dim=1, dtype=torch.int32)
        s = (l.view(m) > 0).to(torch.int8) - (u.view(m) < 0).to(torch.int8)
        sign[sl] = torch.where(oc >= 0, s, torch.zeros_like(s))
    return cert, poss, sign
