"""Audit of real individuals: rigorous per-row masks on the device, exact resolution of what fp32
cannot decide on the host.

``audit_rows`` decides, for every row of a table of individuals and every other PA assignment ``v'``
of the PA domain, whether some counterpart (``ops/audit.py``) flips the sign of the logit strictly.
The rigorous point bounds settle almost every bit (``cert``: certain flips, ``~poss``: certain
non-flips); the ambiguous bits ``poss & ~cert`` are decided with ``exact.exact_signs`` in one
vectorised pass, so ``flip_mask`` is a function of (network, query, row) only -- the same integers on
every backend, in every batch, at every row position and launch shape.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from ..ops import audit as A
from ..ops import rate as R
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from . import exact


@dataclass
class AuditResult:
    own: np.ndarray                       # [N] int32   index into the PA-domain table, -1: not audited
    cert: np.ndarray                      # [N] uint32  bit v': certain flip (rigorous fp32 bounds)
    poss: np.ndarray                      # [N] uint32  bit v': possible flip
    flip_mask: np.ndarray                 # [N] uint32  exact flip bits (with resolve), else cert
    direction: np.ndarray                 # [N] int8    exact sign of a flagged row's own logit, else 0
    ambiguous_bits: np.ndarray            # [N] uint32  bits left undecided (all 0 with resolve)
    own_sign: np.ndarray                  # [N] int8    rigorous sign of the own logit (0: undecided)
    fused: bool = False                   # the masks came from the fused kernel


def counterparts(q: ResolvedQuery, X: np.ndarray, vp: np.ndarray, values: np.ndarray) -> np.ndarray:
    """Rows ``X`` [M, n] with PA := ``values[vp[m]]`` and RA += every offset vector: [M, E, n] int64."""
    X = np.asarray(X, dtype=np.int64)
    off = R.offset_vectors(q)
    XP = np.repeat(X[:, None, :], off.shape[0], axis=1)
    XP[:, :, list(q.pa_idx)] = values[np.asarray(vp, dtype=np.int64)][:, None, :]
    if q.relaxed:
        XP[:, :, list(q.ra_idx)] += off[None]
    return XP


def _bit_list(mask: np.ndarray, V: int) -> Tuple[np.ndarray, np.ndarray]:
    """(row, bit) of every set bit of the uint32 masks."""
    set_ = (mask[:, None] >> np.arange(V, dtype=np.uint32)[None]) & np.uint32(1)
    return np.nonzero(set_)


def device_masks(be: Backend, q: ResolvedQuery, X: np.ndarray, own: np.ndarray, values: np.ndarray,
                 pairs: np.ndarray):
    """(cert, poss uint32 [N], own_sign int8 [N], fused): the fused kernel when ``be.hip`` and it
    covers the shape, otherwise the reference / composed path."""
    dev = be.device
    Xt = torch.from_numpy(X).to(dev, torch.float32)
    ot = torch.from_numpy(own).to(dev)
    vt, pt = torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)
    out = None
    if be.hip:
        from ..ops import hip

        out = hip.audit_masks(be, q, Xt, ot, vt, pt)
    fused = out is not None
    if out is None:
        out = A.audit_masks_ref(be, q, Xt, ot, vt, pt)
    cert, poss, sign = (t.cpu().numpy() for t in out)
    return cert.view(np.uint32), poss.view(np.uint32), sign, fused


def audit_rows(be: Backend, q: ResolvedQuery, X, resolve: bool = True) -> AuditResult:
    """Audit rows ``X`` [N, n] (integral; a non-integral row raises ``ValueError``).  With ``resolve``
    the ambiguous bits of all rows are decided exactly in one vectorised pass and ``flip_mask`` is
    exact; without, ``flip_mask = cert`` and the exact mask lies between ``cert`` and ``poss``."""
    X = A.integral_rows(X)
    if X.shape[1] != q.n:
        raise ValueError(f"audit: rows have {X.shape[1]} columns, the domain {q.n}")
    values, pairs = A.pa_domain_table(q)
    V = values.shape[0]
    own = A.own_index(q, X, values)
    cert, poss, sign, fused = device_masks(be, q, X, own, values, pairs)
    amb = poss & ~cert
    flip = cert.copy()
    direction = np.where(cert != 0, sign, 0).astype(np.int8)      # a set cert bit: the rigorous sign is exact
    if resolve and amb.any():
        rows, bits = _bit_list(amb, V)                             # K ambiguous (row, v') bits
        uniq, inv = np.unique(rows, return_inverse=True)
        s_own = exact.exact_signs(be.mlp, X[uniq])                 # [U]
        XP = counterparts(q, X[rows], bits, values)                # [K, E, n]
        s_cp = exact.exact_signs(be.mlp, XP.reshape(-1, X.shape[1])).reshape(len(rows), -1)
        hit = (s_own[inv.reshape(-1)][:, None] * s_cp < 0).any(axis=1)
        np.bitwise_or.at(flip, rows[hit], np.uint32(1) << bits[hit].astype(np.uint32))
        direction[uniq] = np.where(flip[uniq] != 0, s_own, 0).astype(np.int8)
        amb = np.zeros_like(amb)
    return AuditResult(own=own, cert=cert, poss=poss, flip_mask=flip, direction=direction, ambiguous_bits=amb,
                       own_sign=sign, fused=fused)


def witnesses(mlp, q: ResolvedQuery, X: np.ndarray, v_prime: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """For rows ``X`` [M, n] and one set bit ``v_prime[m]`` each: the exactly confirmed pairs
    (x, x') [M, n], x' the counterpart of the first flipping offset vector in offset order.  A row
    whose bit does not flip raises ``ValueError``."""
    X = A.integral_rows(X)
    values, _ = A.pa_domain_table(q)
    M, n = X.shape
    if M == 0:
        return X, X.copy()
    XP = counterparts(q, X, v_prime, values)                      # [M, E, n]
    s_own = exact.exact_signs(mlp, X)
    s_cp = exact.exact_signs(mlp, XP.reshape(-1, n)).reshape(M, -1)
    flip = s_own[:, None] * s_cp < 0
    if not flip.any(axis=1).all():
        m = int(np.nonzero(~flip.any(axis=1))[0][0])
        raise ValueError(f"audit: row {X[m].tolist()} has no flipping counterpart at PA value "
                         f"{values[int(v_prime[m])].tolist()}")
    return X, XP[np.arange(M), flip.argmax(axis=1)]


def witness(mlp, q: ResolvedQuery, x, v_prime: int) -> Tuple[np.ndarray, np.ndarray]:
    """An exactly confirmed pair (x, x') for a set bit ``v_prime`` of row ``x``: the first offset
    vector in offset order that flips."""
    X, XP = witnesses(mlp, q, np.asarray(x)[None], np.array([int(v_prime)]))
    return X[0], XP[0]


def lowest_bit(mask: np.ndarray) -> np.ndarray:
    """Index of the lowest set bit of non-zero uint32 masks."""
    m = mask.astype(np.int64)
    return np.round(np.log2((m & -m).astype(np.float64))).astype(np.int64)
