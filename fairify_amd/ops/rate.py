"""Discrimination-rate counts: the profile / counterpart rows and their rigorous classification.

For a partition box, its id, a resolved query, the box's PA assignments ``values`` [V, npa] and
the ordered all-differ pairs ``pairs`` [Pp, 2]:

* profile ``s``: the lattice point ``ref.sample_points(lo, hi, pids, S, seed)[p, s]`` (the
  simulation stage's stream); its ``x`` rows are the point with the PA coordinates overwritten by
  each ``values[v]``;
* counterpart rows ``x'``: the ``x`` rows (PA-only query), or the ``x`` rows with the RA coordinates
  shifted by EVERY offset vector ``e`` in ``{-tau..tau}^nra`` (row-major over ``q.ra_idx``, not
  clipped to the box, as in ``spec.py``) -- the measured event is "a counterpart exists";
* with ``[l, u]`` the rigorous logit bounds of a row (``Backend.point_bounds``), a profile is
  *certain* if some pair ``(v, v')`` and offset ``e`` have ``u_x(v) < 0 < l_x'(v', e)`` or
  ``l_x(v) > 0 > u_x'(v', e)``, *possible* with ``l_x(v) < 0 < u_x'(v', e)`` or
  ``u_x(v) > 0 > l_x'(v', e)``, and *ambiguous* if possible but not certain.

``certain => exact flip => possible``: the exact logit lies in ``[l, u]``.  This module is the
reference (any backend); the fused kernel is ``ops/hip.py:rate_counts`` (csrc/rate.hip).
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

from . import reference as ref

MAX_OFFSETS = 32      # launch-shape limit of csrc/rate.hip (FA_RATE_MAX_E)
AMB_SLOTS = 32        # ambiguous sample indices recorded per partition by the kernel (FA_RATE_SLOTS)


def offset_vectors(q) -> np.ndarray:
    """RA offset vectors [E, nra] (int64), row-major over ``q.ra_idx``; [1, 0] for a PA-only query.
    More than ``MAX_OFFSETS`` vectors raise ``ValueError``."""
    if not q.relaxed:
        return np.zeros((1, 0), dtype=np.int64)
    E = (2 * q.tau + 1) ** len(q.ra_idx)
    if E > MAX_OFFSETS:
        raise ValueError(f"rate: {E} RA offset vectors ((2*{q.tau}+1)^{len(q.ra_idx)}) exceed the launch-shape "
                         f"limit of {MAX_OFFSETS} of this first version")
    rng = range(-q.tau, q.tau + 1)
    return np.array(list(itertools.product(*[rng] * len(q.ra_idx))), dtype=np.int64).reshape(E, len(q.ra_idx))


def profile_rows(q, X: torch.Tensor, values: torch.Tensor):
    """Profiles ``X`` [N, n] -> (x rows [N, V, n], counterpart rows [N, E, V, n]); for a PA-only
    query the counterpart rows are the x rows (E = 1, a view)."""
    N, n = X.shape
    V = values.shape[0]
    pa = torch.tensor(list(q.pa_idx), device=X.device, dtype=torch.long)
    XV = X[:, None, :].expand(N, V, n).clone()
    XV[:, :, pa] = values.to(X.dtype)[None].expand(N, V, -1)
    if not q.relaxed:
        return XV, XV[:, None]
    off = torch.from_numpy(offset_vectors(q)).to(X.device, X.dtype)                 # [E, nra]
    ra = torch.tensor(list(q.ra_idx), device=X.device, dtype=torch.long)
    XP = XV[:, None].expand(N, off.shape[0], V, n).clone()
    XP[:, :, :, ra] = XP[:, :, :, ra] + off[None, :, None, :]
    return XV, XP


def classify(lx, ux, lxp, uxp, pairs: torch.Tensor):
    """(certain, possible) [N] from x bounds [N, V], counterpart bounds [N, E, V] and ``pairs``."""
    vi, vj = pairs[:, 0], pairs[:, 1]
    li, ui = lx[:, None, vi], ux[:, None, vi]                                        # [N, 1, Pp]
    lj, uj = lxp[:, :, vj], uxp[:, :, vj]                                            # [N, E, Pp]
    cert = ((ui < 0) & (lj > 0)) | ((li > 0) & (uj < 0))
    poss = ((li < 0) & (uj > 0)) | ((ui > 0) & (lj < 0))
    return cert.flatten(1).any(dim=1), poss.flatten(1).any(dim=1)


def rate_flags_ref(be, q, X: torch.Tensor, values: torch.Tensor, pairs: torch.Tensor):
    """(certain, possible) bool [N] of profiles ``X`` [N, n] with ``be.point_bounds``."""
    N, n = X.shape
    V = values.shape[0]
    XV, XP = profile_rows(q, X.to(torch.float32), values)
    lx, ux = be.point_bounds(XV.reshape(-1, n))
    lx, ux = lx.view(N, V), ux.view(N, V)
    if q.relaxed:
        lxp, uxp = be.point_bounds(XP.reshape(-1, n))
        lxp, uxp = lxp.view(N, -1, V), uxp.view(N, -1, V)
    else:
        lxp, uxp = lx[:, None], ux[:, None]
    return classify(lx, ux, lxp, uxp, pairs)


def rate_counts_ref(be, q, lo: torch.Tensor, hi: torch.Tensor, pids: torch.Tensor, n_samples: int, seed: int,
                    values: torch.Tensor, pairs: torch.Tensor, sub: int = 256):
    """Reference counts of ``P`` partitions: (certain profiles [P] int32, ambiguous profiles [P]
    int32, ambiguous mask [P, S] bool)."""
    offset_vectors(q)                     # the E limit holds on every path
    P, n = lo.shape
    dev = lo.device
    flips = torch.zeros(P, dtype=torch.int32, device=dev)
    amb = torch.zeros(P, dtype=torch.int32, device=dev)
    mask = torch.zeros(P, n_samples, dtype=torch.bool, device=dev)
    if not P or not n_samples:
        return flips, amb, mask
    for s0 in range(0, P, sub):
        sl = slice(s0, min(P, s0 + sub))
        X = ref.sample_points(lo[sl], hi[sl], pids[sl], n_samples, seed)             # [p, S, n]
        cert, poss = rate_flags_ref(be, q, X.reshape(-1, n), values, pairs)
        cert = cert.view(-1, n_samples)
        a = poss.view(-1, n_samples) & ~cert
        flips[sl] = cert.sum(dim=1).to(torch.int32)
        amb[sl] = a.sum(dim=1).to(torch.int32)
        mask[sl] = a
    return flips, amb, mask
