"""Per-partition discrimination counts: rigorous classification on the device, exact resolution
of what fp32 cannot decide on the host.

``measure_partitions`` counts, per partition, the sampled profiles (``ops/rate.py``) that have a
strictly flipping counterpart.  The rigorous point bounds settle almost every profile (*certain*
flips and certain non-flips); the few *ambiguous* ones are regenerated from the hash stream and
decided with ``exact.exact_signs``, so the resolved count ``flips_exact`` is a function of
(network, box, partition id, seed, sample count) only -- the same integer on every path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ..ops import rate as R
from ..ops import reference as ref
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from . import exact
from .search import pa_groups, pa_table


@dataclass
class RateResult:
    flips: np.ndarray                     # [P] int64  certain flips (rigorous fp32 bounds)
    ambiguous_left: np.ndarray            # [P] int64  ambiguous profiles not decided (0 with resolve)
    flips_exact: Optional[np.ndarray]     # [P] int64  exact flip count (None without resolve)


def exact_rows(q: ResolvedQuery, X: np.ndarray, values: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Integer profiles ``X`` [N, n] -> (x rows [N, V, n], counterpart rows [N, E, V, n]) int64."""
    X = np.asarray(X, dtype=np.int64)
    N, n = X.shape
    V = values.shape[0]
    XV = np.repeat(X[:, None, :], V, axis=1)
    XV[:, :, list(q.pa_idx)] = values[None]
    if not q.relaxed:
        return XV, XV[:, None]
    off = R.offset_vectors(q)
    XP = np.repeat(XV[:, None], off.shape[0], axis=1)
    XP[:, :, :, list(q.ra_idx)] += off[None, :, None, :]
    return XV, XP


def exact_flags(mlp, q: ResolvedQuery, X: np.ndarray, values: np.ndarray, pairs: np.ndarray,
                return_pairs: bool = False):
    """Exact strict-sign flip (spec.py) of integer profiles ``X`` [N, n]: bool [N]; with
    ``return_pairs`` also one flipping pair (x, x') [N, n] each (rows of non-flipping profiles are
    unspecified)."""
    X = np.asarray(X, dtype=np.int64)
    N, n = X.shape
    V = values.shape[0]
    if N == 0 or pairs.shape[0] == 0:
        z = np.zeros((N, n), np.int64)
        return (np.zeros(N, bool), z, z) if return_pairs else np.zeros(N, bool)
    XV, XP = exact_rows(q, X, values)
    sx = exact.exact_signs(mlp, XV.reshape(-1, n)).reshape(N, V)
    sxp = sx[:, None] if not q.relaxed else exact.exact_signs(mlp, XP.reshape(-1, n)).reshape(N, -1, V)
    flip = sx[:, None, pairs[:, 0]] * sxp[:, :, pairs[:, 1]] < 0                   # [N, E, Pp]
    flags = flip.reshape(N, -1).any(axis=1)
    if not return_pairs:
        return flags
    first = flip.reshape(N, -1).argmax(axis=1)
    e, k = first // pairs.shape[0], first % pairs.shape[0]
    ar = np.arange(N)
    return flags, XV[ar, pairs[k, 0]], XP[ar, e, pairs[k, 1]]


def _profiles(lo_np, hi_np, pid: int, idx: np.ndarray, seed: int) -> np.ndarray:
    X = ref.sample_points_at(torch.from_numpy(lo_np[None]), torch.from_numpy(hi_np[None]),
                             torch.tensor([int(pid)]), torch.from_numpy(np.asarray(idx, np.int64))[None], seed)
    return X[0].numpy().astype(np.int64)


def first_exact_pair(mlp, q: ResolvedQuery, lo_np: np.ndarray, hi_np: np.ndarray, pid: int, n_samples: int,
                     seed: int):
    """One exactly confirmed flipping pair (x, x') among the sampled profiles of a partition, or None."""
    values, pairs = pa_table(q, lo_np[None], hi_np[None])
    X = _profiles(lo_np, hi_np, pid, np.arange(n_samples), seed)
    flags, x, xp = exact_flags(mlp, q, X, values, pairs, return_pairs=True)
    hit = np.nonzero(flags)[0]
    return (x[hit[0]], xp[hit[0]]) if hit.size else None


def measure_partitions(be: Backend, q: ResolvedQuery, lo: torch.Tensor, hi: torch.Tensor, pids: torch.Tensor,
                       n_samples: int, seed: int, resolve: bool = True) -> RateResult:
    """Discrimination counts of ``P`` partition boxes ``lo, hi`` [P, n] (integral) with ids ``pids``.

    The device (``be.hip``: the fused kernel, otherwise the reference) returns the certain flips
    and the ambiguous profiles; with ``resolve`` the host decides the ambiguous ones exactly -- all
    ``n_samples`` profiles of a partition whose ambiguous indices overflowed the kernel's 32 slots
    -- and ``flips_exact`` is the exact count.  Without, the count lies in
    ``[flips, flips + ambiguous_left]``."""
    P = lo.shape[0]
    S = int(n_samples)
    lo_np = lo.detach().cpu().numpy().astype(np.int64)
    hi_np = hi.detach().cpu().numpy().astype(np.int64)
    pid_np = pids.detach().cpu().numpy().astype(np.int64)
    dev = be.device
    flips = np.zeros(P, np.int64)
    left = np.zeros(P, np.int64)
    fexact = np.zeros(P, np.int64) if resolve else None
    for rows in pa_groups(q, lo_np, hi_np):
        if rows.size == 0:
            continue
        values, pairs = pa_table(q, lo_np[rows], hi_np[rows])
        sel = torch.from_numpy(rows).to(lo.device)
        lo_g, hi_g, pid_g = lo[sel].to(dev), hi[sel].to(dev), pids[sel].to(dev)
        vt, pt = torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)
        if be.hip:
            from ..ops import hip

            f, a, idx = hip.rate_counts(be, q, lo_g, hi_g, pid_g, S, seed, vt, pt)
            f, a, idx = f.cpu().numpy().astype(np.int64), a.cpu().numpy().astype(np.int64), idx.cpu().numpy()
            full = a > R.AMB_SLOTS
            todo = [np.arange(S) if full[k] else idx[k, :a[k]] for k in range(rows.size)]
        else:
            f, a, mask = R.rate_counts_ref(be, q, lo_g, hi_g, pid_g, S, seed, vt, pt)
            f, a, mask = f.cpu().numpy().astype(np.int64), a.cpu().numpy().astype(np.int64), mask.cpu().numpy()
            full = np.zeros(rows.size, bool)
            todo = [np.nonzero(mask[k])[0] for k in range(rows.size)]
        flips[rows] = f
        if not resolve:
            left[rows] = a
            continue
        for k in np.nonzero(a)[0]:
            r = rows[k]
            n_exact = int(exact_flags(be.mlp, q, _profiles(lo_np[r], hi_np[r], pid_np[r], todo[k], seed),
                                      values, pairs).sum())
            # an overflowed partition was decided in full; otherwise the certain flips stand
            fexact[r] = n_exact if full[k] else f[k] + n_exact
        rest = rows[a == 0]
        fexact[rest] = flips[rest]
    return RateResult(flips=flips, ambiguous_left=left, flips_exact=fexact)
