"""Host layer shared by the three Python BaB front ends (engine/bab.py, relu_bab.py, beta_bab.py): the
verdict codes and the result record, the PA grouping, the per-call verdict arrays, the exact confirmation
of candidate pairs, the per-PA-group scatter, the two-orientation solve of a relaxed query, and the small
box operations their torch loops repeat.  What differs between the solvers stays a parameter: the
confirmation order and ``exact_models``, the scatter's ``open_left``, the partitions handed to the final
sweep; the second solver of a relaxed solve is built by the caller.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from ..models.mlp import MLP
from ..spec import ResolvedQuery
from . import exact

UNKNOWN, SAT, UNSAT, RUNNING = 0, 1, 2, 3
VERDICT_NAMES = {UNKNOWN: "unknown", SAT: "sat", UNSAT: "unsat", RUNNING: "running"}


@dataclass
class BaBResult:
    status: np.ndarray               # [P] int8 verdicts
    cex_x: np.ndarray                # [P, n0] int64 (valid where SAT)
    cex_xp: np.ndarray
    nodes: np.ndarray                # [P] int64 nodes expanded
    iters: int = 0
    time: float = 0.0
    open_left: Optional[np.ndarray] = None   # [P] open nodes left when an UNKNOWN partition stopped
                                             # (native runtime; the escalation filter's predictor)


def pa_groups(q: ResolvedQuery, lo: np.ndarray, hi: np.ndarray) -> List[np.ndarray]:
    """Row indices of the partitions sharing one protected-attribute range (one group when the
    chunk's PA ranges are identical, e.g. a PA that the partition size does not split)."""
    pa = list(q.pa_idx)
    if len(lo) == 0 or (np.all(lo[:, pa] == lo[:1, pa]) and np.all(hi[:, pa] == hi[:1, pa])):
        return [np.arange(len(lo))]
    key = np.concatenate([lo[:, pa], hi[:, pa]], axis=1)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return [np.nonzero(inv == g)[0] for g in range(int(inv.max()) + 1)]


def pa_table(q: ResolvedQuery, lo: np.ndarray, hi: np.ndarray):
    """PA assignments shared by all partitions of one PA group (:func:`pa_groups`)."""
    pa = list(q.pa_idx)
    assert np.all(lo[:, pa] == lo[:1, pa]) and np.all(hi[:, pa] == hi[:1, pa]), \
        "internal: one PA table per group (callers split with pa_groups)"
    values = q.pa_values(lo[0], hi[0])
    return values, q.pa_pairs(values)


class Verdicts:
    """What one solve call fills: ``status`` [P] int8 (a copy of ``init_status``, or all RUNNING), the
    SAT witnesses ``cex_x`` / ``cex_xp`` [P, n] and the ``nodes`` expanded [P]."""

    def __init__(self, P: int, n: int, init_status: Optional[np.ndarray] = None):
        self.status = np.full(P, RUNNING, dtype=np.int8) if init_status is None else init_status.astype(np.int8).copy()
        self.cex_x, self.cex_xp = np.zeros((P, n), dtype=np.int64), np.zeros((P, n), dtype=np.int64)
        self.nodes = np.zeros(P, dtype=np.int64)

    def close_running(self, code: int) -> "Verdicts":
        """Every RUNNING partition becomes ``code`` (the early returns)."""
        self.status[self.status == RUNNING] = code
        return self

    def sweep(self, left: Sequence[int]) -> "Verdicts":
        """End of a level loop: a RUNNING partition is UNKNOWN if it has nodes left (``left``: the
        partitions of the nodes a time-out left in the pool) and UNSAT otherwise."""
        run = self.status == RUNNING
        has = np.isin(np.arange(len(run)), np.asarray(left, dtype=np.int64))
        self.status[run] = np.where(has[run], UNKNOWN, UNSAT)
        return self

    def result(self, t0: Optional[float] = None, iters: int = 0, open_left: Optional[np.ndarray] = None) -> BaBResult:
        return BaBResult(self.status, self.cex_x, self.cex_xp, self.nodes, iters,
                         0.0 if t0 is None else time.time() - t0, open_left=open_left)


def confirm_pairs(v: Verdicts, q: ResolvedQuery, lo_np, hi_np, mlp_exact: MLP, parts: np.ndarray, xa: torch.Tensor,
                  xb: torch.Tensor, exact_models=None, lex_order: bool = True) -> List[int]:
    """Candidate pairs (row k: partition ``parts[k]``) rounded to the lattice and checked exactly: the pair
    constraints in the partition's box and a violation of ``mlp_exact`` (of ``exact_models[partition]``, one
    row at a time, where masked networks are given).  A partition not yet SAT takes its first confirmed pair:
    first in (partition, X, XP) lexicographic order (``lex_order``; relu, beta: the witness does not depend
    on the node order) or in the order given (the input-split loop).  Returns the new SAT partitions."""
    X, XP = (t.cpu().numpy().round().astype(np.int64) for t in (xa, xb))
    ok = exact.check_pair_constraints(X, XP, lo_np[parts], hi_np[parts], q.pa_idx, q.ra_idx, q.tau)
    if exact_models is None:
        viol = exact.is_violation(mlp_exact, X, XP) & ok
    else:
        viol = np.zeros(len(parts), dtype=bool)
        for k in np.nonzero(ok)[0]:
            viol[k] = exact.is_violation(exact_models[parts[k]], X[k:k + 1], XP[k:k + 1])[0]
    order = np.arange(len(parts))
    if lex_order:
        order = np.lexsort(tuple(np.concatenate([X, XP], axis=1).T[::-1]) + (parts,))
    newly = []
    for k in order[viol[order]]:
        p = parts[k]
        if v.status[p] != SAT:
            v.status[p] = SAT
            v.cex_x[p], v.cex_xp[p] = X[k], XP[k]
            newly.append(p)
    return newly


def solve_pa_groups(groups: List[np.ndarray], lo_np, hi_np, init_status: Optional[np.ndarray], time_budget: float,
                    t0: float, solve_group: Callable[[np.ndarray, np.ndarray, float], BaBResult],
                    open_left: bool = False) -> BaBResult:
    """One solve per PA group (each has its own PA table), scattered back in input order:
    ``solve_group(rows, status[rows], seconds left of time_budget)`` returns the group's result; ``iters``
    are summed; ``open_left``: frontier sizes, zeros where a group reports none (else ``None``)."""
    v = Verdicts(*lo_np.shape, init_status)
    iters, ol = 0, (np.zeros(len(lo_np), dtype=np.int64) if open_left else None)
    for g in groups:
        left = max(0.0, time_budget - (time.time() - t0))
        r = solve_group(g, v.status[g], left)
        v.status[g], v.cex_x[g], v.cex_xp[g], v.nodes[g] = r.status, r.cex_x, r.cex_xp, r.nodes
        if ol is not None and r.open_left is not None:
            ol[g] = r.open_left
        iters += r.iters
    return v.result(t0, iters, ol)


def merge_orientations(r1: BaBResult, status: np.ndarray, second: Callable[[np.ndarray], BaBResult],
                       t0: float) -> BaBResult:
    """Second orientation of a relaxed query: ``second(init_status)`` solves, on the negated network, the
    partitions the first solve ``r1`` closed (RUNNING in ``status`` before it; the others UNKNOWN).  UNSAT
    only where the second closed too, its witness where it found a pair, nodes summed."""
    closed = (r1.status == UNSAT) & (status == RUNNING)
    if not closed.any():
        return r1
    r2 = second(np.where(closed, RUNNING, UNKNOWN).astype(np.int8))
    out = r1.status.copy()
    out[closed] = r2.status[closed]
    cx, cxp = r1.cex_x.copy(), r1.cex_xp.copy()
    s2 = closed & (r2.status == SAT)
    cx[s2], cxp[s2] = r2.cex_x[s2], r2.cex_xp[s2]
    return BaBResult(out, cx, cxp, r1.nodes + r2.nodes, 0, time.time() - t0)


def clamp_tau(xp_r: torch.Tensor, x_r: torch.Tensor, tau: float) -> torch.Tensor:
    """x'_r pulled into [x_r - tau, x_r + tau] (the RA columns of a candidate pair)."""
    return torch.minimum(torch.maximum(xp_r, x_r - tau), x_r + tau)


def tau_apart(lo_r, hi_r, plo_r, phi_r, tau: float) -> torch.Tensor:
    """Nodes whose x_r and x'_r boxes are more than tau apart on some RA dim: no admissible pair."""
    return ((plo_r > hi_r + tau) | (phi_r < lo_r - tau)).any(dim=1)


def pool_overflow(part: torch.Tensor, max_pool: int, status) -> int:
    """A pool keeping its oldest ``max_pool`` nodes: the partitions losing nodes, where RUNNING in ``status``
    (host array or device tensor), become UNKNOWN.  Returns how many; the caller cuts its tensors."""
    lost = torch.unique(part[max_pool:])
    if isinstance(status, np.ndarray):
        lost = lost.cpu().numpy()
    lost = lost[status[lost] == RUNNING]
    status[lost] = UNKNOWN
    return len(lost)


def halve(lo: torch.Tensor, hi: torch.Tensor, rows: torch.Tensor, dims: torch.Tensor):
    """The boxes twice, dim ``dims[k]`` of row ``rows[k]`` cut at its floor midpoint: lo, hi of the lower
    children [lo, mid], then of the upper children [mid + 1, hi]."""
    lo1, hi1, lo2, hi2 = lo.clone(), hi.clone(), lo.clone(), hi.clone()
    mid = torch.floor((lo[rows, dims] + hi[rows, dims]) / 2)
    hi1[rows, dims] = mid
    lo2[rows, dims] = mid + 1
    return lo1, hi1, lo2, hi2
