"""Certified largest score gap between counterparts, per partition: an optimising branch-and-bound
over the partition's non-PA lattice.

``gap_partitions`` returns, per partition box ``B``, ``gap_lo <= G(B) <= gap_hi`` (definitions:
``ops/gap.py``), an exactly evaluated witness pair whose gap is at least ``gap_lo``, and whether the
search closed (``gap_hi - gap_lo`` is then at most ``tol`` plus two point-bound widths).

Level loop (host, device-resident node pool, the skeleton of ``engine/count.py``): a partition whose
``used + open nodes`` would exceed ``node_budget`` is frozen before the level is bounded -- its open
nodes' parents' bounds (+inf on level 0) go into ``gap_hi`` and ``closed`` is False.  The remaining
nodes get the coupled form bound; each node's candidate corner is bounded rigorously at the point
and may raise the partition's incumbent.  A node with ``ub <= inc_start + tol`` (the incumbent at
the START of the level, so a level's node set does not depend on order) is pruned and its ``ub``
enters ``gap_hi``; an open node of at most ``leaf_points`` points is enumerated (``leaf_hi`` enters
``gap_hi``, ``leaf_lo`` and its argument may raise the incumbent); any other node is halved.

Soundness: every lattice point ends in a pruned node, a leaf or a frozen node, and ``gap_hi`` is the
largest of their upper bounds; ``gap_lo`` is attained by the witness.  The rule looks at one
partition only, incumbents change by strict improvement in pool order (candidates before leaves),
so a partition's numbers do not depend on the partitions sharing the call or on ``slice_nodes``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict

import numpy as np
import torch

from ..ops import count as C
from ..ops import gap as G
from ..ops import rate as R
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from ..utils.timer import NULL, StageTimer
from . import exact
from .search import pa_groups, pa_table

NODE_BUDGET = 65536
LEAF_POINTS = 1024
SLICE_NODES = 32768
TOL = 0.01


@dataclass
class GapResult:
    gap_lo: np.ndarray                    # [P] float64 certified lower bound (attained by the witness)
    gap_hi: np.ndarray                    # [P] float64 certified upper bound
    closed: np.ndarray                    # [P] bool: not frozen by the budget
    nodes: np.ndarray                     # [P] int64 nodes bounded
    x: np.ndarray                         # [P, n] int64 witness
    xp: np.ndarray                        # [P, n] int64 its counterpart
    # totals of the call: levels, leaves, leaf_points, fused_leaves
    stats: Dict[str, int] = field(default_factory=dict)


def exact_gap(mlp, x, xp) -> Fraction:
    return abs(exact.exact_logit_fraction(mlp, x) - exact.exact_logit_fraction(mlp, xp))


def floor_float(fr: Fraction) -> float:
    """The largest float not above ``fr``."""
    f = float(fr)
    return math.nextafter(f, -math.inf) if Fraction(f) > fr else f


def enumerate_leaves(be: Backend, q, llo, lhi, vt, pt, leaf_points: int, stats=None):
    """``(leaf_lo, leaf_hi, arg_s, arg_pair, arg_e)`` of the leaves: the fused kernel when
    ``be.hip``, it is switched on (``FAIRIFY_GAP_FUSED=1``) and it covers the shape, otherwise the
    composed path (materialised points, ``Backend.point_bounds``, torch reduction)."""
    out = None
    if be.hip:
        from ..ops import hip

        if hip.gap_fused():
            out = hip.gap_enum(be, q, llo, lhi, vt, pt, max_vol=leaf_points)
    if stats is not None and out is not None:
        stats["fused_leaves"] = stats.get("fused_leaves", 0) + int(llo.shape[0])
    if out is None:
        # on a GPU about 2^21 rows per point forward; the CPU keeps the reference's small batches
        rows = int(vt.shape[0]) * int(R.offset_vectors(q).shape[0])
        sub = max(16384, (1 << 21) // rows) if be.device.type == "cuda" else 16384
        out = G.enum_gap_ref(be, q, llo, lhi, vt, pt, sub=sub)
    return out


def _raise(inc, wit, p, val, rec):
    """Strict improvements in the given order: ``inc[p[k]] < val[k]`` takes ``rec[k]``."""
    if not p.size:
        return
    order = np.lexsort((np.arange(p.size), -val, p))            # per partition: best value, first index
    first = order[np.concatenate([[True], p[order][1:] != p[order][:-1]])]
    for k in first[val[first] > inc[p[first]]]:
        inc[p[k]] = val[k]
        wit[int(p[k])] = rec(k)


def _level_fused(be, q, nlo, nhi, npart, rx, rp, vt, pt, inc_start, tol, leaf_points, score, tm, stats):
    """The level step of one slice on ``fa_gap_level_kernel`` when ``be.hip``, it is switched on
    (``FAIRIFY_GAP_FUSED=1``) and it covers the shape: ``(NodeBound, codes, children, leaves)`` as
    the reference returns them -- the lists are put back into node order by their keys, so the pool
    does not depend on the order of the kernel's atomics -- or ``None``."""
    if not be.hip:
        return None
    from ..ops import hip

    if not hip.gap_fused():
        return None
    with tm("level"):
        r = hip.gap_level(be, q, nlo, nhi, npart.to(torch.int32), rx, rp, vt, pt, inc_start + float(tol), score,
                          leaf_points)
        if r is None:
            return None
        nk, nl, lost = (int(v) for v in r["counters"].cpu())
        if lost:
            raise RuntimeError("internal: the level's output lists overflowed")
        clo, chi, cpart, _, ckey = (t[:nk] for t in r["kids"])
        ko = torch.argsort(ckey)
        llo, lhi, lpart, lkey = (t[:nl] for t in r["leaves"])
        lo_ = torch.argsort(lkey)
        nb = G.NodeBound(r["ub"], r["pair"].long(), r["orient"].long(), r["c"], r["cand_x"], r["cand_xp"])
    stats["fused_levels"] = stats.get("fused_levels", 0) + 1
    return (nb, r["code"], (clo[ko], chi[ko], cpart[ko].long()), (llo[lo_], lhi[lo_], lpart[lo_].long()))


def _gap_group(be: Backend, q: ResolvedQuery, lo: torch.Tensor, hi: torch.Tensor, values: np.ndarray,
               pairs: np.ndarray, tol: float, node_budget: int, leaf_points: int, slice_nodes: int,
               tm: StageTimer, stats: dict):
    """One PA group: boxes ``lo, hi`` [P, n] on the backend's device."""
    P, n = lo.shape
    dev = be.device
    score = C.split_scores(be.mlp).to(dev)
    vt, pt = torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)
    free = C.free_dims(q)
    inc = np.zeros(P, np.float64)
    top = np.full(P, -math.inf, np.float64)                     # pruned / leaf / frozen upper bounds
    closed = np.ones(P, bool)
    used = np.zeros(P, np.int64)
    wit: Dict[int, tuple] = {}                                  # partition -> (x, x') int64
    plo, phi = lo.to(torch.float32).clone(), hi.to(torch.float32).clone()
    part = torch.arange(P, dtype=torch.int64, device=dev)
    pub = torch.full((P,), math.inf, dtype=torch.float32, device=dev)       # the parents' bounds
    cnt = np.ones(P, np.int64)
    while plo.shape[0]:
        frozen = (cnt > 0) & (used + cnt > node_budget)
        if frozen.any():
            fz = torch.from_numpy(frozen).to(dev)[part]
            np.maximum.at(top, part[fz].cpu().numpy(), pub[fz].double().cpu().numpy())
            closed[frozen] = False
            plo, phi, part, pub = plo[~fz], phi[~fz], part[~fz], pub[~fz]
        used += np.where(frozen, 0, cnt)
        N = plo.shape[0]
        if not N:
            break
        stats["levels"] = stats.get("levels", 0) + 1
        inc_start = torch.from_numpy(inc.copy()).to(dev)
        cands, leaves, nxt = [], [], [[], [], [], []]
        for s0 in range(0, N, slice_nodes):
            sl = slice(s0, min(N, s0 + slice_nodes))
            nlo, nhi, npart = plo[sl], phi[sl], part[sl]
            with tm("bounds"):
                rx, rp = G.node_forms(be, q, nlo, nhi, vt)
            fused = _level_fused(be, q, nlo, nhi, npart, rx, rp, vt, pt, inc_start, tol, leaf_points, score, tm, stats)
            if fused is not None:
                nb, code, kids, lvs = fused
            else:
                with tm("level"):
                    nb = G.node_ub_from(q, nlo, nhi, vt, pt, rx, rp)
                    code, _, kids, lvs = G.level_ref(q, nlo, nhi, npart, nb.ub, nb.c, inc_start, tol, leaf_points,
                                                     score)
            with tm("candidates"):
                lb, ub = be.point_bounds(torch.cat([nb.cand_x, nb.cand_xp]))
                M = nlo.shape[0]
                cval, _ = G.cert_poss(lb[:M], ub[:M], lb[M:], ub[M:])
            pr = code == G.PRUNED
            np.maximum.at(top, npart[pr].cpu().numpy(), nb.ub[pr].double().cpu().numpy())
            cands.append((npart.cpu().numpy(), cval.double().cpu().numpy(), nb.cand_x.cpu().numpy().astype(np.int64),
                          nb.cand_xp.cpu().numpy().astype(np.int64)))
            for dst, t in zip(nxt, kids + (nb.ub[code == G.INNER].repeat_interleave(2),)):
                dst.append(t)
            leaves.append(lvs)
        cp, cv, cx, cxp = (np.concatenate(t) for t in zip(*cands))
        _raise(inc, wit, cp, cv, lambda k: (cx[k], cxp[k]))
        llo, lhi, lpart = (torch.cat(t) for t in zip(*leaves))
        if llo.shape[0]:
            with tm("enum"):
                l_lo, l_hi, a_s, a_p, a_e = enumerate_leaves(be, q, llo, lhi, vt, pt, leaf_points, stats)
            if bool((a_s < 0).any()):
                raise RuntimeError("internal: a leaf over the enumeration limit or without a pair reached the kernel")
            lp = lpart.cpu().numpy()
            stats["leaves"] = stats.get("leaves", 0) + int(lp.size)
            stats["leaf_points"] = stats.get("leaf_points", 0) + int(C.volumes(llo, lhi, free).sum())
            np.maximum.at(top, lp, l_hi.double().cpu().numpy())
            lx, lxp = G.witness_rows(q, llo.cpu().numpy(), lhi.cpu().numpy(), values, pairs, a_s.cpu().numpy(),
                                     a_p.cpu().numpy(), a_e.cpu().numpy())
            _raise(inc, wit, lp, l_lo.double().cpu().numpy(), lambda k: (lx[k], lxp[k]))
        plo, phi, part, pub = (torch.cat(t) for t in nxt)
        cnt = np.bincount(part.cpu().numpy(), minlength=P).astype(np.int64)
    return inc, top, closed, used, wit


def gap_partitions(be: Backend, q: ResolvedQuery, lo: torch.Tensor, hi: torch.Tensor, pids: torch.Tensor,
                   tol: float = TOL, node_budget: int = NODE_BUDGET, leaf_points: int = LEAF_POINTS,
                   slice_nodes: int = SLICE_NODES, timer: StageTimer = NULL) -> GapResult:
    """Certified score-gap brackets of ``P`` partition boxes ``lo, hi`` [P, n] (integral).

    With ``be.hip`` and ``FAIRIFY_GAP_FUSED=1`` the level step (``fa_gap_level_kernel``) and the
    leaf enumeration (``fa_gap_enum_kernel``) run on the kernels of csrc/gap.hip, each where it
    covers the shape; otherwise, and for a declined shape, the torch reference of ``ops/gap.py``
    runs on the backend's device.  The node rows' forms and the candidates' point bounds come from
    ``Backend.bounds`` / ``Backend.point_bounds`` on either path.  The witness is confirmed exactly
    on the host.  Raises ``ValueError`` for a negative ``tol``, more than 32 RA offset vectors or ``leaf_points`` over 65 536."""
    P, n = lo.shape
    tol, node_budget, leaf_points, slice_nodes = float(tol), int(node_budget), int(leaf_points), int(slice_nodes)
    if node_budget < 1 or slice_nodes < 1:
        raise ValueError("gap: node_budget and slice_nodes must be positive")
    if not 1 <= leaf_points <= C.MAX_LEAF_POINTS:
        raise ValueError(f"gap: leaf_points {leaf_points} outside 1..{C.MAX_LEAF_POINTS}")
    if not tol >= 0:
        raise ValueError("gap: tol must be non-negative")
    offs = R.offset_vectors(q)                # the E limit holds on every path
    lo_np = lo.detach().cpu().numpy().astype(np.int64)
    hi_np = hi.detach().cpu().numpy().astype(np.int64)
    res = GapResult(np.zeros(P), np.zeros(P), np.ones(P, bool), np.zeros(P, np.int64), lo_np.copy(), lo_np.copy())
    dev = be.device
    for rows in pa_groups(q, lo_np, hi_np):
        if rows.size == 0:
            continue
        values, pairs = pa_table(q, lo_np[rows], hi_np[rows])
        if pairs.shape[0] == 0:
            continue                          # no pair: G = 0, the witness is the box's corner twice
        sel = torch.from_numpy(rows).to(lo.device)
        inc, top, closed, used, wit = _gap_group(be, q, lo[sel].to(dev), hi[sel].to(dev), values, pairs, tol,
                                                 node_budget, leaf_points, slice_nodes, timer, res.stats)
        zero = int(np.nonzero((offs == 0).all(axis=1))[0][0])
        for k, r in enumerate(rows):
            if k in wit:
                x, xp = wit[k]
            else:                             # the incumbent never rose above 0: any pair serves
                x, xp = G.witness_rows(q, lo_np[r][None], hi_np[r][None], values, pairs, [0], [0], [zero])
                x, xp = x[0], xp[0]
            g = max(float(inc[k]), floor_float(exact_gap(be.mlp, x, xp)))
            res.x[r], res.xp[r] = x, xp
            res.gap_lo[r], res.gap_hi[r] = g, max(float(top[k]), g)
            res.closed[r], res.nodes[r] = closed[k], used[k]
    return res
