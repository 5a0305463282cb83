"""Certified discrimination counts: a branch-and-bound over a partition's non-PA lattice that
counts instead of searching.

``count_partitions`` returns, per partition box, four int64 values ``fair, unfair, open, nodes``
with ``fair + unfair + open == w`` (``w``: the box's non-PA lattice points): ``unfair / w`` is a
certified lower bound of the partition's discrimination rate, ``(unfair + open) / w`` a certified
upper bound, and the rate is exact when ``open == 0``.  Definitions (box test, split, enumeration):
``ops/count.py``.

Level loop (host, device-resident node pool): a partition whose ``used + open nodes`` would exceed
``node_budget`` is frozen before the level is bounded -- its open nodes' volumes go to ``open`` and
leave the pool.  The remaining nodes are box-tested (sound logit intervals of the node rows); FAIR /
UNFAIR nodes add their volume, OPEN nodes of at most ``leaf_points`` points are enumerated point by
point with the rigorous point bounds (ambiguous points decided exactly on the host, the rate
command's 32-slot overflow rule per leaf), the other OPEN nodes are halved.  The rule looks at one
partition only and every bound is a function of its own row, so a partition's integers do not depend
on the partitions sharing the call, on ``slice_nodes`` or on how leaves are spread over workgroups.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..ops import count as C
from ..ops import rate as R
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from ..utils.timer import NULL, StageTimer
from .search import pa_groups, pa_table
from .rate import exact_flags

NODE_BUDGET = 65536
LEAF_POINTS = 1024
SLICE_NODES = 32768
_WITNESS_CHUNK = 4096


@dataclass
class CountResult:
    fair: np.ndarray                      # [P] int64 lattice points certified fair
    unfair: np.ndarray                    # [P] int64 certified unfair
    open: np.ndarray                      # [P] int64 undecided (frozen by the budget)
    nodes: np.ndarray                     # [P] int64 nodes box-tested
    # row -> (lo, hi) int64 [n]: a box known to contain an unfair point (``witness_for`` rows only)
    witness: Dict[int, Tuple[np.ndarray, np.ndarray]] = field(default_factory=dict)
    # totals of the call: levels, leaves, leaf_points, ambiguous_points, overflowed_leaves, host_points
    stats: Dict[str, int] = field(default_factory=dict)


def box_weights(q: ResolvedQuery, lo: np.ndarray, hi: np.ndarray):
    """Non-PA lattice points of each box as Python ints."""
    free = C.free_dims(q)
    return [int(np.prod((hi[k, free] - lo[k, free] + 1).astype(object))) if free else 1 for k in range(lo.shape[0])]


def _points(lo: np.ndarray, hi: np.ndarray, free, idx: np.ndarray) -> np.ndarray:
    X = C.lattice_points_at(torch.from_numpy(lo[None]), torch.from_numpy(hi[None]), free,
                            torch.from_numpy(np.asarray(idx, np.int64))[None])
    return X[0].numpy().astype(np.int64)


def witness_pair(mlp, q: ResolvedQuery, lo: np.ndarray, hi: np.ndarray):
    """One exactly confirmed flipping pair (x, x') inside a witness box of :class:`CountResult`
    (an UNFAIR node flips at its first point, a leaf is enumerated), or None."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    values, pairs = pa_table(q, lo[None], hi[None])
    free = C.free_dims(q)
    vol = box_weights(q, lo[None], hi[None])[0]
    for s0 in range(0, vol, _WITNESS_CHUNK):
        X = _points(lo, hi, free, np.arange(s0, min(vol, s0 + _WITNESS_CHUNK)))
        flags, x, xp = exact_flags(mlp, q, X, values, pairs, return_pairs=True)
        hit = np.nonzero(flags)[0]
        if hit.size:
            return x[hit[0]], xp[hit[0]]
    return None


_EXACT_CHUNK = 1 << 20


def _resolve(be, q, llo, lhi, vt, pt, leaf: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """Exact unfair points among the points ``idx`` [M] of the leaves ``leaf`` [M] (indices into
    ``llo, lhi``), counted per leaf: int64 [L].  One vectorised decode, ``_EXACT_CHUNK`` points per
    exact pass."""
    free = C.free_dims(q)
    lo_np, hi_np = llo.cpu().numpy().astype(np.int64), lhi.cpu().numpy().astype(np.int64)
    values, pairs = vt.cpu().numpy(), pt.cpu().numpy()
    out = np.zeros(lo_np.shape[0], np.int64)
    for c0 in range(0, leaf.size, _EXACT_CHUNK):
        lf, rest = leaf[c0:c0 + _EXACT_CHUNK], idx[c0:c0 + _EXACT_CHUNK].astype(np.int64)
        X = lo_np[lf]
        for d in reversed(free):                        # ops/count.lattice_points_at, per point
            w = hi_np[lf, d] - lo_np[lf, d] + 1
            X[:, d] += rest % w
            rest = rest // w
        out += np.bincount(lf, weights=exact_flags(be.mlp, q, X, values, pairs), minlength=out.size).astype(np.int64)
    return out


def _enumerate(be, q, llo, lhi, vt, pt, leaf_points, tm: StageTimer = NULL, stats: Optional[dict] = None):
    """Exact unfair points of the leaves ``llo, lhi`` [L, n] and their volumes: int64 [L] each (host)."""
    L = llo.shape[0]
    free = C.free_dims(q)
    if be.hip:
        from ..ops import hip

        with tm("enum"):
            cert, amb, idx = hip.count_enum(be, q, llo, lhi, vt, pt, max_vol=leaf_points)
        with tm("enum_host"):
            vol = C.volumes(llo, lhi, free).cpu().numpy()
            cert, amb = cert.cpu().numpy().astype(np.int64), amb.cpu().numpy().astype(np.int64)
            if (cert < 0).any():
                raise RuntimeError("internal: a leaf over the enumeration limit reached the kernel")
            full = amb > R.AMB_SLOTS
            rows = np.nonzero((amb > 0) & ~full)[0]     # only these leaves' index rows cross to the host
            idx = idx[torch.from_numpy(rows).to(idx.device)].cpu().numpy()
            rec = np.arange(R.AMB_SLOTS)[None, :] < amb[rows][:, None]
            leaf, pts = np.repeat(rows, amb[rows]), idx[rec]
    else:
        with tm("enum"):
            vol = C.volumes(llo, lhi, free).cpu().numpy()
            cert, amb, masks = C.enum_counts_ref(be, q, llo, lhi, vt, pt)
            cert, amb = cert.cpu().numpy().astype(np.int64), amb.cpu().numpy().astype(np.int64)
            full = np.zeros(L, bool)
            rows = np.nonzero(amb)[0]
            leaf = np.repeat(rows, amb[rows])
            pts = np.concatenate([np.nonzero(masks[k].cpu().numpy())[0] for k in rows] + [np.zeros(0, np.int64)])
    unfair = cert.copy()
    with tm("enum_host"):
        if leaf.size:
            unfair += _resolve(be, q, llo, lhi, vt, pt, leaf, pts)
        # an overflowed leaf is decided in full: every point of it, the certain ones included; leaves
        # are taken in groups of about _EXACT_CHUNK points
        fr = np.nonzero(full)[0]
        while fr.size:
            g = max(1, int(np.searchsorted(np.cumsum(vol[fr]), _EXACT_CHUNK, side="right")))
            sel, fr = fr[:g], fr[g:]
            start = np.cumsum(vol[sel]) - vol[sel]
            every = np.arange(int(vol[sel].sum())) - np.repeat(start, vol[sel])
            unfair[sel] = _resolve(be, q, llo, lhi, vt, pt, np.repeat(sel, vol[sel]), every)[sel]
    if stats is not None:
        for key, v in (("leaves", L), ("leaf_points", int(vol.sum())), ("ambiguous_points", int(amb.sum())),
                       ("overflowed_leaves", int(full.sum())), ("host_points", int(leaf.size + vol[full].sum()))):
            stats[key] = stats.get(key, 0) + v
    return unfair, vol


def _count_group(be: Backend, q: ResolvedQuery, lo: torch.Tensor, hi: torch.Tensor, values: np.ndarray,
                 pairs: np.ndarray, node_budget: int, leaf_points: int, slice_nodes: int, want: np.ndarray,
                 tm: StageTimer = NULL, stats: Optional[dict] = None):
    """One PA group: boxes ``lo, hi`` [P, n] on the backend's device."""
    P, n = lo.shape
    dev = be.device
    free = C.free_dims(q)
    score = C.split_scores(be.mlp).to(dev)
    vt, pt = torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)
    vf = vt.to(torch.float32)
    V = values.shape[0]
    fold = tuple(q.pa_idx)
    fair = torch.zeros(P, dtype=torch.int64, device=dev)
    unfair = torch.zeros(P, dtype=torch.int64, device=dev)
    open_ = torch.zeros(P, dtype=torch.int64, device=dev)
    leaf_unfair = np.zeros(P, np.int64)
    leaf_fair = np.zeros(P, np.int64)
    used = np.zeros(P, np.int64)
    want_t = torch.from_numpy(want).to(dev)
    witness: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
    plo, phi = lo.to(torch.float32).clone(), hi.to(torch.float32).clone()
    part = torch.arange(P, dtype=torch.int32, device=dev)
    cnt = np.ones(P, np.int64)

    def bounds(rl, rh):
        with tm("bounds"):
            r = be.bounds(rl, rh, mode="symbolic", crown=True, fold=fold)
        return r.out_lb.view(-1, V), r.out_ub.view(-1, V)

    while plo.shape[0]:
        # budget rule, per partition: a partition that cannot bound all its open nodes is frozen
        frozen = (cnt > 0) & (used + cnt > node_budget)
        if frozen.any():
            fz = torch.from_numpy(frozen).to(dev)[part.long()]
            open_.index_add_(0, part[fz].long(), C.volumes(plo[fz], phi[fz], free))
            plo, phi, part = plo[~fz], phi[~fz], part[~fz]
        used += np.where(frozen, 0, cnt)
        N = plo.shape[0]
        if not N:
            break
        if stats is not None:
            stats["levels"] = stats.get("levels", 0) + 1
        child_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
        level = []
        for s0 in range(0, N, slice_nodes):
            sl = slice(s0, min(N, s0 + slice_nodes))
            nlo, nhi, npart = plo[sl], phi[sl], part[sl]
            if be.hip:
                from ..ops import hip

                with tm("rows"):
                    rlo, rhi, clo_, chi_ = hip.count_rows(be, q, nlo, nhi, vf)
                lx, ux = bounds(rlo, rhi)
                lxp, uxp = bounds(clo_, chi_) if q.relaxed else (lx, ux)
                with tm("level"):
                    code, kids, leaves, counters = hip.count_level(be, q, nlo, nhi, npart, lx, ux, lxp, uxp, pt,
                                                                   score, leaf_points, fair, unfair, child_cnt,
                                                                   part_checked=True)
            else:
                with tm("rows"):
                    rlo, rhi, clo_, chi_ = C.node_rows(q, nlo, nhi, vt)
                lx, ux = bounds(rlo, rhi)
                lxp, uxp = bounds(clo_, chi_) if q.relaxed else (lx, ux)
                code = C.box_codes_ref(lx, ux, lxp, uxp, pt)
                vol = C.volumes(nlo, nhi, free)
                pl = npart.long()
                fair.index_add_(0, pl[code == C.FAIR], vol[code == C.FAIR])
                unfair.index_add_(0, pl[code == C.UNFAIR], vol[code == C.UNFAIR])
                leaf = (code == C.OPEN) & (vol <= leaf_points)
                inner = (code == C.OPEN) & ~leaf
                _, klo, khi = C.split_ref(nlo[inner], nhi[inner], free, score)
                kpart = npart[inner].repeat_interleave(2)
                child_cnt += torch.bincount(kpart.long(), minlength=P).to(torch.int32)
                kids, leaves = (klo, khi, kpart), (nlo[leaf], nhi[leaf], npart[leaf])
                counters = torch.tensor([klo.shape[0], int(leaf.sum()), 0], dtype=torch.int32)
            level.append((nlo, nhi, npart, code, kids, leaves, counters))
        # the level's one read-back: list lengths and the children per partition
        tally = torch.cat([c.to(dev) for *_, c in level] + [child_cnt]).cpu().numpy().astype(np.int64)
        cnt = tally[3 * len(level):]
        nxt = [[], [], []]
        for i, (nlo, nhi, npart, code, kids, leaves, _) in enumerate(level):
            nk, nl, lost = tally[3 * i:3 * i + 3]
            if lost:
                raise RuntimeError("internal: the level's output lists overflowed")
            for dst, t in zip(nxt, kids):
                dst.append(t[:nk])
            if nl:
                llo, lhi, lpart = (t[:nl] for t in leaves)
                lu, lvol = _enumerate(be, q, llo, lhi, vt, pt, leaf_points, tm, stats)
                lp = lpart.cpu().numpy().astype(np.int64)
                np.add.at(leaf_unfair, lp, lu)
                np.add.at(leaf_fair, lp, lvol - lu)
                for k in np.nonzero((lu > 0) & want[lp])[0]:
                    if int(lp[k]) not in witness:
                        witness[int(lp[k])] = (llo[k].cpu().numpy().astype(np.int64), lhi[k].cpu().numpy().astype(np.int64))
            if want.any():
                hit = torch.nonzero((code == C.UNFAIR) & want_t[npart.long()]).flatten()
                for k in hit.tolist():
                    p = int(npart[k])
                    if p not in witness:
                        witness[p] = (nlo[k].cpu().numpy().astype(np.int64), nhi[k].cpu().numpy().astype(np.int64))
        plo, phi, part = torch.cat(nxt[0]), torch.cat(nxt[1]), torch.cat(nxt[2])
    return (fair.cpu().numpy() + leaf_fair, unfair.cpu().numpy() + leaf_unfair, open_.cpu().numpy(), used, witness)


def count_partitions(be: Backend, q: ResolvedQuery, lo: torch.Tensor, hi: torch.Tensor, pids: torch.Tensor,
                     node_budget: int = NODE_BUDGET, leaf_points: int = LEAF_POINTS, slice_nodes: int = SLICE_NODES,
                     witness_for: Optional[np.ndarray] = None, timer: StageTimer = NULL) -> CountResult:
    """Certified counts of ``P`` partition boxes ``lo, hi`` [P, n] (integral) with ids ``pids``.

    ``be.hip`` selects the kernels (csrc/count.hip), otherwise the reference runs.  A level larger
    than ``slice_nodes`` runs in slices.  ``witness_for``: bool [P]; a masked partition that gains
    unfair volume gets a box containing an unfair point in ``witness`` (:func:`witness_pair` turns it
    into an exactly confirmed pair).  ``timer``: stage times (rows / bounds / level / enum / enum_host; profiling
    runs pass a synchronising one).  Raises ``ValueError`` for a box of 2^62 or more non-PA points,
    more than 32 RA offset vectors or ``leaf_points`` over 65 536."""
    P = lo.shape[0]
    node_budget, leaf_points, slice_nodes = int(node_budget), int(leaf_points), int(slice_nodes)
    if node_budget < 1 or slice_nodes < 1:
        raise ValueError("count: node_budget and slice_nodes must be positive")
    if not 1 <= leaf_points <= C.MAX_LEAF_POINTS:
        raise ValueError(f"count: leaf_points {leaf_points} outside 1..{C.MAX_LEAF_POINTS}")
    R.offset_vectors(q)                   # the E limit holds on every path
    lo_np = lo.detach().cpu().numpy().astype(np.int64)
    hi_np = hi.detach().cpu().numpy().astype(np.int64)
    weights = box_weights(q, lo_np, hi_np)
    if any(w >= 2 ** 62 for w in weights):
        raise ValueError("count: a partition of 2^62 or more non-PA lattice points is not counted")
    want = np.zeros(P, bool) if witness_for is None else np.asarray(witness_for, bool).reshape(P)
    res = CountResult(*(np.zeros(P, np.int64) for _ in range(4)))
    dev = be.device
    for rows in pa_groups(q, lo_np, hi_np):
        if rows.size == 0:
            continue
        values, pairs = pa_table(q, lo_np[rows], hi_np[rows])
        sel = torch.from_numpy(rows).to(lo.device)
        f, u, o, nodes, wit = _count_group(be, q, lo[sel].to(dev), hi[sel].to(dev), values, pairs, node_budget,
                                           leaf_points, slice_nodes, want[rows], timer, res.stats)
        res.fair[rows], res.unfair[rows], res.open[rows], res.nodes[rows] = f, u, o, nodes
        for k, box in wit.items():
            res.witness[int(rows[k])] = box
    for k, w in enumerate(weights):
        if int(res.fair[k]) + int(res.unfair[k]) + int(res.open[k]) != w:
            raise RuntimeError(f"internal: counts of partition {int(pids[k])} do not add up to its weight {w}")
    return res
