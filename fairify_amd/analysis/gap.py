"""``gap`` command: the certified largest score gap between counterparts, per partition.

The verifier and the rate commands ask about the sign of the logit; this module reports how far the
logits of two individuals who differ only in the protected attributes (and by at most ``tau`` in the
relaxed ones) can lie apart inside a partition: ``gap_lo <= G(B) <= gap_hi`` in units of the logit
(``engine/gap.py``, definitions in ``ops/gap.py``), with an exactly evaluated witness pair that
attains at least ``gap_lo``.  Since the sigmoid's slope is at most 1/4, ``min(1, gap_hi / 4)`` bounds
the gap of the probabilities.

``gap.csv`` has one row per partition, ``gap.json`` the domain-wide maxima, the arg-max partition's
witness with exact logits and probabilities, and -- with the verdicts of a verify run -- the same
maxima per verdict class: the UNSAT line is the largest certified score gap where no decision
flips.  A witness inside an UNSAT partition whose exact signs are strictly opposite contradicts the
prover and raises :class:`~fairify_amd.analysis.rate.SoundnessError`.
"""
from __future__ import annotations

import csv
import json
import math
import os
from typing import Dict, Optional

import numpy as np
import torch

from .. import presets
from ..engine import exact
from ..engine.gap import LEAF_POINTS, NODE_BUDGET, TOL, gap_partitions
from ..models.zoo import get_model
from ..ops.backend import Backend
from ..partition import processing_order
from .hybrid import NOT_ATTEMPTED, V_UNSAT, VerdictTable
from .rate import _NAMES, CHUNK, POOL_NODES, SoundnessError

GAP_HEADER = ["index", "grid_id", "verdict", "gap_lo", "gap_hi", "closed", "nodes", "x", "xp", "sign_x", "sign_xp"]


def _row(v) -> str:
    return " ".join(str(int(t)) for t in v)


def _sigmoid(z: float) -> float:
    return 1.0 / (1.0 + math.exp(-z)) if z >= 0 else math.exp(z) / (1.0 + math.exp(z))


def gap_grid(grid, q, be: Backend, order: np.ndarray, table: Optional[VerdictTable] = None, tol: float = TOL,
             node_budget: int = NODE_BUDGET, leaf_points: int = LEAF_POINTS):
    """Bracket the partitions ``order`` (grid ids) of ``grid`` in chunks whose pools stay below
    ``POOL_NODES`` nodes (a partition's row does not depend on its chunk).  Returns the per-partition
    arrays ``verdict, gap_lo, gap_hi, closed, nodes, x, xp, sign_x, sign_xp`` and the call's stats."""
    n = len(order)
    verdict = np.full(n, NOT_ATTEMPTED, dtype=np.int8) if table is None else table.table[order]
    lo_, hi_ = np.zeros(n), np.zeros(n)
    closed, nodes = np.ones(n, bool), np.zeros(n, np.int64)
    xs, xps = np.zeros((n, q.n), np.int64), np.zeros((n, q.n), np.int64)
    stats: Dict[str, int] = {}
    chunk = max(1, min(CHUNK, POOL_NODES // max(1, int(node_budget))))
    for c0 in range(0, n, chunk):
        ids = order[c0:c0 + chunk]
        lo_np, hi_np = grid.decode(ids)
        pids = torch.from_numpy(ids).to(be.device)
        lo_t = torch.from_numpy(lo_np).to(be.device, torch.float32)
        hi_t = torch.from_numpy(hi_np).to(be.device, torch.float32)
        r = gap_partitions(be, q, lo_t, hi_t, pids, tol, node_budget, leaf_points)
        sl = slice(c0, c0 + len(ids))
        lo_[sl], hi_[sl], closed[sl], nodes[sl], xs[sl], xps[sl] = r.gap_lo, r.gap_hi, r.closed, r.nodes, r.x, r.xp
        for k, v in r.stats.items():
            stats[k] = stats.get(k, 0) + int(v)
    sx, sxp = exact.exact_signs(be.mlp, xs), exact.exact_signs(be.mlp, xps)
    bad = np.nonzero((verdict == V_UNSAT) & (sx * sxp < 0))[0]
    if bad.size:
        k = int(bad[0])
        raise SoundnessError(int(order[k]), xs[k], xps[k])
    return verdict, lo_, hi_, closed, nodes, xs, xps, sx, sxp, stats


def _maxima(lo_, hi_, sel) -> Dict:
    idx = np.nonzero(sel)[0]
    if not idx.size:
        return {"partitions": 0, "gap_lo": 0.0, "gap_hi": 0.0, "argmax_index": None}
    return {"partitions": int(idx.size), "gap_lo": float(lo_[idx].max()), "gap_hi": float(hi_[idx].max()),
            "argmax_index": int(idx[np.argmax(lo_[idx])]) + 1}


def gap_preset(preset: str, model: str, results: Optional[str] = None, tol: float = TOL, node_budget: int = NODE_BUDGET,
               leaf_points: int = LEAF_POINTS, max_partitions: Optional[int] = None, seed: int = 0,
               weights: str = "zoo", device: str = "cpu", out_dir: Optional[str] = None) -> Dict:
    """Bracket ``model`` on the grid of ``preset`` in the seeded processing order (the first
    ``max_partitions`` of it); ``results``: the directory of a verify run (``<model>.csv``).  Writes
    ``gap.csv`` / ``gap.json`` to ``out_dir`` and returns the summary."""
    pre = presets.get(preset)
    grid = pre.grid(seed=seed)
    q = pre.resolved()
    mlp = get_model(model, weights=weights, seed=seed)
    be = Backend(mlp, device=device)
    order = processing_order(grid, seed=seed)
    if max_partitions is not None:
        order = order[:max_partitions]
    table = None
    if results:
        table = VerdictTable.from_csv(grid, os.path.join(results, f"{model}.csv"), seed=seed)
    verdict, lo_, hi_, closed, nodes, xs, xps, sx, sxp, stats = gap_grid(grid, q, be, order, table, tol, node_budget,
                                                                          leaf_points)
    out = {"preset": preset, "model": model, "seed": int(seed), "tol": float(tol), "node_budget": int(node_budget),
           "leaf_points": int(leaf_points), "partitions": int(len(order))}
    top = _maxima(lo_, hi_, np.ones(len(order), bool))
    out.update(gap_lo=top["gap_lo"], gap_hi=top["gap_hi"], argmax_index=top["argmax_index"])
    if top["argmax_index"] is not None:
        k = top["argmax_index"] - 1
        zx = float(exact.exact_logit_fraction(mlp, xs[k]))
        zxp = float(exact.exact_logit_fraction(mlp, xps[k]))
        out["witness"] = {"grid_id": int(order[k]), "x": xs[k].tolist(), "xp": xps[k].tolist(), "logit_x": zx,
                          "logit_xp": zxp, "prob_x": _sigmoid(zx), "prob_xp": _sigmoid(zxp),
                          "prob_gap": abs(_sigmoid(zx) - _sigmoid(zxp))}
    out["prob_gap_upper"] = min(1.0, out["gap_hi"] / 4.0)
    out["closed_partitions"] = int(closed.sum())
    out["frozen_partitions"] = int((~closed).sum())
    out["nodes"] = int(nodes.sum())
    out["leaf_points_enumerated"] = int(stats.get("leaf_points", 0))
    out["fused"] = bool(stats.get("fused_leaves", 0) or stats.get("fused_levels", 0))
    if table is not None:
        out["by_verdict"] = {name: _maxima(lo_, hi_, verdict == code) for code, name in _NAMES.items()}
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "gap.csv"), "w", newline="") as fp:
            wr = csv.writer(fp)
            wr.writerow(GAP_HEADER)
            for k in range(len(order)):
                wr.writerow([k + 1, int(order[k]), _NAMES[int(verdict[k])], repr(float(lo_[k])), repr(float(hi_[k])),
                             int(closed[k]), int(nodes[k]), _row(xs[k]), _row(xps[k]), int(sx[k]), int(sxp[k])])
        with open(os.path.join(out_dir, "gap.json"), "w") as fp:
            json.dump(out, fp, indent=2)
    return out
