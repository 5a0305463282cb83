"""``measure`` command: per-partition discrimination rates and a stratified domain-wide estimate.

The verifier answers SAT / UNSAT / UNKNOWN per partition; this module measures *how much*: the
share of a partition's individuals (profiles: lattice points with every PA assignment) that have
a strictly flipping counterpart, from ``n_samples`` profiles per partition drawn with the
simulation stage's hash stream and classified rigorously (``engine/rate.py``).  The partitions
are strata of the domain, weighted by their number of non-PA lattice points

    w_i = prod_{d not in PA} (hi_d - lo_d + 1),

which gives

* ``rate = sum_i w_i p_i / sum_i w_i`` with ``p_i = flips_i / S``;
* ``stderr = sqrt(sum_i w_i^2 p_i (1 - p_i) / S) / sum_i w_i`` and the normal interval at ``conf``;
* with the verdicts of a verify run: an UNSAT partition has rate exactly 0 and is not sampled, so
  the variance comes from the other strata only, and ``certified_upper = sum_{i not UNSAT} w_i /
  sum_i w_i`` bounds the domain-wide rate with certainty (1.0 without verdicts).

With ``check_unsat`` the UNSAT partitions are sampled too: an exact flip inside one contradicts
the prover and raises :class:`SoundnessError` with the confirmed pair.

With ``certify`` every partition that is sampled is also *counted* by the branch-and-bound of
``engine/count.py``: ``bounds.csv`` carries its ``fair / unfair / open`` volumes, and
``certified_lower = sum unfair / W`` and ``certified_upper = sum (unfair + open) / W`` (an UNSAT
partition of the verify run contributes ``fair = w`` uncounted) bound the domain-wide rate with
certainty from both sides.
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
from ..engine.count import LEAF_POINTS, NODE_BUDGET, count_partitions, witness_pair
from ..engine.rate import first_exact_pair, measure_partitions
from ..models.zoo import get_model
from ..ops.backend import Backend
from ..partition import processing_order
from .causal import _z
from .hybrid import NOT_ATTEMPTED, V_SAT, V_UNKNOWN, V_UNSAT, VerdictTable

CHUNK = 8192
POOL_NODES = 1 << 24     # certify: partitions per chunk x node_budget (256 partitions at the default budget)
_NAMES = {V_SAT: "sat", V_UNSAT: "unsat", V_UNKNOWN: "unknown", NOT_ATTEMPTED: "not_attempted"}
CSV_HEADER = ["Partition_ID", "grid_id", "verdict", "samples", "flips", "rate"]
BOUNDS_HEADER = ["Partition_ID", "grid_id", "verdict", "weight", "fair", "unfair", "open", "nodes", "lower", "upper"]


class SoundnessError(RuntimeError):
    """A sampled profile of an UNSAT partition flips exactly: the prover's verdict is wrong."""

    def __init__(self, grid_id: int, x: np.ndarray, xp: np.ndarray):
        self.grid_id = int(grid_id)
        self.x = np.asarray(x, dtype=np.int64)
        self.xp = np.asarray(xp, dtype=np.int64)
        super().__init__(f"partition with grid id {self.grid_id} is UNSAT in the verify results, but the pair "
                         f"x={self.x.tolist()} x'={self.xp.tolist()} violates the query exactly")


def stratum_weights(q, lo: np.ndarray, hi: np.ndarray):
    """Non-PA lattice points of each box as Python ints (exact at any domain size)."""
    free = [d for d in range(lo.shape[1]) if d not in q.pa_idx]
    width = (hi[:, free] - lo[:, free] + 1).astype(np.int64)
    if float(np.prod(width.max(axis=0).astype(np.float64))) < 2.0 ** 62:
        return [int(v) for v in np.prod(width, axis=1)]
    return [int(v) for v in np.prod(width.astype(object), axis=1)]


def summarize(weights, flips, samples, verdicts, conf: float = 0.95) -> Dict:
    """Stratified estimate from per-partition weights (ints), exact flip counts, sample counts
    (0: not sampled, rate 0) and verdict codes."""
    W = sum(weights)
    num = 0.0
    var = 0.0
    open_w = 0
    for w, f, s, v in zip(weights, flips, samples, verdicts):
        if v != V_UNSAT:
            open_w += w
        if s:
            p = f / s
            num += float(w) * p
            var += float(w) ** 2 * p * (1.0 - p) / s
    rate = num / float(W) if W else 0.0
    stderr = math.sqrt(var) / float(W) if W else 0.0
    half = _z(0.5 + conf / 2.0) * stderr
    counts = {name: int(sum(1 for v in verdicts if v == code)) for code, name in _NAMES.items()}
    return {"rate": rate, "stderr": stderr, "conf": conf, "ci_low": max(0.0, rate - half),
            "ci_high": min(1.0, rate + half), "certified_upper": (open_w / W) if W else 1.0,
            "partitions": len(weights), "sampled": int(sum(1 for s in samples if s)), "verdicts": counts}


def measure_grid(grid, q, be: Backend, order: np.ndarray, table: Optional[VerdictTable] = None,
                 n_samples: int = 1000, seed: int = 0, check_unsat: bool = False, conf: float = 0.95,
                 resolve: bool = True):
    """Measure the partitions ``order`` (grid ids) of ``grid``, 8 192 per chunk.  Returns the
    summary and the per-partition arrays (verdict codes, samples, flips)."""
    n = len(order)
    verdict = np.full(n, NOT_ATTEMPTED, dtype=np.int8) if table is None else table.table[order]
    flips = np.zeros(n, np.int64)
    samples = np.zeros(n, np.int64)
    left = 0
    wts = []
    for c0 in range(0, n, CHUNK):
        ids = order[c0:c0 + CHUNK]
        lo_np, hi_np = grid.decode(ids)
        wts += stratum_weights(q, lo_np, hi_np)
        v = verdict[c0:c0 + CHUNK]
        take = np.nonzero((v != V_UNSAT) | check_unsat)[0]
        if take.size == 0:
            continue
        pids = torch.from_numpy(ids[take]).to(be.device)
        if be.hip:
            from ..ops import hip

            lo_t, hi_t = hip.decode(grid, pids)
        else:
            lo_t = torch.from_numpy(lo_np[take]).to(be.device, torch.float32)
            hi_t = torch.from_numpy(hi_np[take]).to(be.device, torch.float32)
        r = measure_partitions(be, q, lo_t, hi_t, pids, n_samples, seed, resolve=resolve)
        got = r.flips_exact if resolve else r.flips
        left += int(r.ambiguous_left.sum())
        if check_unsat and resolve:
            bad = take[(v[take] == V_UNSAT) & (got > 0)]
            if bad.size:
                k = int(bad[0])
                x, xp = first_exact_pair(be.mlp, q, lo_np[k], hi_np[k], int(ids[k]), n_samples, seed)
                raise SoundnessError(int(ids[k]), x, xp)
        flips[c0 + take] = got
        samples[c0 + take] = n_samples
    out = summarize(wts, flips.tolist(), samples.tolist(), verdict.tolist(), conf)
    out["flips"] = int(flips.sum())
    out["ambiguous_left"] = left
    out["check_unsat"] = bool(check_unsat)
    return out, verdict, samples, flips


def certify_grid(grid, q, be: Backend, order: np.ndarray, table: Optional[VerdictTable] = None,
                 node_budget: int = NODE_BUDGET, leaf_points: int = LEAF_POINTS, check_unsat: bool = False):
    """Count the partitions ``order`` (grid ids) of ``grid`` that :func:`measure_grid` samples, in
    chunks whose pools stay below ``POOL_NODES`` nodes (a partition's counts do not depend on its
    chunk).  Returns the certified summary keys and the ``bounds.csv`` rows (without the
    header).  An UNSAT partition is not counted (``fair = w``) unless ``check_unsat``; then unfair
    volume inside one raises :class:`SoundnessError` with an exactly confirmed pair.  A SAT partition
    that counts ``unfair == 0`` and ``open == 0`` contradicts the verify run's confirmed pair and
    raises ``RuntimeError``."""
    n = len(order)
    verdict = np.full(n, NOT_ATTEMPTED, dtype=np.int8) if table is None else table.table[order]
    rows = []
    chunk = max(1, min(CHUNK, POOL_NODES // max(1, int(node_budget))))
    for c0 in range(0, n, chunk):
        ids = order[c0:c0 + chunk]
        lo_np, hi_np = grid.decode(ids)
        wts = stratum_weights(q, lo_np, hi_np)
        v = verdict[c0:c0 + chunk]
        four = np.zeros((len(ids), 4), dtype=object)
        four[:, 0] = wts
        take = np.nonzero((v != V_UNSAT) | check_unsat)[0]
        if take.size:
            pids = torch.from_numpy(ids[take]).to(be.device)
            lo_t = torch.from_numpy(lo_np[take]).to(be.device, torch.float32)
            hi_t = torch.from_numpy(hi_np[take]).to(be.device, torch.float32)
            r = count_partitions(be, q, lo_t, hi_t, pids, node_budget, leaf_points, witness_for=v[take] == V_UNSAT)
            for j, k in enumerate(take):
                four[k] = [int(r.fair[j]), int(r.unfair[j]), int(r.open[j]), int(r.nodes[j])]
                if v[k] == V_UNSAT and r.unfair[j] > 0:
                    x, xp = witness_pair(be.mlp, q, *r.witness[j])
                    raise SoundnessError(int(ids[k]), x, xp)
                if v[k] == V_SAT and r.unfair[j] == 0 and r.open[j] == 0:
                    raise RuntimeError(f"partition with grid id {int(ids[k])} is SAT in the verify results, but "
                                       f"every one of its {wts[k]} profiles counts as fair")
        for k in range(len(ids)):
            f, u, o, nodes = four[k]
            rows.append([c0 + k + 1, int(ids[k]), _NAMES[int(v[k])], wts[k], f, u, o, nodes,
                         repr(u / wts[k]), repr((u + o) / wts[k])])
    W = sum(r[3] for r in rows)
    unfair, open_ = sum(r[5] for r in rows), sum(r[6] for r in rows)
    out = {"certified_lower": (unfair / W) if W else 0.0, "certified_upper": ((unfair + open_) / W) if W else 1.0,
           "certified_exact": open_ == 0, "count_nodes": sum(r[7] for r in rows)}
    return out, rows


def measure_preset(preset: str, model: str, results: Optional[str] = None, n_samples: int = 1000, seed: int = 0,
                   max_partitions: Optional[int] = None, check_unsat: bool = False, weights: str = "zoo",
                   device: str = "cpu", out_dir: Optional[str] = None, conf: float = 0.95,
                   resolve: bool = True, certify: bool = False, node_budget: int = NODE_BUDGET,
                   leaf_points: int = LEAF_POINTS) -> Dict:
    """Measure ``model`` on the grid of ``preset`` in the seeded processing order (the first
    ``max_partitions`` of it); ``results``: the directory of a verify run (``<model>.csv``).  Writes
    ``rate.csv`` / ``rate.json`` to ``out_dir`` and returns the summary.  ``certify``: also count the
    sampled partitions (:func:`certify_grid`), write ``bounds.csv`` and report the certified bounds."""
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
    out = {"preset": preset, "model": model, "samples_per_partition": int(n_samples), "seed": int(seed)}
    summary, verdict, samples, flips = measure_grid(grid, q, be, order, table, n_samples, seed, check_unsat, conf,
                                                    resolve)
    out.update(summary)
    bounds = None
    if certify:
        cert, bounds = certify_grid(grid, q, be, order, table, node_budget, leaf_points, check_unsat)
        out.update(cert)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "rate.csv"), "w", newline="") as fp:
            wr = csv.writer(fp)
            wr.writerow(CSV_HEADER)
            for k in range(len(order)):
                s = int(samples[k])
                wr.writerow([k + 1, int(order[k]), _NAMES[int(verdict[k])], s, int(flips[k]),
                             repr(int(flips[k]) / s) if s else "0.0"])
        with open(os.path.join(out_dir, "rate.json"), "w") as fp:
            json.dump(out, fp, indent=2)
        if bounds is not None:
            with open(os.path.join(out_dir, "bounds.csv"), "w", newline="") as fp:
                wr = csv.writer(fp)
                wr.writerow(BOUNDS_HEADER)
                wr.writerows(bounds)
    return out
