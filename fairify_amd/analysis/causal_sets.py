"""``causal`` command: which attributes, and which small sets of attributes, do the model's decisions
causally depend on?

``verify`` / ``measure`` / ``audit`` speak about the *declared* protected attributes; this module runs
Themis's discrimination search (``engine/causal.py``) over every attribute set of size 1 ..
``max_size``: a set is discriminatory when, for more than ``threshold`` of the base rows, some other
assignment of the set's attributes changes the predicted class.  Every flip is decided with the
project's guarantee (rigorous fp32 bounds on the device, exact arithmetic for what fp32 cannot
decide), so ``causal.csv`` is the same bytes on CPU and GPU.  One base table is shared by all sets
(docs/DESIGN.md 5h); ``analysis/causal.py`` keeps the reference's detector for ``analyze``.
"""
from __future__ import annotations

import csv
import json
import os
from typing import Dict, List, Optional

import numpy as np

from .. import presets
from ..engine.causal import IMPLIED, causal_search
from ..models.zoo import get_model
from ..ops import causal as CS
from ..ops.backend import Backend
from .audit import load_rows

COLUMNS = ["features", "size", "assignments", "status", "samples_used", "flips", "rate", "half_width",
           "discriminatory", "flips_all", "rate_all"]


def thin(values: np.ndarray, k: Optional[int]) -> np.ndarray:
    """At most ``k`` of the sorted values, evenly spaced by rank, the first and the last kept."""
    values = np.asarray(values)
    if k is None or len(values) <= k:
        return values
    if k < 2:
        raise ValueError("causal: --max-values must be at least 2")
    return values[np.unique(np.rint(np.linspace(0, len(values) - 1, int(k))).astype(np.int64))]


def value_lists(dom, source: str, rows: Optional[np.ndarray], max_values: Optional[int]) -> List[np.ndarray]:
    """Per-feature value lists: ``data`` -- the values observed in ``rows`` (Themis's ``from_data``);
    ``domain`` -- ``lo .. hi``; either thinned to ``max_values``."""
    if source == "data":
        lists = [np.unique(rows[:, k]) for k in range(dom.n)]
    elif source == "domain":
        lists = [np.arange(int(f.lo), int(f.hi) + 1, dtype=np.int64) for f in dom.features]
    else:
        raise ValueError(f"causal: values {source!r} is not data or domain")
    return [thin(v, max_values).astype(np.int64) for v in lists]


def causal_preset(preset: str, model: str, max_size: int = 2, samples: int = 1000, seed: int = 42,
                  threshold: float = 0.15, conf: float = 0.99, margin: float = 0.01, min_samples: int = 100,
                  values: str = "data", max_values: Optional[int] = None,
                  max_assignments: int = CS.MAX_ASSIGNMENTS, base: str = "sampled", data: Optional[str] = None,
                  split: str = "all", weights: str = "zoo", device: str = "cpu", out_dir: Optional[str] = None,
                  pairs_out: Optional[str] = None) -> Dict:
    """Search ``model``'s attribute sets under the domain of ``preset``.  ``values``: where the value
    lists come from (``data``: the suite's dataset or the CSV ``data``; ``domain``: the whole range);
    ``base``: ``sampled`` draws ``samples`` base rows from the lists (``ops/causal.draw_base``),
    ``data`` takes the first ``samples`` real rows (0: all of them).  Writes ``causal.csv`` /
    ``causal.json`` to ``out_dir`` and, with ``pairs_out``, an ``.npz`` of the exactly confirmed pair
    of every discriminatory set (``x``, ``xp``), which ``repair --counterexamples`` reads.  Returns the
    summary."""
    if base not in ("sampled", "data"):
        raise ValueError(f"causal: base {base!r} is not sampled or data")
    pre = presets.get(preset)
    dom = pre.domain()
    q = pre.resolved()
    mlp = get_model(model, weights=weights, seed=0)
    be = Backend(mlp, device=device)
    rows, src = None, {"data": None, "synthetic": False}
    if values == "data" or base == "data":
        rows, src = load_rows(pre, data, split, 0)
    lists = value_lists(dom, values, rows, max_values)
    if base == "data":
        X = rows[:samples] if samples else rows
    else:
        X = CS.draw_base(lists, samples, seed)
    res = causal_search(be, lists, X, max_size=max_size, max_assignments=max_assignments, threshold=threshold,
                        conf=conf, margin=margin, min_samples=min_samples)
    S = int(X.shape[0])
    name = lambda dims: "+".join(dom.names[d] for d in dims)
    minimal = [{"features": [dom.names[d] for d in r.dims], "rate": r.rate, "half_width": r.half_width,
                "samples_used": r.used, "flips": r.flips, "assignments": r.assignments,
                "pair": None if r.pair is None else {"x": list(r.pair[0]), "xp": list(r.pair[1])}}
               for r in res.minimal]
    pa = tuple(sorted(q.pa_idx))
    by_dims = {r.dims: r for r in res.sets}
    inside = [m for m in res.minimal if set(m.dims) <= set(pa)]
    declared = [{"features": [dom.names[d] for d in pa],
                 "status": by_dims[pa].status if pa in by_dims else "not-searched",
                 "minimal": pa in by_dims and by_dims[pa].discriminatory,
                 "implied_by": [name(m.dims) for m in inside if m.dims != pa]}]
    out = {"preset": preset, "model": model, "source": src, "synthetic": bool(src.get("synthetic", False)),
           "settings": {"max_size": int(max_size), "samples": S, "seed": int(seed), "threshold": threshold,
                        "conf": conf, "margin": margin, "min_samples": int(min_samples), "values": values,
                        "max_values": max_values, "max_assignments": int(max_assignments), "base": base},
           "list_sizes": {dom.names[k]: int(len(v)) for k, v in enumerate(lists)},
           "sets": len(res.sets), "tested": sum(r.status == "tested" for r in res.sets),
           "implied": sum(r.status == IMPLIED for r in res.sets),
           "too_many_assignments": sum(r.status == "too-many-assignments" for r in res.sets),
           "minimal": minimal, "declared_pa": declared, "ambiguous": int(res.ambiguous), "fused": bool(res.fused)}
    if pairs_out:
        got = [r.pair for r in res.minimal if r.pair is not None]
        x = np.array([p[0] for p in got], dtype=np.int64).reshape(-1, dom.n)
        xp = np.array([p[1] for p in got], dtype=np.int64).reshape(-1, dom.n)
        os.makedirs(os.path.dirname(os.path.abspath(pairs_out)), exist_ok=True)
        np.savez(pairs_out, x=x, xp=xp)
        out["pairs_out"] = pairs_out
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "causal.csv"), "w", newline="") as fp:
            wr = csv.writer(fp)
            wr.writerow(COLUMNS)
            for r in res.sets:
                wr.writerow([name(r.dims), r.size, r.assignments, r.status, r.used, r.flips, repr(float(r.rate)),
                             repr(float(r.half_width)), int(r.discriminatory), r.flips_all,
                             repr(r.flips_all / S if S else 0.0)])
        with open(os.path.join(out_dir, "causal.json"), "w") as fp:
            json.dump(out, fp, indent=2)
    return out
