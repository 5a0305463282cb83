#!/usr/bin/env python
"""Run ``verify_chunk`` over a fixed list of configurations and save each one's core columns as one
``.npz``, or compare two such directories column by column (every column but the times).

    python tools/pipeline_matrix.py --out DIR [--device cuda] [--tree OTHER_CHECKOUT] [--only a,b]
    python tools/pipeline_matrix.py --compare DIR_A DIR_B

Used to show that a change of the pipeline's structure moves no result: run it on a checkout of the
parent commit (``--tree``) twice and on the new tree, and compare.  Only configurations whose two
parent runs are equal count as evidence.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

A = dict(node_budget=16, escalate_budget=256, relu_budget=128, residual_samples=256, heuristic=True,
         keep_masks=True, pruned_metrics=True)
# name -> (preset, model, model seed, ids, query PA / partition size override, environment, VerifyConfig fields)
CONFIGS = {
    "a": ("src/AC-sex", "AC-8", 0, 64, None, {}, A),
    "b": ("src/AC-sex", "AC-8", 0, 64, None, {},
          dict(node_budget=16, escalate_budget=64, escalate_stages=((256, 0),), relu_budget=0, beta_budget=64,
               beta_min_width=1, residual_samples=0, heuristic=True, heuristic_node_budget=16)),
    "c": ("src/AC-sex", "AC-8", 0, 64, None, {"FAIRIFY_FAULT_FORCE_UNKNOWN": "0.5"},
          dict(node_budget=64, relu_budget=64, residual_samples=256, heuristic=True)),
    "a_escalate_first": ("src/AC-sex", "AC-8", 0, 64, None, {}, dict(A, relu_first=False, heuristic=False)),
    "relaxed_ac": ("relaxed/AC", "AC-8", 0, 32, None, {},
                   dict(node_budget=16, relu_budget=64, residual_samples=128)),
    "gc3": ("src/GC-age", "GC-3", 0, 48, None, {}, dict(node_budget=16, heuristic=True, keep_masks=True)),
    "anytime": ("src/AC-sex", "AC-8", 0, 32, None, {},
                dict(node_budget=8, relu_budget=0, relu_max_width=1, anytime_seconds=600, anytime_beta=0,
                     residual_samples=64)),
    "anytime_lp": ("src/AC-sex", "AC-8", 0, 48, None, {},
                   dict(sim_size=200, node_budget=32, heuristic=False, relu_budget=0, smt_backend="auto",
                        anytime_seconds=20, lp_budget=256, smt_workers=2)),
    "two_groups": ("src/AC-sex", "AC-8", 1, 40, (("age",), 30), {},
                   dict(node_budget=64, heuristic=False, residual_samples=0)),
}
TIME_COLUMNS = ("sv_time", "s_time", "hv_time", "h_time", "total_time")


def run(args) -> None:
    sys.path.insert(0, os.path.abspath(args.tree))
    from dataclasses import replace

    import torch

    from fairify_amd import presets
    from fairify_amd.engine.pipeline import VerifyConfig, _lp_available, verify_chunk
    from fairify_amd.models.zoo import get_model
    from fairify_amd.ops.backend import Backend
    from fairify_amd.partition import processing_order
    from fairify_amd.spec import Query

    os.makedirs(args.out, exist_ok=True)
    for name in (args.only.split(",") if args.only else CONFIGS):
        preset, model, mseed, n_ids, regroup, env, fields = CONFIGS[name]
        if name == "anytime_lp" and not _lp_available():
            print(f"{name}: skipped (no HiGHS bindings)", flush=True)
            continue
        pre = presets.get(preset)
        if regroup is not None:
            pre = replace(pre, query=Query(regroup[0]), partition_size=regroup[1])
        grid, q = pre.grid(), pre.resolved()
        m = get_model(model, weights="random", seed=mseed)
        ids = processing_order(grid, 0)[:n_ids]
        cfg = VerifyConfig(**{"sim_size": 128, "smt_backend": "none", **fields})
        os.environ.update(env)
        t0 = time.time()
        try:
            core = verify_chunk(Backend(m, device=torch.device(args.device)), m, q, grid, ids, cfg).core
        finally:
            for k in env:
                del os.environ[k]
        cols = {k: (v.astype(str) if v.dtype == object else v) for k, v in core.items()}
        np.savez(os.path.join(args.out, name + ".npz"), **cols)
        stages, counts = np.unique(cols["stage"], return_counts=True)
        print(f"{name}: {time.time() - t0:.1f} s, stages {dict(zip(stages.tolist(), counts.tolist()))}", flush=True)


def compare(dir_a: str, dir_b: str) -> int:
    differing = 0
    for name in CONFIGS:
        fa, fb = (os.path.join(d, name + ".npz") for d in (dir_a, dir_b))
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print(f"{name}: missing")
            continue
        a, b = np.load(fa), np.load(fb)
        keys = sorted((set(a.files) | set(b.files)) - set(TIME_COLUMNS))
        bad = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k])]
        differing += bool(bad)
        print(f"{name}: {len(keys) - len(bad)} of {len(keys)} columns equal" + (f"; differ: {bad}" if bad else ""))
    return 1 if differing else 0


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="directory for the .npz files")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose fairify_amd package runs (default: this one)")
    ap.add_argument("--only", default="", help="comma-separated configuration names")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("--out or --compare is required")
    run(args)


if __name__ == "__main__":
    main()
