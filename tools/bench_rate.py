"""Timing of the fused discrimination-rate kernel against the composition of existing ops.

    python tools/bench_rate.py [--partitions 8192] [--samples 1000] [--pairs 7] [--reps 20] [--models AC-4,AC-7] [--out FILE]

Both sides compute the rigorous logit bounds of every x row of every sampled profile of the first
``--partitions`` partitions of ``src/AC-sex`` (seeded order), random-init weights:

* fused: one ``hip.rate_counts`` launch (csrc/rate.hip; points generated in registers);
* composed: ``ref.sample_points`` on the device, the PA overwrite, ``hip.point_bounds`` on the
  materialised rows (1 024 partitions per slice, so the temporaries stay below 1 GB).

Interleaved pairs after a warm-up of both; a timed window is ``--reps`` calls ended by a device
synchronise (a few hundred ms).  Prints the median and the spread of both, per call, and the
per-pair ratio.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partitions", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window (ms reported per call)")
    ap.add_argument("--models", default="AC-4,AC-7")
    ap.add_argument("--slice", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate needs a GPU")

    from fairify_amd import presets
    from fairify_amd.models.zoo import get_model
    from fairify_amd.ops import hip
    from fairify_amd.ops import rate as R
    from fairify_amd.ops import reference as ref
    from fairify_amd.ops.backend import Backend
    from fairify_amd.partition import processing_order

    dev = torch.device("cuda:0")
    pre = presets.get("src/AC-sex")
    grid, q = pre.grid(), pre.resolved()
    ids = processing_order(grid, seed=0)[:args.partitions]
    pids = torch.from_numpy(ids).to(dev)
    lo, hi = hip.decode(grid, pids)
    lo_np, hi_np = grid.decode(ids[:1])
    values_np = q.pa_values(lo_np[0], hi_np[0])
    values = torch.from_numpy(values_np).to(dev)
    pairs = torch.from_numpy(q.pa_pairs(values_np)).to(dev)
    pa = torch.tensor(list(q.pa_idx), device=dev)
    S, V, n = args.samples, values.shape[0], lo.shape[1]
    sync = torch.cuda.synchronize

    def fused(be):
        return hip.rate_counts(be, q, lo, hi, pids, S, 0, values, pairs)

    def composed(be):
        out = []
        for s0 in range(0, lo.shape[0], args.slice):
            sl = slice(s0, s0 + args.slice)
            X = ref.sample_points(lo[sl], hi[sl], pids[sl], S, 0)
            XV = X[:, :, None, :].expand(-1, S, V, n).clone()
            XV[:, :, :, pa] = values.to(torch.float32)[None, None].expand(XV.shape[0], S, V, -1)
            out.append(hip.point_bounds(be, XV.reshape(-1, n)))
        return out

    def timed(fn, be):
        sync()
        t = time.perf_counter()
        for _ in range(args.reps):
            fn(be)
        sync()
        return (time.perf_counter() - t) * 1e3 / args.reps

    res = {"partitions": int(lo.shape[0]), "samples": S, "rows": int(lo.shape[0]) * S * V, "pairs": args.pairs,
           "reps": args.reps, "models": {}}
    for name in args.models.split(","):
        be = Backend(get_model(name, weights="random", seed=0), device=dev)
        # same outputs: the two kernels share the layer arithmetic (csrc/pointfwd.h)
        f, a, _ = fused(be)
        fr, ar, _ = R.rate_counts_ref(be, q, lo[:512], hi[:512], pids[:512], S, 0, values, pairs)
        same = bool(torch.equal(f[:512], fr) and torch.equal(a[:512], ar))
        for _ in range(2):
            timed(fused, be)
            timed(composed, be)
        tf, tc = [], []
        for _ in range(args.pairs):
            tf.append(timed(fused, be))
            tc.append(timed(composed, be))
        ratio = [c / f_ for c, f_ in zip(tc, tf)]
        res["models"][name] = {
            "widths": be.widths, "counts_equal_composition": same,
            "certain": int(f.sum()), "ambiguous": int(a.sum()),
            "fused_ms": {"median": statistics.median(tf), "min": min(tf), "max": max(tf)},
            "composed_ms": {"median": statistics.median(tc), "min": min(tc), "max": max(tc)},
            "composed_over_fused": {"median": statistics.median(ratio), "min": min(ratio), "max": max(ratio)},
        }
        print(name, json.dumps(res["models"][name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(res, fp, indent=2)


if __name__ == "__main__":
    main()
