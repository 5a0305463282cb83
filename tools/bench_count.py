"""Timing of the counting branch-and-bound (`measure --certify`) and of its enumeration kernel.

    python tools/bench_count.py [--partitions 256] [--node-budget 65536] [--leaf-points 1024]
                                [--cases src/AC-sex:AC-1,src/AC-sex:AC-3,src/GC-age:GC-1] [--enum-blocks 1024,4096]
                                [--out FILE]

Per case (zoo weights, the first ``--partitions`` partitions of the seeded order): one untimed
warm-up call of the same shape, then ``--runs`` calls of ``count_partitions`` for the wall time
(host clock around the call, which ends in device read-backs) and the certified bounds, then one
more with a synchronising stage timer for the shares of rows / bounds / level / enumeration (every
stage boundary waits for the device there).

Enumeration kernel against ``fa_rate_kernel`` at the same net and V: ``--enum-leaves`` leaves of at
most ``--leaf-points`` points (each partition box shrunk from its last dim) against the same number
of partitions with as many hash-stream profiles each; interleaved pairs after a warm-up, a timed
window is ``--reps`` calls ended by a device synchronise; nanoseconds per point.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def shrink(lo, hi, free, limit):
    """Sub-boxes of at most ``limit`` non-PA points: widths cut from the last free dim backwards."""
    lo, hi = lo.copy(), hi.copy()
    for k in range(lo.shape[0]):
        room = limit
        for d in reversed(free):
            w = int(min(hi[k, d] - lo[k, d] + 1, max(room, 1)))
            hi[k, d] = lo[k, d] + w - 1
            room //= w
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--node-budget", type=int, default=None)
    ap.add_argument("--leaf-points", type=int, default=None)
    ap.add_argument("--cases", default="src/AC-sex:AC-1,src/AC-sex:AC-3,src/GC-age:GC-1")
    ap.add_argument("--enum-leaves", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--enum-blocks", default="", help="also time the enum kernel at these workgroup counts, e.g. 1024,4096")
    ap.add_argument("--skip-kernel-bench", action="store_true", help="no enum / rate kernel comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_count needs a GPU")

    from fairify_amd import presets
    from fairify_amd.engine import count as EC
    from fairify_amd.engine.search import pa_table
    from fairify_amd.models.zoo import get_model
    from fairify_amd.ops import count as OC
    from fairify_amd.ops import hip
    from fairify_amd.ops.backend import Backend
    from fairify_amd.partition import processing_order
    from fairify_amd.utils.timer import StageTimer

    dev = torch.device("cuda:0")
    budget = args.node_budget or EC.NODE_BUDGET
    leaf = args.leaf_points or EC.LEAF_POINTS
    sync = torch.cuda.synchronize
    res = {"partitions": args.partitions, "node_budget": budget, "leaf_points": leaf, "cases": {}}

    def dump():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fp:
                json.dump(res, fp, indent=2)

    for case in args.cases.split(","):
        preset, model = case.split(":")
        pre = presets.get(preset)
        grid, q = pre.grid(seed=0), pre.resolved()
        be = Backend(get_model(model, weights="zoo", seed=0), device=dev)
        ids = processing_order(grid, seed=0)[:args.partitions]
        lo_np, hi_np = grid.decode(ids)
        lo = torch.from_numpy(lo_np).to(dev, torch.float32)
        hi = torch.from_numpy(hi_np).to(dev, torch.float32)
        pids = torch.from_numpy(ids).to(dev)
        EC.count_partitions(be, q, lo, hi, pids, budget, leaf)                   # warm-up: kernels loaded, pools allocated
        walls = []
        for _ in range(args.runs):
            sync()
            t = time.perf_counter()
            r = EC.count_partitions(be, q, lo, hi, pids, budget, leaf)
            sync()
            walls.append(time.perf_counter() - t)
        W = sum(EC.box_weights(q, lo_np, hi_np))
        un, op = int(r.unfair.astype(object).sum()), int(r.open.astype(object).sum())
        tm = StageTimer(dev, sync=True)
        t = time.perf_counter()
        EC.count_partitions(be, q, lo, hi, pids, budget, leaf, timer=tm)
        wall_timed = time.perf_counter() - t
        out = {"widths": be.widths, "partitions": len(ids),
               "wall_s": {"median": statistics.median(walls), "min": min(walls), "max": max(walls)},
               "certified_lower": un / W, "certified_upper": (un + op) / W,
               "nodes": int(r.nodes.sum()), "exact_partitions": int((r.open == 0).sum()),
               "fair_share": int(r.fair.astype(object).sum()) / W,
               "stats": r.stats, "timed_run_wall_s": wall_timed, "stage_s": dict(tm.t), "stage_calls": dict(tm.n)}
        if args.skip_kernel_bench:
            res["cases"][case] = out
            print(case, json.dumps(out), flush=True)
            dump()
            continue
        # enumeration kernel against the rate kernel, same net and V
        ids_e = processing_order(grid, seed=0)[:args.enum_leaves]
        elo_np, ehi_np = grid.decode(ids_e)
        groups = EC.pa_groups(q, elo_np, ehi_np)
        keep = groups[0]                                                          # one PA table
        elo_np, ehi_np, ids_e = elo_np[keep], ehi_np[keep], ids_e[keep]
        values, pairs = pa_table(q, elo_np, ehi_np)
        vt, pt = torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)
        llo_np, lhi_np = shrink(elo_np, ehi_np, OC.free_dims(q), leaf)
        llo = torch.from_numpy(llo_np).to(dev, torch.float32)
        lhi = torch.from_numpy(lhi_np).to(dev, torch.float32)
        elo = torch.from_numpy(elo_np).to(dev, torch.float32)
        ehi = torch.from_numpy(ehi_np).to(dev, torch.float32)
        epid = torch.from_numpy(ids_e).to(dev)
        points = int(OC.volumes(llo, lhi, OC.free_dims(q)).sum())
        S = max(1, points // len(ids_e))

        def enum():
            return hip.count_enum(be, q, llo, lhi, vt, pt, max_vol=leaf)

        def rate():
            return hip.rate_counts(be, q, elo, ehi, epid, S, 0, vt, pt)

        def timed(fn):
            sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            sync()
            return (time.perf_counter() - t0) / args.reps

        for _ in range(2):
            timed(enum)
            timed(rate)
        te, tr = [], []
        for _ in range(args.pairs):
            te.append(timed(enum) * 1e9 / points)
            tr.append(timed(rate) * 1e9 / (S * len(ids_e)))
        if args.enum_blocks:
            fns = {int(b): (lambda b=int(b): hip.count_enum(be, q, llo, lhi, vt, pt, max_vol=leaf, blocks=b))
                   for b in args.enum_blocks.split(",")}
            tb = {b: [] for b in fns}
            for f in fns.values():
                timed(f)
            for _ in range(args.pairs):
                for b, f in fns.items():
                    tb[b].append(timed(f) * 1e9 / points)
            out["enum_ns_per_point_by_blocks"] = {str(b): statistics.median(v) for b, v in tb.items()}
        out["enum_vs_rate"] = {"V": int(values.shape[0]), "leaves": len(ids_e), "points": points, "rate_profiles": S * len(ids_e),
                               "enum_ns_per_point": {"median": statistics.median(te), "min": min(te), "max": max(te)},
                               "rate_ns_per_point": {"median": statistics.median(tr), "min": min(tr), "max": max(tr)}}
        res["cases"][case] = out
        print(case, json.dumps(out), flush=True)
        dump()


if __name__ == "__main__":
    main()
