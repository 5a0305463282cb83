"""Timing of the fused audit kernel against the composed device path, and of the whole command.

    python tools/bench_audit.py [--rows 65536] [--pairs 7] [--window 0.25] [--cases ...] [--blocks 256,512]
                                [--command-rows 45222] [--out FILE]

Both sides compute the audit masks (ops/audit.py) of the same ``--rows`` synthetic rows of the
preset's domain, zoo weights:

* fused: one ``hip.audit_masks`` launch (csrc/audit.hip);
* composed: ``ops/audit.audit_masks_ref`` on the same CUDA backend -- ``profile_rows`` on the
  device, ``hip.point_bounds`` on the materialised rows, the mask arithmetic in torch.

Two untimed warm-up calls of each, a calibration call that sizes the windows (``--window`` seconds of
calls each), then ``--pairs`` alternating pairs of windows, every window ended by one device
synchronise.  Reports the median with min and max per call, the paired differences composed - fused
(median and their median absolute deviation) and the decision rule of the default path: fused is
kept iff it is faster in the median AND the median paired difference exceeds the MAD of the
differences.  ``--blocks``: also time the fused launch at these workgroup counts.  Last, the wall
time of the whole ``audit`` command (``analysis/audit.audit_preset``: CSV read, masks, exact
resolution, cross-check, witnesses, files written) on ``--command-rows`` rows (the Adult table has
45 222 complete rows) on the GPU and on the CPU.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

CASES = "src/AC-sex:AC-1,src/AC-sex:AC-3,src/AC-sex:AC-7,relaxed/AC:AC-3"


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of calls per timed window")
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--blocks", default="", help="comma list of workgroup counts to time the fused launch at")
    ap.add_argument("--command-rows", type=int, default=45222, help="0: skip the whole-command timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pairs < 7:
        raise SystemExit("bench_audit: at least 7 pairs of windows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_audit needs a GPU")

    from fairify_amd import presets
    from fairify_amd.data import tabular
    from fairify_amd.models.zoo import get_model
    from fairify_amd.ops import audit as A
    from fairify_amd.ops import hip
    from fairify_amd.ops.backend import Backend

    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize

    def window(fn, reps):
        sync()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        return (time.perf_counter() - t) * 1e3 / reps

    def reps_for(fn):
        return max(1, min(2000, int(args.window * 1e3 / max(window(fn, 1), 1e-3)) + 1))

    res = {"rows": args.rows, "pairs": args.pairs, "window_s": args.window, "cases": {}}
    for case in args.cases.split(","):
        preset, model = case.split(":")
        pre = presets.get(preset)
        q = pre.resolved()
        ds = tabular.synthetic(pre.domain(), n=args.rows, seed=0)
        Xn = A.integral_rows(np.concatenate([ds.X_train, ds.X_test]))
        values_np, pairs_np = A.pa_domain_table(q)
        own_np = A.own_index(q, Xn, values_np)
        be = Backend(get_model(model, weights="zoo", seed=0), device=dev)
        X = torch.from_numpy(Xn).to(dev, torch.float32)
        own = torch.from_numpy(own_np).to(dev)
        values, pairs = torch.from_numpy(values_np).to(dev), torch.from_numpy(pairs_np).to(dev)
        E = int((2 * q.tau + 1) ** len(q.ra_idx)) if q.relaxed else 1
        table = np.zeros((values_np.shape[0],) * 2, bool)
        table[pairs_np[:, 0], pairs_np[:, 1]] = True
        counterparts = int(table[own_np[own_np >= 0]].sum()) * E

        def fused(blocks=None):
            return hip.audit_masks(be, q, X, own, values, pairs, blocks=blocks)

        def composed():
            return A.audit_masks_ref(be, q, X, own, values, pairs)

        f = fused()
        if f is None:
            res["cases"][case] = {"widths": be.widths, "fused": None}
            print(case, "fused kernel declines this shape", flush=True)
            continue
        c = composed()
        same = all(bool(torch.equal(a, b)) for a, b in zip(f, c))
        for _ in range(2):
            fused()
            composed()
        rf, rc = reps_for(fused), reps_for(composed)
        tf, tc = [], []
        for _ in range(args.pairs):
            tf.append(window(fused, rf))
            tc.append(window(composed, rc))
        diff = [b - a for a, b in zip(tf, tc)]
        md = statistics.median(diff)
        mad = statistics.median([abs(d - md) for d in diff])
        keep = statistics.median(tf) < statistics.median(tc) and md > mad
        out = {"widths": be.widths, "V": int(values_np.shape[0]), "E": E, "counterpart_rows": counterparts,
               "masks_equal_composition": same, "cert_bits": int(sum(bin(v & 0xFFFFFFFF).count("1") for v in f[0].tolist())),
               "ambiguous_bits": int(sum(bin((p & ~c_) & 0xFFFFFFFF).count("1")
                                         for c_, p in zip(f[0].tolist(), f[1].tolist()))),
               "reps": {"fused": rf, "composed": rc},
               "fused_ms": _stats(tf), "composed_ms": _stats(tc), "fused_ms_windows": tf, "composed_ms_windows": tc,
               "paired_diff_ms": {"values": diff, "median": md, "mad": mad},
               "fused_ns_per_counterpart_row": statistics.median(tf) * 1e6 / max(1, counterparts),
               "fused_is_default": bool(keep)}
        for b in [int(v) for v in args.blocks.split(",") if v]:
            if 1 <= b <= hip.audit_passes(args.rows):
                out.setdefault("fused_ms_by_blocks", {})[str(b)] = _stats(
                    [window(lambda: fused(b), rf) for _ in range(args.pairs)])
        res["cases"][case] = out
        print(case, json.dumps(out), flush=True)

    if args.command_rows:
        from fairify_amd.analysis.audit import audit_preset

        pre = presets.get("src/AC-sex")
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "rows.csv")
            tabular.synthetic(pre.domain(), n=args.command_rows, seed=1).df.to_csv(path, index=False)
            cmd = {"rows": args.command_rows, "preset": "src/AC-sex", "model": "AC-3", "input": "synthetic domain rows"}
            for device in ("cuda:0", "cuda:0", "cpu"):          # the first GPU call is the warm-up
                t = time.perf_counter()
                out = audit_preset("src/AC-sex", "AC-3", data=path, device=device, out_dir=os.path.join(tmp, "o"),
                                   pairs_out=os.path.join(tmp, "p.npz"))
                cmd[device + "_wall_s"] = time.perf_counter() - t
                cmd["flagged"] = out["flagged"]
        res["command"] = cmd
        print("command", json.dumps(cmd), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(res, fp, indent=2)


if __name__ == "__main__":
    main()
