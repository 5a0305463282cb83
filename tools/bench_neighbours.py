"""Single-attribute neighbourhoods: the fused kernel against the composed path (the audit kernel fed
materialised neighbours), whole ``audit_neighbours`` calls on zoo shapes.

    python tools/bench_neighbours.py [--rows 65536] [--pairs 7] [--calls 4] [--out FILE.json]

Per case: one warm-up call of each arm (which also checks that both give the same ``flag``), then
``--pairs`` alternating pairs of windows (fused, composed / composed, fused / ...); a window is
``--calls`` calls between two device synchronises, host clock; seconds per call.  The composed arm is
selected with ``FAIRIFY_NEIGHBOURS_FUSED=0``.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fairify_amd import presets                                  # noqa: E402
from fairify_amd.data import tabular                             # noqa: E402
from fairify_amd.engine.neighbours import audit_neighbours, device_words  # noqa: E402
from fairify_amd.models.zoo import get_model                     # noqa: E402
from fairify_amd.ops import audit as A                           # noqa: E402
from fairify_amd.ops import neighbours as NB                     # noqa: E402
from fairify_amd.ops.backend import Backend                      # noqa: E402

CASES = [("src/AC-sex", "AC-3", None), ("src/AC-sex", "AC-7", None),
         ("src/GC-age", "GC-1", {"credit_amount": 3, "month": 5}),
         ("src/BM-age", "BM-8", {"duration": 3, "pdays": 3})]


def window(be, q, X, table, fused, calls):
    """(seconds per call, last result) of ``calls`` whole calls of one arm."""
    os.environ["FAIRIFY_NEIGHBOURS_FUSED"] = "1" if fused else "0"
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        r = audit_neighbours(be, q, X, radii=table)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbours: no GPU")
    results = []
    for preset, model, radii in CASES:
        pre = presets.get(preset)
        q = pre.resolved()
        X = tabular.synthetic(pre.domain(), n=a.rows, seed=1).df[pre.domain().names].to_numpy().astype(np.int64)
        be = Backend(get_model(model, weights="zoo"), device="cuda:0")
        table = NB.neighbour_table(q, radii)
        tf, rf = window(be, q, X, table, True, 1)
        tc, rc = window(be, q, X, table, False, 1)
        if not rf.fused or rc.fused:
            raise SystemExit(f"bench_neighbours: {model}: the arms did not take their paths")
        same = bool(np.array_equal(rf.flag, rc.flag))
        F, C = [], []
        for i in range(a.pairs):
            for fused in ((True, False) if i % 2 == 0 else (False, True)):
                t, r = window(be, q, X, table, fused, a.calls)
                (F if fused else C).append(t)
                same = same and bool(np.array_equal(r.flag, rf.flag))
        # the device part alone (rows up, one launch or the chunked composition, words back), same windows
        values, pairs = A.pa_domain_table(q)
        own = A.own_index(q, X, values)
        DF, DC = [], []
        for i in range(a.pairs):
            for fused in ((True, False) if i % 2 == 0 else (False, True)):
                os.environ["FAIRIFY_NEIGHBOURS_FUSED"] = "1" if fused else "0"
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.calls):
                    device_words(be, q, X, own, values, pairs, table)
                torch.cuda.synchronize()
                (DF if fused else DC).append((time.perf_counter() - t) / a.calls)
        F, C = np.array(F), np.array(C)
        d = C - F
        rec = {"preset": preset, "model": model, "widths": [int(w) for w in be.widths], "rows": int(a.rows),
               "M": table.M, "pairs": int(a.pairs), "calls_per_window": int(a.calls), "same_flag": same,
               "valid_neighbours": int(sum(NB.neighbour_values(X[s:s + 4096], table)[1].sum()
                                           for s in range(0, len(X), 4096))),
               "flagged_neighbours": int(NB.unpack_bits(rf.flag, table.M).sum()), "ambiguous": int(rf.ambiguous),
               "warmup_s": [tf, tc], "fused_s": F.tolist(), "composed_s": C.tolist(),
               "fused_median_s": float(np.median(F)), "composed_median_s": float(np.median(C)),
               "diff_median_s": float(np.median(d)), "diff_min_s": float(d.min()), "diff_max_s": float(d.max()),
               "diff_mad_s": float(np.median(np.abs(d - np.median(d)))),
               "device_fused_median_s": float(np.median(DF)), "device_composed_median_s": float(np.median(DC)),
               "device_fused_s": DF, "device_composed_s": DC}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fp:
                json.dump(results, fp, indent=1)


if __name__ == "__main__":
    main()
