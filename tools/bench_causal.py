"""Causal search over attribute sets: the fused kernel against the composed path (``point_bounds`` fed
materialised altered rows), whole ``causal_search`` calls on zoo shapes.

    python tools/bench_causal.py [--case AC-3] [--rows 16384] [--pairs 5] [--calls 1] [--out FILE.json]

Per case (``--values domain --max-values 10 --max-size 2`` of the ``causal`` command, drawn base rows):
one warm-up call of each arm, then ``--pairs`` alternating pairs of windows (fused, composed /
composed, fused / ...); a window is ``--calls`` calls between two device synchronises, host clock;
seconds per call.  Every window's exact flip bits are compared with the warm-up's.  The arms are
selected with ``FAIRIFY_CAUSAL_FUSED=1`` / ``0``.  ``--case`` runs one case, so that each can have a
time limit of its own.  Needs a GPU: there is no fall-back.
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
from fairify_amd.analysis.causal_sets import value_lists         # noqa: E402
from fairify_amd.engine.causal import causal_search              # noqa: E402
from fairify_amd.models.zoo import get_model                     # noqa: E402
from fairify_amd.ops import causal as CS                         # noqa: E402
from fairify_amd.ops.backend import Backend                      # noqa: E402

CASES = [("src/AC-sex", "AC-3"), ("src/AC-sex", "AC-7"), ("src/GC-age", "GC-1"), ("src/BM-age", "BM-8")]


def window(be, lists, X, fused, calls):
    """(seconds per call, last result) of ``calls`` whole calls of one arm."""
    os.environ["FAIRIFY_CAUSAL_FUSED"] = "1" if fused else "0"
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        r = causal_search(be, lists, X, max_size=2)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls, r


def same_bits(a, b) -> bool:
    return a.flip.keys() == b.flip.keys() and all(np.array_equal(a.flip[s], b.flip[s]) for s in a.flip) \
        and a.sets == b.sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="one model of the case list (default: all)")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--max-values", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_causal: no GPU")
    cases = [c for c in CASES if a.case in (None, c[1])]
    if not cases:
        raise SystemExit(f"bench_causal: {a.case!r} is not one of {[c[1] for c in CASES]}")
    results = []
    for preset, model in cases:
        dom = presets.get(preset).domain()
        lists = value_lists(dom, "domain", None, a.max_values)
        X = CS.draw_base(lists, a.rows, 42)
        be = Backend(get_model(model, weights="zoo"), device="cuda:0")
        tf, rf = window(be, lists, X, True, 1)
        tc, rc = window(be, lists, X, False, 1)
        if not rf.fused or rc.fused:
            raise SystemExit(f"bench_causal: {model}: the arms did not take their paths")
        same = same_bits(rf, rc)
        F, C = [], []
        for i in range(a.pairs):
            for fused in ((True, False) if i % 2 == 0 else (False, True)):
                t, r = window(be, lists, X, fused, a.calls)
                (F if fused else C).append(t)
                same = same and same_bits(r, rf)
        F, C = np.array(F), np.array(C)
        d = C - F
        tested = [s for s in rf.sets if s.status == "tested"]
        rec = {"preset": preset, "model": model, "widths": [int(w) for w in be.widths], "rows": int(a.rows),
               "sets": len(rf.sets), "tested": len(tested), "assignments": int(sum(s.assignments for s in tested)),
               "discriminatory": len(rf.minimal), "pairs": int(a.pairs), "calls_per_window": int(a.calls),
               "same_bits": bool(same), "ambiguous_fused": int(rf.ambiguous), "ambiguous_composed": int(rc.ambiguous),
               "bytes": int(a.rows) * len(tested),
               "warmup_s": [tf, tc], "fused_s": F.tolist(), "composed_s": C.tolist(),
               "fused_median_s": float(np.median(F)), "composed_median_s": float(np.median(C)),
               "diff_median_s": float(np.median(d)), "diff_min_s": float(d.min()), "diff_max_s": float(d.max()),
               "diff_mad_s": float(np.median(np.abs(d - np.median(d))))}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fp:
                json.dump(results, fp, indent=1)


if __name__ == "__main__":
    main()
