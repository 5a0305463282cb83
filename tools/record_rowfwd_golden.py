#!/usr/bin/env python
"""Record the raw outputs of the six rigorous row-forward kernels (``hip.rate_counts``,
``hip.count_enum``, ``hip.gap_enum``, ``hip.audit_masks``, ``hip.neighbour_masks``,
``hip.causal_codes``) as the golden file of ``tests/test_rowfwd_golden_gpu.py``, which compares a
later build against them bitwise.

Inputs come from the builders of ``tests/*_cases.py`` (``cases()`` below, shared with the test);
outputs are stored in full.  Every case is run twice and must repeat bitwise before it is recorded.

    python tools/record_rowfwd_golden.py --out tests/golden/rowfwd_parent.npz
"""
from __future__ import annotations

import argparse
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FILE = "rowfwd_parent.npz"
KERNELS = ("rate", "count_enum", "gap_enum", "audit", "neighbours", "causal")
# net -> seed k: one per TM bucket (1, 2, 4, 7, 10 tiles), three layers (both HA / HB parities) and
# the zero-bias net, which has ambiguous bits
NETS = {"8x6": 5, "20x6": 5, "50x6": 3, "70x6": 5, "150x6": 2, "17x9x4": 2, "5x5": 5}
# every query kind on the 1- and 2-tile nets (and the three-layer one), PA-only and relaxed elsewhere
ALL_KINDS = ("pa", "relaxed", "two_pa", "three_valued")
KINDS = {n: ALL_KINDS if n in ("8x6", "20x6", "17x9x4") else ("pa", "relaxed") for n in NETS}
ROWS = (17, 65)              # one 64-row pass with a ragged wave, and two passes
SAMPLES = 70                 # two 64-profile passes
LEAF_VOLUMES = (15, 17, 65)  # under one wave's 16 points, just over, and over one 64-point pass


def model(name):
    import audit_cases as AC

    return AC.net(name, NETS[name])


def query(kind):
    import count_cases as cc

    return cc.query(kind)


@functools.lru_cache(maxsize=None)
def _rows(f3_low):
    import audit_cases as AC

    X = AC.rows(f3_low)[::8].copy()
    X.setflags(write=False)
    return X


def rows(kind, N):
    """N audited rows; row 3 has a PA coordinate outside the PA domain (own = -1)."""
    X = _rows(kind == "three_valued")[:N].copy()
    X[3, query(kind).pa_idx[0]] = 9
    return X


def boxes(kind):
    import count_cases as cc

    lo, hi, pids = cc.boxes(kind)
    lo, hi = lo[:3].clone(), hi[:3].clone()
    for d in query(kind).pa_idx:          # one PA table for the three boxes: the first box's PA range
        lo[:, d], hi[:, d] = lo[0, d], hi[0, d]
    return lo, hi, pids[:3].clone()


def leaves(kind):
    """Three leaves of LEAF_VOLUMES non-PA points over f0 x f1; PA dims span their domain (f3: 0..2)."""
    import torch

    q = query(kind)
    span = {2: (0, 1), 3: (0, 2), 4: (0, 6)}
    lo = torch.tensor([[1., 0., 0., 2., 3.]] * 3)
    hi = lo.clone()
    for r, (w0, w1) in enumerate(((3, 5), (17, 1), (5, 13))):
        hi[r, 0], hi[r, 1] = lo[r, 0] + w0 - 1, lo[r, 1] + w1 - 1
    for d in q.pa_idx:
        lo[:, d], hi[:, d] = span[d]
    return lo, hi


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _box_tables(q, lo, hi, dev):
    import torch

    from fairify_amd.engine.search import pa_table

    values, pairs = pa_table(q, lo.numpy().astype(np.int64), hi.numpy().astype(np.int64))
    return torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev)


def _row_inputs(q, X, dev):
    import torch

    from fairify_amd.ops import audit as A

    values, pairs = A.pa_domain_table(q)
    own = A.own_index(q, X, values)
    assert (own < 0).any() and (own >= 0).any()
    return (torch.from_numpy(X).to(dev, torch.float32), torch.from_numpy(own).to(dev),
            torch.from_numpy(values).to(dev), torch.from_numpy(pairs).to(dev))


def run_rate(be, dev, kind, split):
    from fairify_amd.ops import hip

    q = query(kind)
    lo, hi, pids = boxes(kind)
    vt, pt = _box_tables(q, lo, hi, dev)
    f, a, idx = hip.rate_counts(be, q, lo.to(dev), hi.to(dev), pids.to(dev), SAMPLES, 7, vt, pt, split=split)
    return dict(zip(("flips", "amb", "amb_idx"), _np(f, a, idx)))


def run_count_enum(be, dev, kind, blocks):
    from fairify_amd.ops import hip

    q = query(kind)
    lo, hi = leaves(kind)
    vt, pt = _box_tables(q, lo, hi, dev)
    c, a, idx = hip.count_enum(be, q, lo.to(dev), hi.to(dev), vt, pt, blocks=blocks)
    return dict(zip(("cert", "amb", "amb_idx"), _np(c, a, idx)))


def run_gap_enum(be, dev, kind, blocks):
    from fairify_amd.ops import hip

    q = query(kind)
    lo, hi = leaves(kind)
    vt, pt = _box_tables(q, lo, hi, dev)
    out = hip.gap_enum(be, q, lo.to(dev), hi.to(dev), vt, pt, blocks=blocks)
    assert out is not None, "gap_enum: shape not covered"
    return dict(zip(("leaf_lo", "leaf_hi", "arg_s", "arg_pair", "arg_e"), _np(*out)))


def run_audit(be, dev, kind, N, blocks):
    from fairify_amd.ops import hip

    q = query(kind)
    out = hip.audit_masks(be, q, *_row_inputs(q, rows(kind, N), dev), blocks=blocks)
    assert out is not None, "audit: shape not covered"
    return dict(zip(("cert", "poss", "own_sign"), _np(*out)))


def run_neighbours(be, dev, kind, N, blocks, wide):
    """``wide``: the toy domain with f0 widened to 0..20, a table of M = 42 entries in two words."""
    import neighbour_cases as NC
    from fairify_amd.ops import hip
    from fairify_amd.ops import neighbours as NB

    q = NC.wide_query(20) if wide else query(kind)
    table = NB.neighbour_table(q)
    assert table.M == 42 if wide else table.W == 1
    out = hip.neighbour_masks(be, q, *_row_inputs(q, rows(kind, N), dev), table, blocks=blocks)
    assert out is not None, "neighbours: shape not covered"
    return dict(zip(("cert", "poss"), _np(*out)))


def run_causal(be, dev, N, blocks):
    import torch

    import causal_cases as CC
    from fairify_amd.ops import causal as CS
    from fairify_amd.ops import hip

    X = torch.from_numpy(_rows(False)[:N].copy()).to(dev, torch.float32)
    out = hip.causal_codes(be, X, CS.table_of(CC.LISTS, CC.SETS), blocks=blocks)
    assert out is not None, "causal: shape not covered"
    return {"code": out.cpu().numpy()}


def cases():
    """(kernel, net, key, runner(be, dev) -> dict of arrays) for every golden case."""
    for net in NETS:
        for kind in KINDS[net]:
            for s in (1, 2):
                yield "rate", net, f"rate/{net}/{kind}/split{s}", functools.partial(run_rate, kind=kind, split=s)
            for b in (1, 3):
                yield ("count_enum", net, f"count_enum/{net}/{kind}/blocks{b}",
                       functools.partial(run_count_enum, kind=kind, blocks=b))
                yield ("gap_enum", net, f"gap_enum/{net}/{kind}/blocks{b}",
                       functools.partial(run_gap_enum, kind=kind, blocks=b))
            for N, b in ((17, 1), (65, 1), (65, 2)):
                yield ("audit", net, f"audit/{net}/{kind}/{N}/blocks{b}",
                       functools.partial(run_audit, kind=kind, N=N, blocks=b))
                yield ("neighbours", net, f"neighbours/{net}/{kind}/{N}/blocks{b}",
                       functools.partial(run_neighbours, kind=kind, N=N, blocks=b, wide=False))
        for N, b in ((17, 2), (65, 1), (65, 4)):          # (pass, word) items: 2 and 4
            yield ("neighbours", net, f"neighbours/{net}/wide/{N}/blocks{b}",
                   functools.partial(run_neighbours, kind="pa", N=N, blocks=b, wide=True))
        for N, b in ((17, 1), (65, 1), (65, 7)):
            yield "causal", net, f"causal/{net}/{N}/blocks{b}", functools.partial(run_causal, N=N, blocks=b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args()
    import torch

    import fairify_amd
    from fairify_amd.ops.backend import Backend

    print("recording the build of", os.path.dirname(os.path.abspath(fairify_amd.__file__)), flush=True)
    dev = torch.device("cuda")
    bes, store = {}, {}
    for kernel, net, key, run in cases():
        if net not in bes:
            bes[net] = Backend(model(net), dev)
            assert bes[net].hip
        a, b = run(bes[net], dev), run(bes[net], dev)
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), (key, name, "does not repeat")
            store[f"{key}/{name}"] = a[name]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **store)
    print(len(store), "arrays", os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
