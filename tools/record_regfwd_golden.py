#!/usr/bin/env python
"""Record the outputs of the register-resident forward kernels other than the simulation kernel
(``fa_point_kernel``, the fused falsifier, ``fa_agree_kernel``) as golden files for
``tests/test_regfwd_golden_gpu.py``, which compares a later build against them bitwise.

Inputs are derived from seeds (``cases()`` below, shared with the test); outputs are stored in full.
Every case is run twice and must repeat bitwise before it is recorded.

    python tools/record_regfwd_golden.py --out tests/golden
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

SHAPES = [[5, 5], [16, 8], [64, 32, 16, 8, 4], [100], [100, 100]]     # hidden widths, n0 = 13
POINTS = [1, 15, 16, 17, 701]
PART_IDS = [5, 4321, 15999]
FILES = {"point": "regfwd_point.npz", "falsify": "regfwd_falsify.npz", "agree": "regfwd_agree.npz"}


def shape_key(hidden):
    return "13_" + "_".join(map(str, hidden)) + "_1"


def model(hidden):
    from fairify_amd.models.mlp import random_mlp

    return random_mlp(13, hidden, seed=11 + len(hidden), bias_scale=0.5)


def dead_mask(rows, n_hidden, seed, on):
    g = np.random.default_rng(seed)
    m = (g.random((rows, n_hidden)) < 0.25).astype(np.uint8)
    return m if on else np.zeros_like(m)


def run_point(be, dev, hidden, R, dead_on):
    """lb, ub [R] of R integer points, optionally with a per-point dead mask."""
    import torch

    g = np.random.default_rng(1000 + R)
    x = torch.from_numpy(g.integers(-5, 40, size=(R, 13)).astype(np.float32)).to(dev)
    dead = torch.from_numpy(dead_mask(R, be.n_hidden, 2000 + R, True)).to(dev) if dead_on else None
    lb, ub = be.point_bounds(x, dead)
    return {"lb": lb.cpu().numpy(), "ub": ub.cpu().numpy()}


def _boxes(dev):
    import torch

    from fairify_amd.partition import Grid
    from fairify_amd.spec import ADULT, Query

    q = Query(("race",)).resolve(ADULT)
    ids = np.array(PART_IDS)
    lo, hi = Grid.reference(ADULT, 10).decode(ids)
    values = q.pa_values(lo[0], hi[0])
    pairs = q.pa_pairs(values)
    t = lambda a: torch.from_numpy(a).to(dev)
    return q, t(lo).float(), t(hi).float(), t(ids), t(values), t(pairs)


def run_falsify(be, dev, hidden, S):
    """Fused falsifier over S samples per partition (no dead mask: the kernel takes none)."""
    from fairify_amd.ops import hip

    q, lo, hi, pids, values, pairs = _boxes(dev)
    free = [d for d in range(13) if d not in set(q.pa_idx)]
    out = hip.falsify(be, q, lo, hi, pids, values, pairs, 77, S, 64, 4, 6, 8, 6, free, dseed=78)
    assert out is not None, "falsify: shape not supported"
    found, wx, wxp, how = out
    return {"found": found.cpu().numpy(), "wit_x": wx.cpu().numpy(), "wit_xp": wxp.cpu().numpy(),
            "how": how.cpu().numpy()}


def run_agree(be, dev, hidden, S, dead_on):
    """Pruned-acc counts over S samples per partition; the mask is all zero when dead_on is False."""
    import torch

    from fairify_amd.ops import hip

    q, lo, hi, pids, values, pairs = _boxes(dev)
    rows = torch.tensor([2, 0, 1], device=dev)
    dead = torch.from_numpy(dead_mask(3, be.n_hidden, 3000 + S, dead_on)).to(dev)
    out = hip.agree(be, rows, lo, hi, pids, dead, S, 9)
    assert out is not None, "agree: shape not supported"
    return {"agree": out.cpu().numpy()}


def cases():
    """(file, key prefix, runner(be, dev) -> dict of arrays) for every golden case."""
    for hidden in SHAPES:
        for n in POINTS:
            for dead_on in (False, True):
                k = f"{shape_key(hidden)}/{n}/{'dead' if dead_on else 'nodead'}"
                yield "point", hidden, k, (lambda be, dev, h=hidden, n=n, d=dead_on: run_point(be, dev, h, n, d))
                yield "agree", hidden, k, (lambda be, dev, h=hidden, n=n, d=dead_on: run_agree(be, dev, h, n, d))
            k = f"{shape_key(hidden)}/{n}/nodead"
            yield "falsify", hidden, k, (lambda be, dev, h=hidden, n=n: run_falsify(be, dev, h, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="repository tree whose build is recorded")
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import torch

    from fairify_amd.ops.backend import Backend

    import fairify_amd

    print("recording the build of", os.path.dirname(os.path.abspath(fairify_amd.__file__)), flush=True)
    dev = torch.device("cuda")
    bes = {}
    store = {f: {} for f in FILES}
    for kind, hidden, key, run in cases():
        if shape_key(hidden) not in bes:
            bes[shape_key(hidden)] = Backend(model(hidden), dev)
        be = bes[shape_key(hidden)]
        assert be.hip
        a, b = run(be, dev), run(be, dev)
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), (kind, key, name, "does not repeat")
            store[kind][f"{key}/{name}"] = a[name]
    os.makedirs(args.out, exist_ok=True)
    for kind, f in FILES.items():
        np.savez_compressed(os.path.join(args.out, f), **store[kind])
        print(kind, len(store[kind]), "arrays", os.path.getsize(os.path.join(args.out, f)), "bytes")


if __name__ == "__main__":
    main()
