"""Shared inputs of the counting branch-and-bound tests (tests/test_count_cpu.py,
tests/test_count_gpu.py): the toy domain, nets and boxes of tests/rate_cases.py, the query kinds and
a brute-force count of a box's unfair non-PA lattice points written independently of
engine/count.py."""
import functools
import itertools

import numpy as np
import torch

import rate_cases as rc
from fairify_amd.engine import exact

# nets of the exactness matrix and their brute-force unfair totals over the 24 boxes (1 914 non-PA
# points): (PA-only f2, relaxed f2 with RA f1 and tau 1)
NETS = (("8x6", 5), ("20x6", 0), ("20x6", 5), ("5x5", 5), ("8x6", 0), ("17x9x4", 0), ("17x9x4", 5), ("5x5", 0))
TOTALS = {("8x6", 5): (17, 65), ("20x6", 0): (1, 14), ("20x6", 5): (86, 164), ("5x5", 5): (416, 688),
          ("8x6", 0): (0, 0), ("17x9x4", 0): (0, 0), ("17x9x4", 5): (0, 0), ("5x5", 0): (0, 0)}
TOY_POINTS = 1914
KINDS = ("pa", "relaxed")
# the wider query kinds, on two nets
EXTRA_NETS = (("17x9x4", 2), ("5x5", 5))
EXTRA_KINDS = ("two_pa", "three_valued")
NO_BUDGET = 10 ** 6


def query(kind: str):
    if kind == "pa":
        return rc.query()
    if kind == "relaxed":
        return rc.query(ra=("f1",), tau=1)
    if kind == "two_pa":
        return rc.query(pa=("f2", "f4"))
    if kind == "three_valued":       # f3 set to 0..2 in every box (boxes())
        return rc.query(pa=("f3",))
    raise KeyError(kind)


def boxes(kind: str = "pa"):
    lo, hi, pids = rc.boxes()
    if kind == "three_valued":
        lo, hi = lo.clone(), hi.clone()
        lo[:, 3], hi[:, 3] = 0, 2
    return lo, hi, pids


def weights(q, lo, hi) -> np.ndarray:
    free = [d for d in range(lo.shape[1]) if d not in q.pa_idx]
    return np.prod((hi[:, free] - lo[:, free] + 1).numpy().astype(np.int64), axis=1)


def brute_unfair(m, q, lo, hi) -> np.ndarray:
    """Exact unfair non-PA lattice points of each box, int64 [P]: itertools.product over the non-PA
    dims, plain loops over the PA assignments, the ordered all-differ pairs and the unclipped RA
    offsets, exact_signs per row."""
    lo_np, hi_np = lo.numpy().astype(np.int64), hi.numpy().astype(np.int64)
    n = lo_np.shape[1]
    free = [d for d in range(n) if d not in q.pa_idx]
    offs = [()]
    if q.ra_idx and q.tau > 0:
        offs = list(itertools.product(range(-q.tau, q.tau + 1), repeat=len(q.ra_idx)))
    out = np.zeros(lo_np.shape[0], np.int64)
    for p in range(lo_np.shape[0]):
        pts = list(itertools.product(*[range(lo_np[p, d], hi_np[p, d] + 1) for d in free]))
        vals = list(itertools.product(*[range(lo_np[p, d], hi_np[p, d] + 1) for d in q.pa_idx]))
        rows = np.zeros((len(pts), len(vals), n), np.int64)
        rows[:, :, free] = np.asarray(pts, np.int64).reshape(len(pts), 1, len(free))
        for v, val in enumerate(vals):
            rows[:, v, list(q.pa_idx)] = val
        sx = exact.exact_signs(m, rows.reshape(-1, n)).reshape(len(pts), len(vals))
        flip = np.zeros(len(pts), bool)
        for e in offs:
            rp = rows.copy()
            for d, o in zip(q.ra_idx, e):
                rp[:, :, d] += o
            sxp = exact.exact_signs(m, rp.reshape(-1, n)).reshape(len(pts), len(vals))
            for v, val in enumerate(vals):
                for w, wal in enumerate(vals):
                    if all(a != b for a, b in zip(val, wal)):
                        flip |= sx[:, v] * sxp[:, w] < 0
        out[p] = int(flip.sum())
    return out


@functools.lru_cache(maxsize=None)
def brute(name: str, k: int, kind: str) -> np.ndarray:
    """Brute-force unfair counts [24] of family net (name, k) on the toy boxes (cached per process)."""
    lo, hi, _ = boxes(kind)
    return brute_unfair(rc.family_net(name, k), query(kind), lo, hi)


def ambiguous_box():
    """144 non-PA points, every one flips exactly under rate_cases.ambiguous_net(), fp32 decides none."""
    return torch.zeros(1, 5), torch.tensor([[3., 3., 1., 2., 2.]]), torch.arange(1)


def count(be, q, lo, hi, pids, node_budget=NO_BUDGET, leaf_points=8, **kw):
    from fairify_amd.engine.count import count_partitions

    return count_partitions(be, q, lo, hi, pids, node_budget, leaf_points, **kw)


def four(r):
    return np.stack([r.fair, r.unfair, r.open, r.nodes], axis=1)


def walk(be, q, lo, hi, leaf_points, max_levels=64):
    """The level loop written out with the ops/count.py reference pieces (no budget, nothing
    enumerated): per level the node pool with its class codes and volumes.  Returns a list of dicts
    ``lo, hi, part, code, vol`` (CPU tensors)."""
    from fairify_amd.engine.search import pa_table
    from fairify_amd.ops import count as OC

    lo_np, hi_np = lo.numpy().astype(np.int64), hi.numpy().astype(np.int64)
    values, pairs = pa_table(q, lo_np, hi_np)
    vt, pt = torch.from_numpy(values), torch.from_numpy(pairs)
    free = OC.free_dims(q)
    score = OC.split_scores(be.mlp)
    V = values.shape[0]
    plo, phi, part = lo.float().clone(), hi.float().clone(), torch.arange(lo.shape[0])
    levels = []
    while plo.shape[0] and len(levels) < max_levels:
        rlo, rhi, clo, chi = OC.node_rows(q, plo, phi, vt)
        rx = be.bounds(rlo, rhi, mode="symbolic", crown=True)
        rp = be.bounds(clo, chi, mode="symbolic", crown=True) if q.relaxed else rx
        code = OC.box_codes_ref(rx.out_lb.view(-1, V), rx.out_ub.view(-1, V), rp.out_lb.view(-1, V),
                                rp.out_ub.view(-1, V), pt)
        vol = OC.volumes(plo, phi, free)
        levels.append(dict(lo=plo, hi=phi, part=part, code=code, vol=vol))
        inner = (code == OC.OPEN) & (vol > leaf_points)
        _, plo, phi = OC.split_ref(plo[inner], phi[inner], free, score)
        part = part[inner].repeat_interleave(2)
    return levels
