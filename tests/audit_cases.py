"""Shared inputs of the audit tests (tests/test_audit_cpu.py, tests/test_audit_gpu.py): the toy cases
of tests/rate_cases.py audited as tables of rows, the expected counts, two wider nets for the 4- and
10-tile kernel instances, and a brute-force flip mask written independently of engine/audit.py."""
import functools
import itertools

import numpy as np

from fairify_amd.engine import exact
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import reference as ref

import rate_cases as C

# name -> (family or net, k, query arguments, boxes restricted to f3 in 0..2, V, flagged, direction -1,
#          ambiguous bits of the CPU reference)
CASES = {
    "8x6": ("8x6", 5, (("f2",),), False, 2, 51, 22, 0),
    "20x6": ("20x6", 5, (("f2",),), False, 2, 212, 101, 0),
    "5x5": ("5x5", 5, (("f2",),), False, 2, 860, 443, 10),
    "relaxed": ("17x9x4", 2, (("f2",), ("f1",), 1), False, 2, 972, 565, 0),
    "two-pa": ("17x9x4", 2, (("f2", "f4"),), False, 14, 2586, 1916, 0),
    "three-values": ("17x9x4", 2, (("f3",),), True, 6, 1591, 528, 0),
    "three-values-5x5": ("5x5", 5, (("f3",),), True, 6, 1165, 315, 45),
    "ambiguous": ("ambiguous", 0, (("f2",),), False, 2, 800, 406, 800),
}
BIAS_CASES = ("8x6", "20x6", "relaxed", "two-pa", "three-values")


def net(family: str, k: int):
    if family == "ambiguous":
        return C.ambiguous_net()
    if family == "50x6":                        # four-tile kernel instance
        return random_mlp(5, [50, 6], seed=100 + k, bias_scale=0.5)
    if family == "150x6":                       # ten-tile kernel instance
        return random_mlp(5, [150, 6], seed=100 + k, bias_scale=0.5)
    return C.family_net(family, k)


def rows(f3_low: bool = False, ambiguous: bool = False) -> np.ndarray:
    """The audited rows: 200 hash samples of each of the 24 toy boxes (4 800 rows, the PA is whatever
    was sampled), or of the 4 all-ambiguous boxes (800 rows)."""
    lo, hi, pids = C.ambiguous_boxes() if ambiguous else C.boxes()
    if f3_low:
        lo[:, 3], hi[:, 3] = 0, 2
    return ref.sample_points(lo, hi, pids, C.S, C.SEED).reshape(-1, 5).numpy().astype(np.int64)


def case(name: str):
    """(MLP, resolved query, rows [N, 5] int64) of a table row."""
    family, k, qargs, f3_low = CASES[name][:4]
    return net(family, k), C.query(*qargs), rows(f3_low, family == "ambiguous")


def brute_masks(m, q, X: np.ndarray):
    """Exact flip mask and own sign of every row: plain loops over the PA assignments v' of the PA
    DOMAIN (all components differing from the row's own) and the RA offsets (unclipped),
    exact_signs per counterpart.  Rows whose PA lies outside the PA domain get 0."""
    X = np.asarray(X, dtype=np.int64)
    dom = q.domain
    vals = list(itertools.product(*[range(dom.features[d].lo, dom.features[d].hi + 1) for d in q.pa_idx]))
    offs = [()]
    if q.ra_idx and q.tau > 0:
        offs = list(itertools.product(range(-q.tau, q.tau + 1), repeat=len(q.ra_idx)))
    sx = exact.exact_signs(m, X)
    inside = np.ones(len(X), bool)
    for d in q.pa_idx:
        inside &= (X[:, d] >= dom.features[d].lo) & (X[:, d] <= dom.features[d].hi)
    mask = np.zeros(len(X), np.uint32)
    for w, val in enumerate(vals):
        differ = inside.copy()
        for d, c in zip(q.pa_idx, val):
            differ &= X[:, d] != c
        for e in offs:
            XP = X.copy()
            for d, c in zip(q.pa_idx, val):
                XP[:, d] = c
            for d, o in zip(q.ra_idx, e):
                XP[:, d] += o
            flip = differ & (sx * exact.exact_signs(m, XP) < 0)
            mask[flip] |= np.uint32(1 << w)
    return mask, sx


@functools.lru_cache(maxsize=None)
def brute(name: str):
    m, q, X = case(name)
    return brute_masks(m, q, X)


@functools.lru_cache(maxsize=None)
def cpu_audit(name: str):
    """CPU-tier ``AuditResult`` of a table row (cached per process)."""
    from fairify_amd.engine.audit import audit_rows
    from fairify_amd.ops.backend import Backend

    m, q, X = case(name)
    return audit_rows(Backend(m, "cpu"), q, X)


def popcount(a: np.ndarray) -> int:
    return int(sum(bin(int(v)).count("1") for v in np.asarray(a).reshape(-1) if v))
