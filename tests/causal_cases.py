"""Shared inputs of the causal-search tests (tests/test_causal_cpu.py, tests/test_causal_gpu.py): the
toy domain of tests/rate_cases.py with whole-domain value lists, its 30 attribute sets of size <= 4,
the base rows, a brute-force flip oracle written independently of ops/causal.py and engine/causal.py,
and its pinned per-set counts."""
import functools
import itertools
import math

import numpy as np

from fairify_amd.engine import exact

import audit_cases as AC
import rate_cases as C

LISTS = [list(range(f.lo, f.hi + 1)) for f in C.DOM.features]          # 7, 8, 2, 6 and 7 values
SETS = [s for k in (1, 2, 3, 4) for s in itertools.combinations(range(5), k)]     # 5 + 10 + 10 + 5
SETS3 = [s for s in SETS if len(s) <= 3]

# nets whose CPU reference leaves no point of the toy domain with l <= 0 < u (the ambiguity cap rests on it)
CLEAN_NETS = (("8x6", 5), ("20x6", 5), ("17x9x4", 2), ("70x6", 5), ("50x6", 3), ("150x6", 2))
BIAS_CASES = (("8x6", 5), ("20x6", 5), ("17x9x4", 2))
# one net per kernel instance: TM = 1, 2, 2 (three layers), 4, 7, 10
TILE_NETS = (("8x6", 5), ("20x6", 5), ("17x9x4", 2), ("50x6", 3), ("70x6", 5), ("150x6", 2))

# exact flips of the 600 base rows per set, in SETS order (the oracle below)
COUNTS = {
    ("8x6", 5): [33, 28, 3, 13, 25, 85, 50, 94, 163, 46, 91, 162, 23, 35, 72, 125, 201, 377, 142, 235, 388, 172,
                 261, 378, 127, 315, 554, 600, 514, 600],
    ("20x6", 5): [240, 66, 32, 165, 72, 459, 302, 588, 299, 92, 267, 191, 214, 98, 397, 515, 600, 600, 600, 352,
                  600, 335, 212, 600, 451, 600, 600, 600, 600, 600],
    ("17x9x4", 2): [372, 331, 56, 202, 309, 597, 422, 492, 580, 376, 420, 592, 235, 400, 470, 600, 600, 600, 533,
                    600, 600, 477, 598, 600, 552, 600, 600, 600, 600, 600],
    ("5x5", 5): [544, 305, 97, 157, 197, 600, 575, 592, 589, 384, 460, 564, 242, 316, 353, 600, 600, 600, 600,
                 600, 600, 554, 596, 597, 436, 600, 600, 600, 600, 600],
}
# (row, set) bytes the CPU reference leaves to the host on the zero-bias net, all 30 sets
AMBIGUOUS_5x5 = 2


def rows() -> np.ndarray:
    """The 600 base rows."""
    return AC.rows()[::8].copy()


def labels(m, X) -> np.ndarray:
    return exact.exact_signs(m, np.asarray(X, dtype=np.int64)) > 0


def oracle(m, X, sets=SETS, lists=LISTS) -> np.ndarray:
    """Exact flip bits bool [S, T]: plain loops over the sets and over ``itertools.product`` of the
    value lists; an assignment counts when it differs from the row's own values somewhere and the
    exact label of the altered row differs from the base row's."""
    X = np.asarray(X, dtype=np.int64)
    base = labels(m, X)
    out = np.zeros((len(X), len(sets)), dtype=bool)
    for t, s in enumerate(sets):
        for val in itertools.product(*[lists[d] for d in s]):
            Z = X.copy()
            differ = np.zeros(len(X), dtype=bool)
            for d, c in zip(s, val):
                differ |= X[:, d] != c
                Z[:, d] = c
            out[:, t] |= differ & (labels(m, Z) != base)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(family: str, k: int) -> np.ndarray:
    """Oracle bits of net (family, k) on the 600 rows, all 30 sets (cached per process)."""
    out = oracle(AC.net(family, k), rows())
    out.setflags(write=False)
    return out


def stat_oracle(flip, z: float, margin: float, min_samples: int):
    """Themis's stopping rule as a plain loop: (used, flips within used, rate)."""
    S = len(flip)
    c, used, c_used = 0, S, None
    for k in range(1, S + 1):
        c += int(flip[k - 1])
        rate = c / k
        err = 0.0 if rate in (0.0, 1.0) else z * math.sqrt(rate * (1 - rate) / k)
        if k >= min_samples and err < margin:
            used, c_used = k, c
            break
    if c_used is None:
        c_used = c
    return used, c_used, (c_used / used if used >= min_samples else 0.0)


def search_oracle(flip_of, n: int, lists, max_size: int, max_assignments: int, z: float, threshold: float,
                  margin: float, min_samples: int):
    """Level-by-level search over exact flip bits ``flip_of(set) -> bool [S]``:
    {set: status}, [discriminatory sets in discovery order]."""
    status, found = {}, []
    for size in range(1, max_size + 1):
        new = []
        for s in itertools.combinations(range(n), size):
            if any(set(f) <= set(s) for f in found):
                status[s] = "implied"
            elif math.prod(len(lists[d]) for d in s) > max_assignments:
                status[s] = "too-many-assignments"
            else:
                status[s] = "tested"
                if stat_oracle(flip_of(s), z, margin, min_samples)[2] > threshold:
                    new.append(s)
        found += new
    return status, found
