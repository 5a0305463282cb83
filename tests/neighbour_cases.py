"""Shared inputs of the neighbourhood tests (tests/test_neighbours_cpu.py, tests/test_neighbours_gpu.py):
every 8th row of the audit tests' table (600 rows), the toy domain and three widened copies of it for
the word edges, the oracle's pinned counts, and the oracle itself -- plain loops over features and
values, the validity rules written out, and the audit tests' brute-force mask per materialised
neighbour; written independently of ops/neighbours.py and engine/neighbours.py."""
import functools

import numpy as np

from fairify_amd.spec import Domain, Feature, Query

import audit_cases as AC
import rate_cases as C

FULL = None

# name -> (family, k, query arguments, f3 restricted to 0..2 in the rows, M at full radius,
#          own-flagged / exposed / robust rows and flagged neighbours of the ORACLE at full radius)
CASES = {
    "8x6": ("8x6", 5, (("f2",),), False, 28, (3, 87, 510), 101),
    "20x6": ("20x6", 5, (("f2",),), False, 28, (32, 350, 218), 858),
    "5x5": ("5x5", 5, (("f2",),), False, 28, (97, 445, 58), 2496),
    "relaxed": ("17x9x4", 2, (("f2",), ("f1",), 1), False, 28, (133, 451, 16), 3125),
    "two-pa": ("17x9x4", 2, (("f2", "f4"),), False, 21, (341, 258, 1), 5739),
    "three-values": ("17x9x4", 2, (("f3",),), True, 24, (202, 395, 3), 4729),
    "three-values-5x5": ("5x5", 5, (("f3",),), True, 24, (157, 380, 63), 2803),
}
BIAS_CASES = ("8x6", "20x6", "relaxed", "two-pa", "three-values")
# ambiguous bits of the CPU reference at full radius (0 on the bias cases)
CPU_AMBIGUOUS = {"5x5": 13, "three-values-5x5": 7}
# the wider kernel instances (GPU tier): family -> (seed k, flagged neighbours of the oracle).  Seeds
# whose oracle flags something: 50x6 with k = 5 and 70x6 with k = 0 have no flagged neighbour on these rows
TILE_SEEDS = {"50x6": (0, 1896), "70x6": (5, 410), "150x6": (5, 568)}


def rows(f3_low: bool = False) -> np.ndarray:
    return AC.rows(f3_low)[::8].copy()


def case(name: str):
    """(MLP, resolved query, rows [600, 5] int64)."""
    family, k, qargs, f3_low = CASES[name][:4]
    return AC.net(family, k), C.query(*qargs), rows(f3_low)


def wide_query(f0_hi: int):
    """The toy domain with f0 widened to 0..f0_hi (PA f2): M = f0_hi + 1 + 21 at full radius."""
    feats = tuple(Feature(f.name, 0, f0_hi) if f.name == "f0" else f for f in C.DOM.features)
    return Query(pa=("f2",)).resolve(Domain("toy-wide", feats))


def oracle_entries(q, radii):
    """The candidate list [(feature, kind, value or offset)], feature by feature: ``radii`` maps a
    feature index to None (full) or an integer; features it does not name are full."""
    out = []
    for k, f in enumerate(q.domain.features):
        if k in q.pa_idx:
            continue
        r = radii.get(k, FULL)
        if r is FULL or r >= f.hi - f.lo:
            out += [(k, "abs", c) for c in range(f.lo, f.hi + 1)]
        else:
            out += [(k, "rel", o) for o in range(-r, r + 1) if o != 0]
    return out


def oracle(m, q, X, radii=None):
    """(flag bool [N, M], valid bool [N, M], delta int [N, M], own flag bool [N], feature of each
    entry [M]): plain loops, one brute-force audit of the materialised neighbours per entry."""
    radii = radii or {}
    X = np.asarray(X, dtype=np.int64)
    entries = oracle_entries(q, radii)
    N = len(X)
    flag = np.zeros((N, len(entries)), bool)
    valid = np.zeros((N, len(entries)), bool)
    delta = np.zeros((N, len(entries)), np.int64)
    for j, (k, kind, val) in enumerate(entries):
        f = q.domain.features[k]
        r = radii.get(k, FULL)
        Z = X.copy()
        for i in range(N):
            c = val if kind == "abs" else int(X[i, k]) + val
            ok = f.lo <= c <= f.hi and c != X[i, k]
            if r is not FULL and abs(c - int(X[i, k])) > r:
                ok = False
            valid[i, j] = ok
            delta[i, j] = c - int(X[i, k])
            Z[i, k] = c
        flag[:, j] = (AC.brute_masks(m, q, Z)[0] != 0) & valid[:, j]
    own = AC.brute_masks(m, q, X)[0] != 0
    return flag, valid, delta, own, np.array([e[0] for e in entries], dtype=np.int64)


def oracle_exposure(q, flag, delta, own, feat):
    """(count [N, n], nearest [N, n], class per row) from the oracle's bits, with plain loops."""
    N = flag.shape[0]
    count = np.zeros((N, q.n), np.int64)
    nearest = np.zeros((N, q.n), np.int64)
    for i in range(N):
        for j in np.nonzero(flag[i])[0]:
            k, d = int(feat[j]), int(delta[i, j])
            count[i, k] += 1
            b = int(nearest[i, k])
            if b == 0 or abs(d) < abs(b) or (abs(d) == abs(b) and d < b):
                nearest[i, k] = d
    return count, nearest


def classes(own_flag, audited, count):
    """Class name per row: 'flagged', 'exposed', 'robust', or '' for a row that is not audited."""
    out = []
    for i in range(len(own_flag)):
        out.append("" if not audited[i] else "flagged" if own_flag[i] else "exposed" if count[i].sum() else "robust")
    return np.array(out)


@functools.lru_cache(maxsize=None)
def oracle_case(name: str, radius=None):
    """Oracle of a table row at full radius, or with ``radius`` on every feature (cached)."""
    m, q, X = case(name)
    radii = {} if radius is None else {k: radius for k in range(q.n)}
    return oracle(m, q, X, radii)


@functools.lru_cache(maxsize=None)
def cpu_result(name: str, radius=None):
    """CPU-tier ``NeighbourResult`` of a table row (cached per process)."""
    from fairify_amd.engine.neighbours import audit_neighbours
    from fairify_amd.ops.backend import Backend

    m, q, X = case(name)
    return audit_neighbours(Backend(m, "cpu"), q, X, radii=radius)


def bits(words, M):
    """uint32 words [N, W] -> bool [N, M], written out."""
    words = np.asarray(words).astype(np.uint32)
    out = np.zeros((words.shape[0], M), bool)
    for j in range(M):
        out[:, j] = (words[:, j // 32] >> np.uint32(j % 32)) & np.uint32(1)
    return out


def padding_clear(words, M) -> bool:
    words = np.asarray(words).astype(np.uint32)
    W = words.shape[1]
    keep = np.zeros(W, np.uint32)
    for j in range(M):
        keep[j // 32] |= np.uint32(1 << (j % 32))
    return W == (M + 31) // 32 and not (words & ~keep[None]).any()
