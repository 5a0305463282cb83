"""Causal-discrimination search over attribute sets: rigorous per-(base row, set) bits on the device,
exact resolution of what fp32 cannot decide on the host, Themis's sequential statistic per set.

``causal_search`` answers which attributes, and which small sets of attributes, a model's decisions
causally depend on (``ops/causal.py`` has the definitions, docs/DESIGN.md 5h the argument).  Levels
run by set size; one device pass per level gives a byte per (base row, set); the bytes equal to 1
(possible, not certain) are decided with ``exact.exact_signs`` on the few altered rows whose bounds
straddle 0.  The exact bits, and with them ``used``, ``rate`` and the minimal discriminatory sets, are
functions of (network, value lists, base table, settings) only: the same integers on CPU and GPU.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import causal as CS
from ..ops.audit import integral_rows
from ..ops.backend import Backend
from . import exact

TESTED, IMPLIED, TOO_MANY = "tested", "implied", "too-many-assignments"
_RESOLVE_ROWS = 1 << 16   # altered rows per re-evaluation chunk of the resolver


@dataclass
class SetResult:
    dims: Tuple[int, ...]
    assignments: int                      # A_t
    status: str                           # tested | implied | too-many-assignments
    flips_all: int = 0                    # exact flips over all S base rows
    used: int = 0                         # samples the stopping rule used
    flips: int = 0                        # exact flips within the first ``used``
    rate: float = 0.0
    half_width: float = 0.0
    discriminatory: bool = False
    pair: Optional[Tuple[Tuple[int, ...], Tuple[int, ...]]] = None   # first flipped row, lowest flipping assignment

    @property
    def size(self) -> int:
        return len(self.dims)


@dataclass
class CausalResult:
    sets: List[SetResult]
    minimal: List[SetResult]              # the discriminatory sets, by descending rate
    X: np.ndarray                         # [S, n] the base table
    ambiguous: int                        # (row, set) bits the rigorous bounds left to the host
    fused: bool                           # every level's bytes came from the fused kernel
    flip: dict = field(default_factory=dict)    # dims -> exact flip bits [S] bool of every tested set


def z_value(conf: float) -> float:
    from ..analysis.causal import _z

    return _z(conf)


def statistic(flip: np.ndarray, conf: float, margin: float, min_samples: int):
    """Themis's rule over exact flip bits in sample order: (used, flips within used, rate,
    half-width).  ``rate_k = c_k / k``; ``err_k = 0`` when the rate is 0 or 1, else
    ``z(conf) sqrt(rate_k (1 - rate_k) / k)``; ``used`` is the first ``k >= min_samples`` with
    ``err_k < margin``, else S; the rate is 0 when ``used < min_samples``."""
    flip = np.asarray(flip, dtype=bool)
    S = int(flip.shape[0])
    if S == 0:
        return 0, 0, 0.0, 0.0
    counts = np.cumsum(flip)
    k = np.arange(1, S + 1)
    rate = counts / k
    err = np.where((rate == 0) | (rate == 1), 0.0, z_value(conf) * np.sqrt(rate * (1 - rate) / k))
    stop = (k >= min_samples) & (err < margin)
    used = int(np.argmax(stop)) + 1 if stop.any() else S
    c = int(counts[used - 1])
    return used, c, (float(c / used) if used >= min_samples else 0.0), float(err[used - 1])


def device_codes(be: Backend, X: np.ndarray, table: CS.SetTable):
    """(code uint8 [S, T], fused): the fused kernel when ``be.hip``, it is not switched off
    (``FAIRIFY_CAUSAL_FUSED=0``) and it covers the shape, otherwise the reference / composed path."""
    Xt = torch.from_numpy(X).to(be.device)
    out = None
    if be.hip:
        from ..ops import hip

        if hip.causal_fused():
            out = hip.causal_codes(be, Xt.to(torch.float32), table)
    fused = out is not None
    if out is None:
        out = CS.causal_codes_ref(be, Xt, table)
    return np.ascontiguousarray(out.cpu().numpy()), fused


def _altered(X: np.ndarray, dims: Sequence[int], combos: np.ndarray):
    """(Z [m, A, n], cand [m, A]): every assignment applied to every row, and whether it differs from
    the row's own values."""
    d = list(dims)
    Z = np.repeat(X[:, None, :], combos.shape[0], axis=1)
    Z[:, :, d] = combos[None]
    return Z, (combos[None] != X[:, d][:, None, :]).any(axis=2)


def resolve_set(be: Backend, X: np.ndarray, rows: np.ndarray, table: CS.SetTable, t: int) -> np.ndarray:
    """Exact flip bits of base rows ``rows`` under set ``t``: the rows' assignments are re-evaluated
    with ``be.point_bounds``; those whose bounds already decide the comparison are kept out, the others
    (and the base row, if its own bounds straddle 0) are decided with ``exact.exact_signs``."""
    dims = table.set(t)
    combos = table.assignments(t)
    A, n = combos.shape[0], X.shape[1]
    out = np.zeros(len(rows), dtype=bool)
    step = max(1, _RESOLVE_ROWS // A)
    for s0 in range(0, len(rows), step):
        Xc = X[rows[s0:s0 + step]]
        m = len(Xc)
        Z, cand = _altered(Xc, dims, combos)
        pts = torch.from_numpy(np.concatenate([Xc, Z.reshape(-1, n)])).to(be.device, torch.float32)
        lb, ub = (b.float().cpu().numpy() for b in be.point_bounds(pts))
        lo, up, lp, upp = lb[:m, None], ub[:m, None], lb[m:].reshape(m, A), ub[m:].reshape(m, A)
        cert, poss = CS.bits(lo, up, lp, upp)
        hit = (cert & cand).any(axis=1)
        open_ = poss & ~cert & cand & ~hit[:, None]
        r, a = np.nonzero(open_)
        if r.size:
            base_label = np.zeros(m, dtype=bool)
            decided = lb[:m] > 0
            straddle = (lb[:m] <= 0) & (ub[:m] > 0)
            base_label[decided] = True
            need = np.nonzero(straddle)[0]
            base_label[need] = exact.exact_signs(be.mlp, Xc[need]) > 0
            # an altered row whose own bounds decide its label needs no exact arithmetic either
            alt_lo, alt_up = lp[r, a], upp[r, a]
            alt_label = alt_lo > 0
            ex = np.nonzero((alt_lo <= 0) & (alt_up > 0))[0]
            alt_label[ex] = exact.exact_signs(be.mlp, Z[r[ex], a[ex]]) > 0
            np.logical_or.at(hit, r, alt_label != base_label[r])
        out[s0:s0 + m] = hit
    return out


def exact_pair(mlp, x: np.ndarray, dims: Sequence[int], combos: np.ndarray):
    """The lowest assignment that exactly flips the label of ``x``, as the pair (x, x')."""
    Z, cand = _altered(x[None], dims, combos)
    lab = exact.exact_signs(mlp, np.concatenate([x[None], Z[0]])) > 0
    hits = np.nonzero(cand[0] & (lab[1:] != lab[0]))[0]
    if not hits.size:
        raise ValueError("causal: no flipping assignment for this row")
    return tuple(int(v) for v in x), tuple(int(v) for v in Z[0, hits[0]])


def causal_search(be: Backend, value_lists, base, max_size: int = 2, max_assignments: int = CS.MAX_ASSIGNMENTS,
                  threshold: float = 0.15, conf: float = 0.99, margin: float = 0.01, min_samples: int = 100,
                  resolve: bool = True, sets=None) -> CausalResult:
    """Search the attribute sets of size 1 .. ``max_size`` (at most 4) for causal discrimination.

    ``base``: the base table [S, n] (integral), or ``(S, seed)`` for ``ops/causal.draw_base``; one
    table is shared by every set.  Levels run by size; a set that contains an already discriminatory
    set is not tested (``implied``), nor is one with more than ``max_assignments`` assignments
    (``too-many-assignments``).  ``sets``: test only these sets (any order; still by level, up to the
    largest given).  Without ``resolve`` the flip bits are the certain ones only (a lower bound)."""
    n = be.n0
    lists = CS.check_value_lists(n, value_lists)
    if not 1 <= int(max_size) <= CS.MAX_DIMS:
        raise ValueError(f"causal: max_size {max_size} outside 1..{CS.MAX_DIMS}")
    if isinstance(base, tuple) and len(base) == 2 and np.ndim(base[0]) == 0:
        X = CS.draw_base(lists, int(base[0]), int(base[1]))
    else:
        X = integral_rows(base)
    if X.shape[1] != n:
        raise ValueError(f"causal: rows have {X.shape[1]} columns, the network {n} inputs")
    S = X.shape[0]
    wanted = None if sets is None else [tuple(int(d) for d in s) for s in sets]
    results: List[SetResult] = []
    found: List[frozenset] = []
    flips = {}
    ambiguous, fused_all, launched = 0, True, False
    if wanted is not None:
        CS.table_of(lists, wanted)                                           # raises on a malformed set
        max_size = max((len(s) for s in wanted), default=0)
    for size in range(1, int(max_size) + 1):
        cands = [s for s in wanted if len(s) == size] if wanted is not None else \
            list(itertools.combinations(range(n), size))
        level = []
        for s in cands:
            r = SetResult(dims=s, assignments=CS.assignments_of(lists, s), status=TESTED)
            if any(f.issubset(s) for f in found):
                r.status = IMPLIED
            elif r.assignments > max_assignments:
                r.status = TOO_MANY
            else:
                level.append(r)
            results.append(r)
        if not level or not S:
            continue
        table = CS.table_of(lists, [r.dims for r in level])
        code, fused = device_codes(be, X, table)
        launched, fused_all = True, fused_all and fused
        for t, r in enumerate(level):
            flip = (code[:, t] & CS.CERT) != 0
            amb = np.nonzero(code[:, t] == CS.POSS)[0]
            ambiguous += int(amb.size)
            if resolve and amb.size:
                flip[amb] = resolve_set(be, X, amb, table, t)
            flips[r.dims] = flip
            r.flips_all = int(flip.sum())
            r.used, r.flips, r.rate, r.half_width = statistic(flip, conf, margin, min_samples)
            r.discriminatory = bool(r.rate > threshold)
            if r.discriminatory:
                first = int(np.nonzero(flip[:r.used])[0][0])
                if resolve:
                    r.pair = exact_pair(be.mlp, X[first], r.dims, table.assignments(t))
        found += [frozenset(r.dims) for r in level if r.discriminatory]
    minimal = sorted((r for r in results if r.discriminatory), key=lambda r: (-r.rate, r.dims))
    return CausalResult(sets=results, minimal=minimal, X=X, ambiguous=ambiguous, fused=launched and fused_all,
                        flip=flips)
