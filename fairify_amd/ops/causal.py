"""Causal-discrimination search over attribute sets (Themis): the set table, the base table and the
rigorous per-(base row, set) bits.

Definitions -- docs/DESIGN.md 5h:

* **value lists**: ``vals_k``, a sorted list of distinct integers per feature k, ``|vals_k| >= 1``;
  flat as ``vals`` (int32) with offsets ``voff`` [n + 1];
* **base rows**: ``X`` [S, n], integral;
* **attribute set** t: a strictly increasing tuple of 1 .. 4 feature indices, ``dims`` [T, 4] int32
  padded with -1.  ``A_t = prod |vals_k|`` is its number of assignments, enumerated row-major over the
  tuple, the last feature fastest; assignment a sets ``x[dims_j] := vals[voff[dims_j] + digit_j(a)]``;
* ``label(x) = [N(x) > 0]`` with the logit exact: Themis's and ``analyze``'s predicted class (not the
  strict sign product of the audit);
* ``flip(s, t)``: some assignment whose values differ from ``X[s, dims_t]`` in at least one component
  changes the label of row s.  The row's own assignment is skipped, so a set with ``A_t == 1`` flips
  nothing for a row that holds the one value; a base value absent from its list makes every assignment
  a candidate;
* with ``[l, u]`` the rigorous logit bounds of the base row and ``[l', u']`` those of an altered row
  (``Backend.point_bounds``):  **cert**: ``(l > 0 and u' <= 0) or (u <= 0 and l' > 0)`` for some
  candidate;  **poss**: ``(u > 0 and l' <= 0) or (l <= 0 and u' > 0)`` for some candidate.
  ``cert <= flip <= poss`` per (s, t);
* ``code`` [S, T] uint8: bit 0 poss, bit 1 cert -- 0, 1 or 3.  One byte per (row, set): work items
  never share an output word.

One base table is shared by all sets of a call (common random numbers, one upload); the reference
detector draws a new one per set.  This module is the reference on any backend -- on a HIP backend it
is the composed device path (``point_bounds`` fed materialised rows in chunks); the fused kernel is
``ops/hip.py:causal_codes`` (csrc/causal.hip).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Iterable, Sequence, Tuple

import numpy as np
import torch

MAX_DIMS = 4              # features per attribute set
MAX_ASSIGNMENTS = 4096    # default cap on A_t
MAX_VALUE = 2 ** 24       # |value|: exact in fp32
_REF_ROWS = 1 << 17       # materialised altered rows per chunk of the reference
POSS, CERT = 1, 2


@dataclass(frozen=True)
class SetTable:
    dims: np.ndarray      # [T, 4] int32  strictly increasing feature indices, padded with -1
    count: np.ndarray     # [T] int64     A_t
    vals: np.ndarray      # [nvals] int32 every feature's value list, flat
    voff: np.ndarray      # [n + 1] int32 feature k's list is vals[voff[k] : voff[k + 1]]

    @property
    def T(self) -> int:
        return int(self.dims.shape[0])

    @property
    def n(self) -> int:
        return int(self.voff.shape[0]) - 1

    def set(self, t: int) -> Tuple[int, ...]:
        return tuple(int(d) for d in self.dims[t] if d >= 0)

    def sets(self):
        return [self.set(t) for t in range(self.T)]

    def values(self, k: int) -> np.ndarray:
        return self.vals[self.voff[k]:self.voff[k + 1]].astype(np.int64)

    def assignments(self, t: int) -> np.ndarray:
        """[A_t, |t|] int64: the set's assignments in the kernel's order."""
        return np.array(list(itertools.product(*[self.values(k).tolist() for k in self.set(t)])), dtype=np.int64)

    def select(self, idx) -> "SetTable":
        idx = np.asarray(idx, dtype=np.int64)
        return SetTable(dims=np.ascontiguousarray(self.dims[idx]), count=self.count[idx], vals=self.vals,
                        voff=self.voff)


def check_value_lists(n: int, value_lists) -> list:
    """The lists as sorted int64 arrays; anything but n non-empty lists of distinct integers within
    +-2^24 raises ``ValueError``."""
    if len(value_lists) != n:
        raise ValueError(f"causal: {len(value_lists)} value lists for {n} features")
    out = []
    for k, v in enumerate(value_lists):
        a = np.asarray(v)
        if a.ndim != 1 or a.size < 1:
            raise ValueError(f"causal: feature {k} needs a flat list of at least one value")
        if not np.issubdtype(a.dtype, np.integer):
            f = a.astype(np.float64)
            if not (np.isfinite(f) & (f == np.rint(f))).all():
                raise ValueError(f"causal: feature {k} has a non-integral value")
            a = np.rint(f)
        a = a.astype(np.int64)
        if np.unique(a).size != a.size:
            raise ValueError(f"causal: feature {k} repeats a value")
        if np.abs(a).max() > MAX_VALUE:
            raise ValueError(f"causal: feature {k} has a value beyond +-2^24 (not exact in fp32)")
        out.append(np.sort(a))
    return out


def table_of(value_lists, sets: Iterable[Sequence[int]]) -> SetTable:
    """The table of explicitly given attribute sets, in the given order."""
    n = len(value_lists)
    lists = check_value_lists(n, value_lists)
    voff = np.zeros(n + 1, dtype=np.int64)
    voff[1:] = np.cumsum([len(v) for v in lists])
    sets = [tuple(int(d) for d in s) for s in sets]
    dims = np.full((len(sets), MAX_DIMS), -1, dtype=np.int32)
    count = np.ones(len(sets), dtype=np.int64)
    for t, s in enumerate(sets):
        if not 1 <= len(s) <= MAX_DIMS:
            raise ValueError(f"causal: set {s} has {len(s)} features, a set has 1..{MAX_DIMS}")
        if any(not 0 <= d < n for d in s) or any(b <= a for a, b in zip(s, s[1:])):
            raise ValueError(f"causal: set {s} is not a strictly increasing tuple of features 0..{n - 1}")
        dims[t, :len(s)] = s
        for d in s:
            count[t] *= len(lists[d])
    return SetTable(dims=dims, count=count, vals=np.concatenate(lists).astype(np.int32), voff=voff.astype(np.int32))


def assignments_of(value_lists, s: Sequence[int]) -> int:
    a = 1
    for d in s:
        a *= len(value_lists[d])
    return a


def set_table(n: int, value_lists, sizes=(1,), exclude=(), max_assignments: int = MAX_ASSIGNMENTS) -> SetTable:
    """Every attribute set of the given sizes over features 0 .. n - 1 (by size, then lexicographic)
    that contains no set of ``exclude`` and has at most ``max_assignments`` assignments."""
    if len(value_lists) != n:
        raise ValueError(f"causal: {len(value_lists)} value lists for {n} features")
    exclude = [frozenset(int(d) for d in e) for e in exclude]
    sets = []
    for size in sizes:
        if not 1 <= int(size) <= MAX_DIMS:
            raise ValueError(f"causal: set size {size} outside 1..{MAX_DIMS}")
        for s in itertools.combinations(range(n), int(size)):
            if any(e.issubset(s) for e in exclude) or assignments_of(value_lists, s) > max_assignments:
                continue
            sets.append(s)
    return table_of(value_lists, sets)


def draw_base(value_lists, S: int, seed: int) -> np.ndarray:
    """The base table [S, n] int64: column by column in feature order,
    ``vals_k[rng.integers(0, len(vals_k), size=S)]`` from ``np.random.default_rng(seed)`` -- the
    order of the first ``causal_discrimination`` call of a fresh ``CausalDiscriminationDetector``."""
    lists = check_value_lists(len(value_lists), value_lists)
    rng = np.random.default_rng(seed)
    X = np.zeros((int(S), len(lists)), dtype=np.int64)
    for k, v in enumerate(lists):
        X[:, k] = v[rng.integers(0, len(v), size=int(S))]
    return X


def bits(lo, up, lp, upp):
    """(cert, poss) of base bounds ``[lo, up]`` against altered bounds ``[lp, upp]`` (broadcast)."""
    cert = ((lo > 0) & (upp <= 0)) | ((up <= 0) & (lp > 0))
    poss = ((up > 0) & (lp <= 0)) | ((lo <= 0) & (upp > 0))
    return cert, poss


def causal_codes_ref(be, X: torch.Tensor, table: SetTable, sub: int = 4096) -> torch.Tensor:
    """Reference bytes of base rows ``X`` [S, n]: ``code`` uint8 [S, T] on ``X``'s device.  The altered
    rows of one set are materialised in chunks of at most ``sub`` base rows (and at most ``_REF_ROWS``
    altered rows), bounded with ``be.point_bounds`` and compared with the base rows' bounds."""
    S, n = X.shape
    if n != table.n:
        raise ValueError(f"causal: rows have {n} columns, the table {table.n} features")
    dev = X.device
    code = torch.zeros(S, table.T, dtype=torch.uint8, device=dev)
    if not S or not table.T:
        return code
    X = X.to(torch.int64)
    lo = torch.empty(S, dtype=torch.float32, device=dev)
    up = torch.empty(S, dtype=torch.float32, device=dev)
    for s0 in range(0, S, _REF_ROWS):
        l, u = be.point_bounds(X[s0:s0 + _REF_ROWS].to(torch.float32))
        lo[s0:s0 + _REF_ROWS], up[s0:s0 + _REF_ROWS] = l.float(), u.float()
    for t in range(table.T):
        d = torch.tensor(table.set(t), dtype=torch.int64, device=dev)
        combos = torch.from_numpy(table.assignments(t)).to(dev)                        # [A, k]
        A = combos.shape[0]
        rows = max(1, min(int(sub), _REF_ROWS // A))
        for s0 in range(0, S, rows):
            Xc = X[s0:s0 + rows]
            m = Xc.shape[0]
            cand = (combos[None] != Xc[:, d][:, None, :]).any(dim=2)                   # [m, A]
            Z = Xc[:, None, :].expand(m, A, n).clone()
            Z[:, :, d] = combos[None]
            lp, upp = be.point_bounds(Z.reshape(-1, n).to(torch.float32))
            ce, po = bits(lo[s0:s0 + m, None], up[s0:s0 + m, None], lp.float().view(m, A), upp.float().view(m, A))
            ce, po = (ce & cand).any(dim=1), (po & cand).any(dim=1)
            code[s0:s0 + m, t] = (ce.to(torch.uint8) * CERT) | (po.to(torch.uint8) * POSS)
    return code
