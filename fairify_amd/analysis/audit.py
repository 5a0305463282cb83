"""``audit`` command: which individuals of a dataset does the model treat differently because of
their protected attribute?

``verify`` / ``measure`` speak about the input domain; this module takes a table of real rows and
decides each one with the project's guarantee (``engine/audit.py``: rigorous fp32 bounds on the
device, exact arithmetic for what fp32 cannot decide).  Per row: the exact mask of the PA
assignments some counterpart flips to, and the direction (-1: predicted negative with a positive
counterpart, +1: the reverse).  The summary counts audited and flagged rows, per own PA value and
direction, and the matrix ``M[v][v']`` of rows with own value ``v`` whose bit ``v'`` is set.

With the verdicts of a verify run a row's partition is looked up (``analysis/hybrid.py``) and rows /
flagged rows are reported per verdict class.  A flagged row *contradicts* an UNSAT verdict only if
the row lies in the grid and some set bit ``v'`` has every PA component inside that partition's PA
range -- the verify query of a partition covers the pairs inside its own PA range only, so a PA that
the partition size splits raises no false alarm.  A contradiction raises
:class:`analysis.rate.SoundnessError` with an exactly confirmed pair.
"""
from __future__ import annotations

import csv
import json
import os
from typing import Dict, Optional

import numpy as np

from .. import presets
from ..engine.audit import AuditResult, audit_rows, lowest_bit, witness, witnesses
from ..engine.neighbours import audit_neighbours, exposure
from ..models.zoo import get_model
from ..ops import audit as A
from ..ops import neighbours as NB
from ..ops.backend import Backend
from .hybrid import NOT_ATTEMPTED, V_SAT, V_UNKNOWN, V_UNSAT, VerdictTable
from .rate import SoundnessError

_NAMES = {V_SAT: "sat", V_UNSAT: "unsat", V_UNKNOWN: "unknown", NOT_ATTEMPTED: "not_attempted"}


def summarize(values: np.ndarray, res: AuditResult) -> Dict:
    """Counts of an audit (Python ints): audited / flagged rows, the rate, per own PA value ``n``,
    ``flagged`` and its split by direction, and the matrix ``M[v][v']``."""
    V = values.shape[0]
    ok = res.own >= 0
    flagged = res.flip_mask != 0
    audited = int(ok.sum())
    groups = []
    M = []
    for v in range(V):
        g = res.own == v
        fg = g & flagged
        groups.append({"value": [int(c) for c in values[v]], "n": int(g.sum()), "flagged": int(fg.sum()),
                       "flagged_negative": int((fg & (res.direction < 0)).sum()),
                       "flagged_positive": int((fg & (res.direction > 0)).sum())})
        M.append([int((((res.flip_mask[g] >> np.uint32(w)) & np.uint32(1)) != 0).sum()) for w in range(V)])
    return {"rows": int(len(res.own)), "audited": audited, "pa_out_of_domain": int((~ok).sum()),
            "flagged": int(flagged.sum()), "rate": (int(flagged.sum()) / audited) if audited else 0.0,
            "flagged_negative": int((flagged & (res.direction < 0)).sum()),
            "flagged_positive": int((flagged & (res.direction > 0)).sum()),
            "ambiguous_left": int(sum(bin(int(b)).count("1") for b in res.ambiguous_bits[res.ambiguous_bits != 0])),
            "groups": groups, "matrix": M}


def cross_check(grid, table: Optional[VerdictTable], q, mlp, X: np.ndarray, res: AuditResult, values: np.ndarray):
    """Partition and verdict of every row: (grid ids [N] (-1 outside the grid), verdict codes [N],
    per-class counts).  A flagged row of an UNSAT partition with a set bit whose PA value lies inside
    the partition's PA range raises :class:`SoundnessError` with an exactly confirmed pair."""
    ids = grid.encode(X)
    verdict = np.full(len(X), NOT_ATTEMPTED, dtype=np.int8)
    if table is not None:
        verdict[ids >= 0] = table.table[ids[ids >= 0]]
    flagged = res.flip_mask != 0
    sus = np.nonzero(flagged & (verdict == V_UNSAT) & (ids >= 0))[0]
    if sus.size:
        lo, hi = grid.decode(ids[sus])
        pa = list(q.pa_idx)
        inside = np.all((values[None] >= lo[:, None, pa]) & (values[None] <= hi[:, None, pa]), axis=2)   # [M, V]
        cover = (inside.astype(np.uint32) << np.arange(values.shape[0], dtype=np.uint32)[None]).sum(
            axis=1, dtype=np.uint32)
        bad = res.flip_mask[sus] & cover
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            x, xp = witness(mlp, q, X[sus[k]], int(lowest_bit(bad[k:k + 1])[0]))
            raise SoundnessError(int(ids[sus[k]]), x, xp)
    classes = {name: {"rows": int((verdict == code).sum()), "flagged": int(((verdict == code) & flagged).sum())}
               for code, name in _NAMES.items()}
    return ids, verdict, classes


def load_rows(pre, data: Optional[str], split: str, seed: int):
    """(rows [N, n] int64, source description).  ``data``: a CSV whose header holds the domain's
    feature names (other columns are ignored; the values are encoded integers); otherwise the
    suite's dataset (``data/tabular.load``: the real files when present, else synthetic rows)."""
    dom = pre.domain()
    if data:
        import pandas as pd

        df = pd.read_csv(data)
        missing = [c for c in dom.names if c not in df.columns]
        if missing:
            raise ValueError(f"audit: {data} lacks the domain's columns {missing}")
        return A.integral_rows(df[dom.names].to_numpy()), {"data": data, "synthetic": False}
    from ..data import tabular

    if split not in ("all", "train", "test"):
        raise ValueError(f"audit: split {split!r} is not all, train or test")
    ds = tabular.load(pre.suite, seed=seed)
    parts = {"train": [ds.X_train], "test": [ds.X_test], "all": [ds.X_train, ds.X_test]}[split]
    return A.integral_rows(np.concatenate(parts, axis=0)), {"data": ds.name, "split": split,
                                                            "synthetic": bool(ds.synthetic)}


def _fmt_values(values: np.ndarray, mask: int) -> str:
    return ";".join("/".join(str(int(c)) for c in values[v]) for v in range(values.shape[0]) if (mask >> v) & 1)


def audit_preset(preset: str, model: str, data: Optional[str] = None, split: str = "all",
                 results: Optional[str] = None, weights: str = "zoo", seed: int = 0, device: str = "cpu",
                 max_rows: Optional[int] = None, out_dir: Optional[str] = None,
                 pairs_out: Optional[str] = None, neighbours: bool = False, radius=None,
                 radius_of: Optional[Dict] = None) -> Dict:
    """Audit ``model`` on the rows of ``data`` (or of the preset's dataset) under the query of
    ``preset``; ``results``: the directory of a verify run (``<model>.csv``) for the verdict
    cross-check.  Writes ``audit.csv`` / ``audit.json`` to ``out_dir`` and, with ``pairs_out``, an
    ``.npz`` of one exactly confirmed pair (``x``, ``xp``) per flagged row, which
    ``repair --counterexamples`` reads.  Returns the summary.

    ``neighbours``: also decide every single-attribute neighbour of every row
    (``engine/neighbours.py``; ``radius``: an integer or ``'full'`` for every non-protected
    feature, ``radius_of``: per feature name) and write ``neighbours.csv`` / ``neighbours.json``;
    the summary then carries a ``"neighbours"`` entry, and ``audit.csv`` / ``audit.json`` are the
    bytes they are without it."""
    pre = presets.get(preset)
    grid = pre.grid(seed=seed)
    q = pre.resolved()
    mlp = get_model(model, weights=weights, seed=seed)
    be = Backend(mlp, device=device)
    X, src = load_rows(pre, data, split, seed)
    if max_rows is not None:
        X = X[:max_rows]
    values, _ = A.pa_domain_table(q)
    res = audit_rows(be, q, X)
    table = None
    if results:
        table = VerdictTable.from_csv(grid, os.path.join(results, f"{model}.csv"), seed=seed)
    ids, verdict, classes = cross_check(grid, table, q, mlp, X, res, values)
    out = {"preset": preset, "model": model, "seed": int(seed), "source": src,
           "pa": [q.domain.names[i] for i in q.pa_idx], "pa_values": values.tolist()}
    out.update(summarize(values, res))
    out["verdicts"] = classes
    out["checked_against_results"] = table is not None
    flagged = np.nonzero(res.flip_mask)[0]
    if pairs_out:
        x, xp = witnesses(mlp, q, X[flagged], lowest_bit(res.flip_mask[flagged]))
        os.makedirs(os.path.dirname(os.path.abspath(pairs_out)), exist_ok=True)
        np.savez(pairs_out, x=x, xp=xp)
        out["pairs_out"] = pairs_out
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        dom = q.domain
        inside = np.all((X >= dom.lo()) & (X <= dom.hi()), axis=1)
        pa_names = [dom.names[i] for i in q.pa_idx]
        with open(os.path.join(out_dir, "audit.csv"), "w", newline="") as fp:
            wr = csv.writer(fp)
            wr.writerow(["row"] + pa_names + ["audited", "in_domain", "grid_id", "verdict", "flagged", "direction",
                                              "flip_mask", "flipped_to"])
            for i in range(len(X)):
                m = int(res.flip_mask[i])
                wr.writerow([i] + [int(X[i, d]) for d in q.pa_idx] +
                            [int(res.own[i] >= 0), int(inside[i]), int(ids[i]), _NAMES[int(verdict[i])], int(m != 0),
                             int(res.direction[i]), m, _fmt_values(values, m)])
        with open(os.path.join(out_dir, "audit.json"), "w") as fp:
            json.dump(out, fp, indent=2)
    if neighbours:
        out = dict(out)
        out["neighbours"] = _neighbours(be, grid, table, q, mlp, X, res, values, radius, radius_of, out_dir)
    return out


def neighbour_cross_check(be, grid, table: Optional[VerdictTable], q, mlp, X: np.ndarray, nres, values) -> int:
    """The flagged neighbours that lie in UNSAT partitions, deduplicated, audited as rows of their own
    and passed through :func:`cross_check` (which raises :class:`SoundnessError` on a
    contradiction).  Returns how many were checked."""
    if table is None:
        return 0
    rows, js = np.nonzero(NB.unpack_bits(nres.flag, nres.table.M))
    if not rows.size:
        return 0
    t = nres.table
    Z = X[rows].copy()
    d = t.dim[js].astype(np.int64)
    at = np.arange(len(rows))
    Z[at, d] = np.where(t.abs[js] != 0, t.off[js].astype(np.int64), Z[at, d] + t.off[js])
    ids = grid.encode(Z)
    keep = ids >= 0
    keep[keep] = table.table[ids[keep]] == V_UNSAT
    Z = np.unique(Z[keep], axis=0)
    if len(Z):
        cross_check(grid, table, q, mlp, Z, audit_rows(be, q, Z), values)
    return int(len(Z))


def _neighbours(be, grid, table, q, mlp, X, res: AuditResult, values, radius, radius_of, out_dir) -> Dict:
    """The ``--neighbours`` part of :func:`audit_preset`: summary dictionary, and the two files."""
    dom = q.domain
    radii = {"*": radius}
    radii.update(radius_of or {})
    nres = audit_neighbours(be, q, X, radii=radii)
    ex = exposure(nres, X, res.flip_mask != 0)
    t = nres.table
    feats = [k for k in range(q.n) if k not in q.pa_idx]
    n_valid = 0                                                     # valid neighbours of audited rows, in chunks
    for s0 in range(0, len(X), 4096):
        sl = slice(s0, s0 + 4096)
        n_valid += int(NB.neighbour_values(X[sl], t)[1][nres.own[sl] >= 0].sum())
    checked = neighbour_cross_check(be, grid, table, q, mlp, X, nres, values)
    audited = nres.own >= 0
    cls = np.where(ex.flagged, "flagged", np.where(ex.exposed, "exposed", np.where(ex.robust, "robust", "")))
    out = {"radii": {dom.names[k]: ("full" if t.radius[k] >= NB.FULL else int(t.radius[k])) for k in feats},
           "M": t.M, "audited": int(audited.sum()), "flagged": int(ex.flagged.sum()),
           "exposed": int(ex.exposed.sum()), "robust": int(ex.robust.sum()),
           "valid_neighbours": n_valid, "flagged_neighbours": int(ex.count.sum()),
           "features": {dom.names[k]: {"rows_exposed": int((ex.exposed & (ex.count[:, k] > 0)).sum()),
                                       "flagged_neighbours": int(ex.count[:, k].sum())} for k in feats},
           "ambiguous_left": int(nres.ambiguous_left), "checked_against_results": table is not None,
           "neighbours_in_unsat_checked": checked}
    if out_dir:
        total = ex.count.sum(axis=1)
        with open(os.path.join(out_dir, "neighbours.csv"), "w", newline="") as fp:
            wr = csv.writer(fp)
            head = ["row", "audited", "flagged", "class", "flagged_neighbours"]
            for k in feats:
                head += [dom.names[k] + "_count", dom.names[k] + "_nearest"]
            wr.writerow(head)
            for i in range(len(X)):
                line = [i, int(audited[i]), int(ex.flagged[i]), cls[i], int(total[i])]
                for k in feats:
                    line += [int(ex.count[i, k]), int(ex.nearest[i, k])]
                wr.writerow(line)
        with open(os.path.join(out_dir, "neighbours.json"), "w") as fp:
            json.dump(out, fp, indent=2)
    return out
