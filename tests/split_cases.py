"""Shared inputs of the BaB level tests (tests/test_split_cpu.py, tests/test_split_level_gpu.py): a case
builder (queries, node boxes, synthetic certificates, per-partition state) and a plain numpy oracle of one
level -- the split step and the level end -- written with loops, one node at a time, from the rules in
the header comment of csrc/bab.hip.  Nothing here knows about waves, workgroups or atomics.

All coordinates are integers far below 2^23, so float32 evaluates every rule exactly and the tests
compare with ==.

Preconditions of a level (the certificate and the runtime guarantee them; the builders keep them, and
:func:`check_preconditions` asserts them):
  * a dim with lo == hi has score -1 on the x side, a dim with plo == phi has score -1 on the x' side:
    the split step checks the feasibility of a child for relaxed queries only;
  * PA dims are never split (score -1 on both sides); the x' side of a shared dim has score -1 (every x'
    score of a query that is not relaxed);
  * the x' box of a shared dim equals its x box.
"""
import itertools
from types import SimpleNamespace

import numpy as np

ST_UNKNOWN, ST_SAT, ST_UNSAT, ST_RUNNING, ST_STOPPING = 0, 1, 2, 3, 4
MAX_SPLIT = 6
F = np.float32


# ------------------------------------------------------------------------------------------- builder
def query(n0, pa, pa_max, ra=(), tau=0, npairs=None):
    """A query on n0 dims: PA dims ``pa`` ranging over 0..pa_max[k] (every assignment a row of
    ``values``, every ordered pair of different assignments a row of ``pairs``), relaxed dims ``ra``
    with |x_r - x'_r| <= tau.  Relaxed queries test both orientations of a pair."""
    rows = list(itertools.product(*[range(v + 1) for v in pa_max]))      # no PA dim: one empty assignment
    values = np.array(rows, np.int64).reshape(len(rows), len(pa))
    V = len(values)
    pairs = np.array([(i, j) for i in range(V) for j in range(V) if i != j], np.int64).reshape(-1, 2)
    if npairs is not None:
        pairs = pairs[:npairs]
    shared = np.ones(n0, np.uint8)
    shared[list(ra)] = 0
    return SimpleNamespace(n0=n0, pa=tuple(pa), pa_max=tuple(pa_max), ra=tuple(ra), tau=int(tau), relaxed=bool(ra),
                           shared=shared, values=values, pairs=pairs, V=V, Pp=len(pairs), norient=2 if ra else 1)


def random_boxes(q, Nn, rng, wmax=3, span=8, tight=0.5):
    """Integer node boxes: lo in [-span, span], widths 0..wmax; PA dims hold their whole range.  Relaxed:
    the x' box equals the x box on the shared dims and is, on the RA dims, the x box widened by tau and
    then (with probability ``tight`` per side) cut back by up to 2 tau + 2 -- so the coupling bites, some
    children come out empty and a few nodes hold no coupled pair at all."""
    n0 = q.n0
    lo = rng.integers(-span, span + 1, (Nn, n0)).astype(F)
    hi = lo + rng.integers(0, wmax + 1, (Nn, n0)).astype(F)
    for k, d in enumerate(q.pa):
        lo[:, d], hi[:, d] = 0, q.pa_max[k]
    plo, phi = lo.copy(), hi.copy()
    for d in q.ra:
        cut_l = np.where(rng.random(Nn) < tight, rng.integers(0, 2 * q.tau + 3, Nn), 0)
        cut_h = np.where(rng.random(Nn) < tight, rng.integers(0, 2 * q.tau + 3, Nn), 0)
        plo[:, d] = lo[:, d] - q.tau + cut_l
        phi[:, d] = np.maximum(hi[:, d] + q.tau - cut_h, plo[:, d])
    return lo, hi, plo.astype(F), phi.astype(F)


SCORE_VALUES = (0.25, 0.5, 1.0, 1.0, 2.0, 2.0, 3.0, 7.5)    # few values: ties are the rule


def random_scores(q, lo, hi, plo, phi, rng, odd=0.15):
    """Split scores [Nn, 2 n0] from a few values (many ties); a fraction ``odd`` of the entries each are
    NaN, exactly -0.5 and -1.  The preconditions are applied last."""
    Nn, n0 = lo.shape
    sc = rng.choice(np.array(SCORE_VALUES, F), (Nn, 2 * n0)).astype(F)
    u = rng.random((Nn, 2 * n0))
    sc[u < odd] = np.nan
    sc[(u >= odd) & (u < 2 * odd)] = -0.5
    sc[(u >= 2 * odd) & (u < 3 * odd)] = -1.0
    return fix_scores(q, sc, lo, hi, plo, phi)


def fix_scores(q, sc, lo, hi, plo, phi):
    """``sc`` with the preconditions enforced (score -1 where a dim must not be split)."""
    n0 = q.n0
    sc = sc.copy()
    sc[:, :n0][lo == hi] = -1.0
    sc[:, n0:][plo == phi] = -1.0
    sc[:, n0:][:, q.shared.astype(bool)] = -1.0
    for d in q.pa:
        sc[:, d] = sc[:, n0 + d] = -1.0
    return sc


def runs_to_part(runs):
    """[(partition, length), ...] -> part [Nn]."""
    return np.concatenate([np.full(n, p, np.int32) for p, n in runs]) if runs else np.zeros(0, np.int32)


def make_level(q, part, P, seed, *, open_frac=0.5, leaf_frac=0.2, wmax=3, span=8, status=None, w=None,
               nodes_start=None, budget=1 << 20, budget2=1 << 21, escalate=False, m=6, target=256, cap=None,
               cand_cap=None, boxes=None, odd=0.15):
    """One level's inputs around the node -> partition map ``part`` [Nn]: random boxes (or ``boxes`` =
    (lo, hi, plo, phi)), synthetic certificates with values from {-1, 0, 1} (exact zeros: the tests are
    strict), random open / leaf flags, and per-partition state.  ``status`` [P] defaults to mostly
    RUNNING with some partitions of every other status; ``w`` [P] is each partition's node count of the
    level (nodes_start - prev_start)."""
    rng = np.random.default_rng(seed)
    part = np.ascontiguousarray(part, np.int32)
    Nn, n0, V = len(part), q.n0, q.V
    lo, hi, plo, phi = boxes if boxes is not None else random_boxes(q, Nn, rng, wmax, span)
    lo, hi, plo, phi = (np.array(a, F).reshape(Nn, n0) for a in (lo, hi, plo, phi))
    leaf = (rng.random(Nn) < leaf_frac).astype(np.uint8)
    if boxes is None:
        for a, b in ((hi, lo), (plo, lo), (phi, lo)):      # a leaf is one lattice point off the PA dims
            keep = a[:, list(q.pa)].copy()
            a[leaf == 1] = b[leaf == 1]
            a[:, list(q.pa)] = keep
    sgn = np.array([-1.0, 0.0, 1.0], F)
    c = SimpleNamespace(
        q=q, Nn=Nn, P=P, xlo=lo, xhi=hi, xplo=plo, xphi=phi, part=part,
        open=(rng.random(Nn) < open_frac).astype(np.uint8), leaf=leaf,
        scores=random_scores(q, lo, hi, plo, phi, rng, odd),
        cand_x=rng.integers(-9, 10, (Nn, n0)).astype(F), cand_xp=rng.integers(-9, 10, (Nn, n0)).astype(F),
        pe_lb=rng.choice(sgn, 2 * Nn), pe_ub=rng.choice(sgn, 2 * Nn),
        olb=rng.choice(sgn, Nn * V), oub=rng.choice(sgn, Nn * V), olbp=rng.choice(sgn, Nn * V),
        oubp=rng.choice(sgn, Nn * V),
        budget=int(budget), budget2=int(budget2), m=int(m), target=int(target))
    if status is None:
        status = np.where(rng.random(P) < 0.7, ST_RUNNING, rng.integers(0, 5, P))
    c.status = np.array(status, np.int8).reshape(P)
    w = np.array(rng.integers(1, 9, P) if w is None else w, np.int32).reshape(P)
    c.nodes_start = np.array(rng.integers(0, 50, P) if nodes_start is None else nodes_start, np.int32).reshape(P)
    c.prev_start = (c.nodes_start - w).astype(np.int32)
    c.part_nodes = (c.nodes_start + rng.integers(0, 5, P)).astype(np.int32)   # earlier sub-batches counted already
    c.lvl_open = rng.integers(0, 3, P).astype(np.int32)
    c.pbudget = np.full(P, budget, np.int32) if escalate else None
    c.prob = np.zeros(P, np.uint8) if escalate else None
    o = split_oracle(c)
    c.cap = int(o.n_children + 7 if cap is None else cap)
    c.cand_cap = int(o.n_cands + 3 if cand_cap is None else cand_cap)
    check_preconditions(c)
    return c


def check_preconditions(c):
    q, n0 = c.q, c.q.n0
    sc = c.scores
    pick = sc > -0.5                                   # NaN compares false
    assert not np.any(pick[:, :n0] & (c.xlo == c.xhi)), "x score on a dim of width 0"
    assert not np.any(pick[:, n0:] & (c.xplo == c.xphi)), "x' score on a dim of width 0"
    assert not np.any(pick[:, n0:][:, q.shared.astype(bool)]), "x' score on a shared dim"
    assert not np.any(pick[:, list(q.pa)]) and not np.any(pick[:, [n0 + d for d in q.pa]]), "score on a PA dim"
    sh = q.shared.astype(bool)
    assert np.array_equal(c.xplo[:, sh], c.xlo[:, sh]) and np.array_equal(c.xphi[:, sh], c.xhi[:, sh])
    for a in (c.xlo, c.xhi, c.xplo, c.xphi, c.cand_x, c.cand_xp):
        assert np.all(a == np.round(a)) and np.all(np.abs(a) < 2 ** 23)
    assert np.all(c.xlo <= c.xhi) and np.all(c.xplo <= c.xphi)
    assert c.Nn == 0 or (c.part.min() >= 0 and c.part.max() < c.P)


def sub_level(c, a, b):
    """Nodes a..b-1 of the level as a sub-batch (same per-partition state objects)."""
    s = SimpleNamespace(**vars(c))
    V = c.q.V
    s.Nn = b - a
    for k in ("xlo", "xhi", "xplo", "xphi", "part", "open", "leaf", "scores", "cand_x", "cand_xp"):
        setattr(s, k, getattr(c, k)[a:b])
    for k in ("pe_lb", "pe_ub"):
        v = getattr(c, k)
        setattr(s, k, np.concatenate([v[a:b], v[c.Nn + a:c.Nn + b]]))
    for k in ("olb", "oub", "olbp", "oubp"):
        setattr(s, k, getattr(c, k)[a * V:b * V])
    return s


# -------------------------------------------------------------------------------------------- oracle
def mreq_of(w, m, target):
    """Split count of a partition with w nodes in the level: the largest m' <= min(m, 6) with
    w * 2^m' <= target, at least 1."""
    best = 1
    for mm in range(1, min(int(m), MAX_SPLIT) + 1):
        if int(w) * 2 ** mm <= int(target):
            best = mm
    return best


def pick_dims(row, mreq):
    """The top-mreq scores above -0.5 of one node's 2 n0 scores, best first; NaN is never picked, ties go
    to the lower index."""
    picked = []
    for _ in range(mreq):
        best = None
        for i, s in enumerate(row):
            if i in picked or not (s > F(-0.5)):
                continue
            if best is None or s > row[best]:
                best = i
        if best is None:
            break
        picked.append(best)
    return picked


def child_box(q, lo, hi, plo, phi, dims, c):
    """Child c of the node (lo, hi, plo, phi) split along ``dims``: bit j of c set = the upper half along
    dims[j] (index d: x side of dim d, n0 + d: x' side), halves at mid = floor((lo + hi) / 2) of the
    parent; splitting the x side of a shared dim of a relaxed query moves x' with it; then the
    |x_r - x'_r| <= tau tightening of the RA dims.  -> (lo, hi, plo, phi, feasible); a query that is not
    relaxed has x' = x and every child feasible."""
    n0 = q.n0
    L, H, PL, PH = (np.array(a, F) for a in (lo, hi, plo, phi))
    for j, dd in enumerate(dims):
        up = (c >> j) & 1
        if dd < n0:
            d = dd
            mid = np.floor(F(0.5) * (F(lo[d]) + F(hi[d])))
            if up:
                L[d] = mid + F(1)
            else:
                H[d] = mid
            if q.relaxed and q.shared[d]:
                PL[d], PH[d] = L[d], H[d]
        else:
            d = dd - n0
            mid = np.floor(F(0.5) * (F(plo[d]) + F(phi[d])))
            if up:
                PL[d] = mid + F(1)
            else:
                PH[d] = mid
    if not q.relaxed:
        return L, H, L.copy(), H.copy(), True
    tau = F(q.tau)
    for d in q.ra:
        PL[d] = max(PL[d], L[d] - tau)
        PH[d] = min(PH[d], H[d] + tau)
        L[d] = max(L[d], PL[d] - tau)
        H[d] = min(H[d], PH[d] + tau)
    return L, H, PL, PH, bool(np.all(L <= H) and np.all(PL <= PH))


def leaf_records(c, n):
    """The candidate records of leaf n: one per possible (orientation, pair), in t = o * Pp + pair
    order -- orientation 0: olb[n, vi] < 0 < oubp[n, vj]; orientation 1: oub[n, vi] > 0 > olbp[n, vj]
    (strict) -- the node's point with the pair's PA values on x and x'."""
    q, V = c.q, c.q.V
    recs = []
    for t in range(q.norient * q.Pp):
        o, pr = divmod(t, q.Pp)
        vi, vj = int(q.pairs[pr, 0]), int(q.pairs[pr, 1])
        if o == 0:
            poss = c.olb[n * V + vi] < 0 and c.oubp[n * V + vj] > 0
        else:
            poss = c.oub[n * V + vi] > 0 and c.olbp[n * V + vj] < 0
        if not poss:
            continue
        x = c.xlo[n].copy()
        xp = (c.xplo[n] if q.relaxed else c.xlo[n]).copy()
        for k, d in enumerate(q.pa):
            x[d] = q.values[vi, k]
            xp[d] = q.values[vj, k]
        recs.append(np.concatenate([x, xp, [c.part[n]]]).astype(np.float64))
    return recs


def split_oracle(c):
    """One split launch over the nodes of ``c`` with unbounded pool and candidate buffer.

    -> children[n]: the node's feasible children (part, lo, hi, plo, phi) in child order; cands[n]: its
    candidate records (x, x', partition) as float64 rows; is_leaf[n] (of the active nodes); dims[n] and
    fmask[n]: the picked split dims and the feasible children as a bit mask; status,
    part_nodes, lvl_open, prob after the launch; n_children, n_cands: the level counters' increments."""
    q, n0 = c.q, c.q.n0
    status, part_nodes, lvl_open = c.status.copy(), c.part_nodes.copy(), c.lvl_open.copy()
    prob = None if c.prob is None else c.prob.copy()
    children = [[] for _ in range(c.Nn)]
    cands = [[] for _ in range(c.Nn)]
    is_leaf = np.zeros(c.Nn, bool)
    dims_of = [[] for _ in range(c.Nn)]          # the picked dims and, bit ch, the feasible children
    fmask = [0] * c.Nn
    for n in np.nonzero(c.open)[0]:
        p = int(c.part[n])
        if c.status[p] not in (ST_RUNNING, ST_STOPPING):      # the status at the start of the launch
            continue
        if c.leaf[n]:
            is_leaf[n] = True
            cands[n] = leaf_records(c, n)
            continue
        lvl_open[p] += 1                                       # open inner node, whether it splits or not
        lbx, ubx, lbp, ubp = c.pe_lb[n], c.pe_ub[n], c.pe_lb[c.Nn + n], c.pe_ub[c.Nn + n]
        if (lbx < 0 and ubp > 0) or (ubx > 0 and lbp < 0):
            cands[n] = [np.concatenate([c.cand_x[n], c.cand_xp[n], [p]]).astype(np.float64)]
        dims = pick_dims(c.scores[n], mreq_of(int(c.nodes_start[p]) - int(c.prev_start[p]), c.m, c.target))
        dims_of[n] = dims
        if not dims:
            continue
        bud = int(c.budget if c.pbudget is None else c.pbudget[p])
        if c.nodes_start[p] >= bud:
            if prob is not None and bud < c.budget2:
                prob[p] = 1                                    # on probation: children are made
            else:
                status[p] = ST_STOPPING
                continue
        for ch in range(1 << len(dims)):
            L, H, PL, PH, ok = child_box(q, c.xlo[n], c.xhi[n], c.xplo[n], c.xphi[n], dims, ch)
            if ok:
                children[n].append((p, L, H, PL, PH))
                fmask[n] |= 1 << ch
        part_nodes[p] += len(children[n])
    return SimpleNamespace(children=children, cands=cands, is_leaf=is_leaf, dims=dims_of, fmask=fmask, status=status,
                           part_nodes=part_nodes,
                           lvl_open=lvl_open, prob=prob, n_children=sum(len(k) for k in children),
                           n_cands=sum(len(k) for k in cands))


def child_row(q, ch):
    """(part, lo, hi, plo, phi) -> one float64 row [part | lo | hi (| plo | phi when relaxed)]."""
    p, L, H, PL, PH = ch
    cols = [[p], L, H] + ([PL, PH] if q.relaxed else [])
    return np.concatenate(cols).astype(np.float64)


def in_order(c, o, cap=None, cand_cap=None):
    """What the buffers hold when the nodes reserve their slots in node order (one workgroup), with the
    capacities applied: a node whose children do not all fit below ``cap`` stops its partition and fills
    its slots below the capacity with copies of itself; a leaf record at or past ``cand_cap`` stops the
    partition, an inner node's candidate there is dropped silently.
    -> (pool rows [min(n_children, cap), ...], candidate rows, status)."""
    q = c.q
    cap = c.cap if cap is None else cap
    cand_cap = c.cand_cap if cand_cap is None else cand_cap
    status = o.status.copy()
    rows, recs = [], []
    off = slot = 0
    for n in range(c.Nn):
        k = len(o.children[n])
        if k and off + k > cap:
            p = int(c.part[n])
            status[p] = ST_STOPPING
            parent = (p, c.xlo[n], c.xhi[n], c.xplo[n], c.xphi[n])
            rows += [child_row(q, parent)] * max(0, cap - off)
        else:
            rows += [child_row(q, ch) for ch in o.children[n]]
        off += k
        for r in o.cands[n]:
            if slot < cand_cap:
                recs.append(r)
            elif o.is_leaf[n]:
                status[int(c.part[n])] = ST_STOPPING
            slot += 1
    width = 1 + (4 if q.relaxed else 2) * q.n0
    return (np.array(rows, np.float64).reshape(-1, width), np.array(recs, np.float64).reshape(-1, 2 * q.n0 + 1),
            status)


def settle_oracle(s):
    """Level end on the per-partition state ``s`` (status, lvl_open, part_open, part_nodes, nodes_start,
    prev_start, pbudget / prob or None, budget2, max_open, esc_budget, esc_open, counters_cur): a
    STOPPING partition ends UNKNOWN with part_open = its open inner nodes of the level; a RUNNING
    partition on probation continues with the next budget of budget -> esc_budget[0] -> ... -> budget2
    iff its open nodes are at most max_open (first step) / esc_open[k - 1] (step k, after k steps
    taken), else it ends UNKNOWN the same way; then the flags and the level's open count are cleared and
    the budget references move on.  -> the new state with host_counts and counters_next."""
    r = SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(s).items()})
    for p in range(len(s.status)):
        if s.status[p] == ST_STOPPING:
            r.status[p] = ST_UNKNOWN
            r.part_open[p] = s.lvl_open[p]
        elif s.prob is not None and s.prob[p] and s.status[p] == ST_RUNNING:
            taken = sum(1 for b in s.esc_budget if b <= s.pbudget[p])
            limit = s.max_open if taken == 0 else s.esc_open[taken - 1]
            if s.lvl_open[p] <= limit:
                r.pbudget[p] = s.esc_budget[taken] if taken < len(s.esc_budget) else s.budget2
            else:
                r.status[p] = ST_UNKNOWN
                r.part_open[p] = s.lvl_open[p]
        if s.prob is not None:
            r.prob[p] = 0
        r.lvl_open[p] = 0
        r.prev_start[p] = s.nodes_start[p]
        r.nodes_start[p] = s.part_nodes[p]
    r.host_counts = np.array(s.counters_cur, np.int32)
    r.counters_next = np.zeros(2, np.int32)
    return r
