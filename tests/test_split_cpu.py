"""The oracle of the BaB level tests (tests/split_cases.py) checked without a GPU: children tile their
parent (lattice points, or -- relaxed -- coupled lattice pairs), the split count against a table written
out by hand, the tie and NaN rules, and the budget / probation / level-end transitions on hand-written
three-partition cases."""
import itertools

import numpy as np
import pytest

import split_cases as sc
from split_cases import ST_RUNNING, ST_SAT, ST_STOPPING, ST_UNKNOWN, ST_UNSAT, F


def points(lo, hi):
    return list(itertools.product(*[range(int(a), int(b) + 1) for a, b in zip(lo, hi)]))


def inside(x, lo, hi):
    return all(a <= v <= b for v, a, b in zip(x, lo, hi))


# ------------------------------------------------------------------------------------------ tiling
@pytest.mark.parametrize("seed", range(4))
def test_children_tile_the_parent_lattice(seed):
    """Not relaxed: every lattice point of the parent lies in exactly one child, every child inside the
    parent -- negative coordinates, odd widths and width-1 dims included."""
    rng = np.random.default_rng(seed)
    q = sc.query(4, (1,), (1,))
    part = np.zeros(24, np.int32)
    c = sc.make_level(q, part, 1, seed, open_frac=1.0, leaf_frac=0.0, status=[ST_RUNNING], w=[rng.choice([1, 40, 100])],
                      wmax=3, span=5)
    o = sc.split_oracle(c)
    split = 0
    for n in range(c.Nn):
        kids = o.children[n]
        if not kids:
            continue
        split += 1
        assert len(kids) in (2, 4, 8, 16, 32, 64)
        for _, L, H, PL, PH in kids:
            assert np.all(L >= c.xlo[n]) and np.all(H <= c.xhi[n]) and np.all(L <= H)
            assert np.array_equal(PL, L) and np.array_equal(PH, H)
        for x in points(c.xlo[n], c.xhi[n]):
            assert sum(inside(x, L, H) for _, L, H, _, _ in kids) == 1, (n, x)
    assert split >= 10


def coupled_pairs(q, lo, hi, plo, phi):
    """(x, x') lattice pairs of a node: x in its x box, x' in its x' box, equal on the shared dims, within
    tau on the RA dims."""
    free = [d for d in range(q.n0) if d in q.ra]
    out = []
    for x in points(lo, hi):
        rng = [range(max(int(plo[d]), x[d] - q.tau), min(int(phi[d]), x[d] + q.tau) + 1) if d in free else [x[d]]
               for d in range(q.n0)]
        for xp in itertools.product(*rng):
            if inside(xp, plo, phi):
                out.append((x, xp))
    return out


@pytest.mark.parametrize("tau,ra", [(1, (2,)), (5, (2,)), (1, (0, 2)), (2, (0, 3))])
def test_relaxed_children_tile_the_coupled_pairs(tau, ra):
    """Relaxed: every coupled pair of the parent lies in exactly one kept child, and a child holds no
    coupled pair outside the parent -- with one and two RA dims, splits on x and on x' sides, shared
    dims split on the x side, and children dropped as empty."""
    q = sc.query(4, (1,), (1,), ra=ra, tau=tau)
    part = np.zeros(40, np.int32)
    c = sc.make_level(q, part, 1, 10 * tau + len(ra), open_frac=1.0, leaf_frac=0.0, status=[ST_RUNNING], w=[40],
                      wmax=3 if tau < 5 else 6, span=4, odd=0.05)
    o = sc.split_oracle(c)
    dropped = xp_split = shared_split = 0
    for n in range(c.Nn):
        dims = sc.pick_dims(c.scores[n], sc.mreq_of(40, c.m, c.target))
        kids = o.children[n]
        if not dims:
            assert not kids
            continue
        dropped += (1 << len(dims)) - len(kids)
        xp_split += any(d >= q.n0 for d in dims)
        shared_split += any(d < q.n0 and q.shared[d] for d in dims)
        parent = set(coupled_pairs(q, c.xlo[n], c.xhi[n], c.xplo[n], c.xphi[n]))
        seen = {}
        for k, (_, L, H, PL, PH) in enumerate(kids):
            for pr in coupled_pairs(q, L, H, PL, PH):
                assert pr in parent, (n, k, pr)
                assert pr not in seen, (n, k, seen[pr], pr)
                seen[pr] = k
        assert set(seen) == parent, n
    assert dropped > 0 and xp_split > 0 and shared_split > 0


def test_child_geometry_by_hand():
    q = sc.query(2, (), ())
    # [-3, -2]: mid = floor(-2.5) = -3; [-339603, -339503]: mid = -339553
    L, H, _, _, ok = sc.child_box(q, F([-3, -339603]), F([-2, -339503]), F([-3, -339603]), F([-2, -339503]), [0, 1], 0)
    assert ok and L.tolist() == [-3, -339603] and H.tolist() == [-3, -339553]
    L, H, _, _, ok = sc.child_box(q, F([-3, -339603]), F([-2, -339503]), F([-3, -339603]), F([-2, -339503]), [0, 1], 3)
    assert L.tolist() == [-2, -339552] and H.tolist() == [-2, -339503]
    # child bit j belongs to dims[j]: child 1 is the upper half along dims[0] = dim 1
    L, H, _, _, _ = sc.child_box(q, F([0, 0]), F([3, 3]), F([0, 0]), F([3, 3]), [1, 0], 1)
    assert L.tolist() == [0, 2] and H.tolist() == [1, 3]
    # relaxed, tau = 1, RA dim 0: x in [0, 7], x' in [6, 9]; lower x half [0, 3] is more than tau away
    qr = sc.query(2, (), (), ra=(0,), tau=1)
    lo, hi, plo, phi = F([0, 0]), F([7, 2]), F([6, 0]), F([9, 2])
    assert not sc.child_box(qr, lo, hi, plo, phi, [0], 0)[4]
    L, H, PL, PH, ok = sc.child_box(qr, lo, hi, plo, phi, [0], 1)
    assert ok and (L[0], H[0], PL[0], PH[0]) == (5, 7, 6, 8)
    # a shared dim split on the x side takes x' along
    L, H, PL, PH, ok = sc.child_box(qr, lo, hi, plo, phi, [1], 1)
    assert ok and (L[1], H[1], PL[1], PH[1]) == (2, 2, 2, 2)


def test_tightening_order_is_immaterial():
    """The tightening writes x' from x, then x from the new x'.  For tau >= 0 the other order gives the same
    boxes: lo1 = max(lo, max(plo, lo - tau) - tau) = max(lo, plo - tau), which does not see the new plo
    (and alike for the three other bounds).  So no case can tell the two orders apart -- checked here
    over every small box, because a kernel with the two pairs of lines swapped passes the GPU tests."""
    for tau in (0, 1, 2, 5):
        for lo, hi, plo, phi in itertools.product(range(-3, 4), repeat=4):
            a_plo, a_phi = max(plo, lo - tau), min(phi, hi + tau)
            a = (max(lo, a_plo - tau), min(hi, a_phi + tau), a_plo, a_phi)
            b_lo, b_hi = max(lo, plo - tau), min(hi, phi + tau)
            b = (b_lo, b_hi, max(plo, b_lo - tau), min(phi, b_hi + tau))
            assert a == b, (tau, lo, hi, plo, phi)


# ------------------------------------------------------------------------------------ branching rule
def mreq_by_hand(w, target):
    """The table: (target, largest w) -> split count, for m_max = 6."""
    if target <= 2:
        return 1                                   # w * 2 <= 2 only for w = 1, and 1 is the floor anyway
    table = {64: ((1, 6), (2, 5), (4, 4), (8, 3), (16, 2)),
             256: ((4, 6), (8, 5), (16, 4), (32, 3), (64, 2))}[target]
    for wmax, m in table:
        if w <= wmax:
            return m
    return 1


def test_split_count_table():
    for target in (1, 2, 64, 256):
        for w in range(1, 301):
            want = mreq_by_hand(w, target)
            assert sc.mreq_of(w, 6, target) == want, (w, target)
            assert sc.mreq_of(w, 9, target) == want                 # never more than 6
            for m in (1, 2, 3, 5):
                assert sc.mreq_of(w, m, target) == min(want, m), (w, m, target)
    assert sc.mreq_of(1, 0, 256) == 1                                # at least one dim


def test_pick_rules():
    nan = np.nan
    row = F([1.0, 3.0, 3.0, nan, -0.5, -1.0, 3.0, 0.25])
    assert sc.pick_dims(row, 1) == [1]                               # tie: the lower index
    assert sc.pick_dims(row, 3) == [1, 2, 6]
    assert sc.pick_dims(row, 6) == [1, 2, 6, 0, 7]                   # NaN, -0.5 and -1 are never picked
    assert sc.pick_dims(F([nan, -0.5, -1.0]), 2) == []
    assert sc.pick_dims(F([-0.4999, nan]), 2) == [0]
    assert sc.pick_dims(F([0.5, np.inf, 0.5]), 2) == [1, 0]


# ------------------------------------------------------------------ budget, probation and level end
def three_parts(nodes_start, budget, budget2, escalate, status=(ST_RUNNING,) * 3):
    """Three partitions, two open inner nodes each (boxes [0, 3]^2, one splittable score), w = 2."""
    q = sc.query(2, (), ())
    part = np.repeat(np.arange(3, dtype=np.int32), 2)
    box = (np.zeros((6, 2), F), np.full((6, 2), 3, F), np.zeros((6, 2), F), np.full((6, 2), 3, F))
    c = sc.make_level(q, part, 3, 0, open_frac=1.0, leaf_frac=0.0, status=status, w=[2, 2, 2], nodes_start=nodes_start,
                      budget=budget, budget2=budget2, escalate=escalate, target=2, boxes=box)
    c.scores[:] = F([1.0, -1.0, -1.0, -1.0])
    c.lvl_open[:] = 0
    c.part_nodes[:] = c.nodes_start
    return c


def test_budget_rule_by_hand():
    # budget 10: below, at and over it at the start of the level
    c = three_parts([9, 10, 11], 10, 20, escalate=False)
    o = sc.split_oracle(c)
    assert o.status.tolist() == [ST_RUNNING, ST_STOPPING, ST_STOPPING]
    assert [len(k) for k in o.children] == [2, 2, 0, 0, 0, 0]
    assert o.part_nodes.tolist() == [13, 10, 11] and o.lvl_open.tolist() == [2, 2, 2]
    # the same with escalation: probation instead of the stop, children made
    c = three_parts([9, 10, 11], 10, 20, escalate=True)
    o = sc.split_oracle(c)
    assert o.status.tolist() == [ST_RUNNING] * 3 and o.prob.tolist() == [0, 1, 1]
    assert o.part_nodes.tolist() == [13, 14, 15]
    # budget >= budget2: no probation
    c = three_parts([9, 10, 11], 10, 10, escalate=True)
    o = sc.split_oracle(c)
    assert o.status.tolist() == [ST_RUNNING, ST_STOPPING, ST_STOPPING] and o.prob.tolist() == [0, 0, 0]
    # STOPPING on entry but below its budget: still splits; decided partitions do nothing
    c = three_parts([3, 3, 3], 10, 20, escalate=False, status=(ST_STOPPING, ST_UNSAT, ST_SAT))
    o = sc.split_oracle(c)
    assert [len(k) for k in o.children] == [2, 2, 0, 0, 0, 0] and o.lvl_open.tolist() == [2, 0, 0]
    assert o.status.tolist() == [ST_STOPPING, ST_UNSAT, ST_SAT]


def settle_state(status, lvl_open, prob, pbudget, esc_budget=(), esc_open=(), max_open=2, budget2=100):
    i32 = np.int32
    return sc.SimpleNamespace(status=np.array(status, np.int8), lvl_open=np.array(lvl_open, i32),
                              part_open=np.full(3, -1, i32), part_nodes=np.array([30, 31, 32], i32),
                              nodes_start=np.array([20, 21, 22], i32), prev_start=np.array([10, 11, 12], i32),
                              pbudget=None if pbudget is None else np.array(pbudget, i32),
                              prob=None if prob is None else np.array(prob, np.uint8), budget2=budget2,
                              max_open=max_open, esc_budget=tuple(esc_budget), esc_open=tuple(esc_open),
                              counters_cur=np.array([17, 5], i32))


def test_settle_by_hand():
    r = sc.settle_oracle(settle_state([ST_STOPPING, ST_RUNNING, ST_UNSAT], [4, 5, 6], None, None))
    assert r.status.tolist() == [ST_UNKNOWN, ST_RUNNING, ST_UNSAT] and r.part_open.tolist() == [4, -1, -1]
    assert r.lvl_open.tolist() == [0, 0, 0] and r.prev_start.tolist() == [20, 21, 22]
    assert r.nodes_start.tolist() == [30, 31, 32] and r.host_counts.tolist() == [17, 5]
    assert r.counters_next.tolist() == [0, 0]
    # one step (esc.n = 0): frontier <= max_open continues with budget2
    r = sc.settle_oracle(settle_state([ST_RUNNING] * 3, [2, 3, 0], [1, 1, 0], [10, 10, 10]))
    assert r.status.tolist() == [ST_RUNNING, ST_UNKNOWN, ST_RUNNING] and r.pbudget.tolist() == [100, 10, 10]
    assert r.part_open.tolist() == [-1, 3, -1] and r.prob.tolist() == [0, 0, 0]
    # probation of a partition that also stopped (capacity): UNKNOWN
    r = sc.settle_oracle(settle_state([ST_STOPPING, ST_RUNNING, ST_RUNNING], [1, 1, 1], [1, 0, 0], [10, 10, 10]))
    assert r.status.tolist() == [ST_UNKNOWN, ST_RUNNING, ST_RUNNING] and r.pbudget.tolist() == [10, 10, 10]
    # two steps between: budgets 10 -> 20 -> 40 -> 100, limits max_open = 2, then 5, then 9
    esc = dict(esc_budget=(20, 40), esc_open=(5, 9))
    r = sc.settle_oracle(settle_state([ST_RUNNING] * 3, [2, 5, 9], [1, 1, 1], [10, 20, 40], **esc))
    assert r.status.tolist() == [ST_RUNNING] * 3 and r.pbudget.tolist() == [20, 40, 100]
    r = sc.settle_oracle(settle_state([ST_RUNNING] * 3, [3, 6, 10], [1, 1, 1], [10, 20, 40], **esc))
    assert r.status.tolist() == [ST_UNKNOWN] * 3 and r.part_open.tolist() == [3, 6, 10]
    # one step between
    r = sc.settle_oracle(settle_state([ST_RUNNING] * 3, [2, 3, 5], [1, 1, 1], [10, 20, 20], esc_budget=(20,),
                                      esc_open=(4,)))
    assert r.status.tolist() == [ST_RUNNING, ST_RUNNING, ST_UNKNOWN] and r.pbudget.tolist() == [20, 100, 20]


def test_capacities_in_node_order():
    """in_order: the pool cut in the middle of a node's children, and the candidate buffer cut in a leaf
    (stops) and at an inner node's candidate (dropped silently)."""
    c = three_parts([3, 3, 3], 10, 20, escalate=False)
    c.pe_lb[:], c.pe_ub[:] = -1, 1                                     # every node has a candidate
    o = sc.split_oracle(c)
    assert o.n_children == 12 and o.n_cands == 6
    rows, recs, status = sc.in_order(c, o, cap=7, cand_cap=4)
    assert len(rows) == 7 and len(recs) == 4
    assert status.tolist() == [ST_RUNNING, ST_STOPPING, ST_STOPPING]   # node 3 cut, nodes 4 and 5 past the end
    parent = sc.child_row(c.q, (1, c.xlo[3], c.xhi[3], c.xplo[3], c.xphi[3]))
    assert np.array_equal(rows[6], parent) and not np.array_equal(rows[5], parent)
    rows, recs, status = sc.in_order(c, o, cap=0, cand_cap=0)
    assert len(rows) == 0 and len(recs) == 0 and status.tolist() == [ST_STOPPING] * 3
