"""The BaB level kernels of csrc/bab.hip run one launch at a time (ops/hip.py: split_level, settle,
bab_init, bab_finish, mark_unknown, set_status) against the plain oracle of tests/split_cases.py, which
tests/test_split_cpu.py checks without a GPU.

Every level runs with the 16-lane-group split kernel (FAIRIFY_SPLIT_GROUPS=1; networks with 2 n0 <= 32)
and with the one-wave-per-node kernel (=0).  All values are small integers: every comparison is ==.  The
order of workgroups in the pool and in the candidate buffer follows device atomics, so both are compared
as sorted rows; per-partition state and the level counters are compared as they are, and each node's
children must sit contiguously in the pool, in child order."""
import functools

import numpy as np
import pytest
import torch

import split_cases as sc
from fairify_amd.ops import hip
from split_cases import ST_RUNNING, ST_SAT, ST_STOPPING, ST_UNKNOWN, ST_UNSAT, F  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = -7777          # what the output buffers hold before a launch
GUARD_ROWS = 5         # rows past the capacity that must keep it


@pytest.fixture(params=["1", "0"], ids=["groups", "waves"])
def kernel(request, monkeypatch):
    monkeypatch.setenv("FAIRIFY_SPLIT_GROUPS", request.param)
    return request.param


# ------------------------------------------------------------------------------------------ harness
def to_dev(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_state(dev, c):
    """The per-partition state of ``c`` on the device (updated in place by the launches)."""
    s = {k: to_dev(dev, getattr(c, k)) for k in ("status", "part_nodes", "nodes_start", "prev_start", "lvl_open",
                                                 "pbudget", "prob")}
    s["part_open"] = torch.full((c.P,), GUARD, dtype=torch.int32, device=dev)
    return s


def new_buffers(dev, c):
    q = c.q
    rows, crows = max(c.cap, 1) + GUARD_ROWS, max(c.cand_cap, 1) + GUARD_ROWS
    f = lambda *shape: torch.full(shape, float(GUARD), dtype=torch.float32, device=dev)      # noqa: E731
    pool = dict(oxlo=f(rows, q.n0), oxhi=f(rows, q.n0), opart=torch.full((rows,), GUARD, dtype=torch.int32, device=dev))
    if q.relaxed:
        pool.update(oxplo=f(rows, q.n0), oxphi=f(rows, q.n0))
    return pool, f(crows, 2 * q.n0 + 1), torch.zeros(2, dtype=torch.int32, device=dev)


def launch(dev, c, state, bufs, settle=None):
    """One split launch over the nodes of ``c`` on the device state ``state`` into ``bufs``."""
    q = c.q
    node = {k: to_dev(dev, getattr(c, k)) for k in ("xlo", "xhi", "part", "open", "leaf", "scores", "cand_x", "cand_xp",
                                                    "pe_lb", "pe_ub", "olb", "oub", "olbp", "oubp")}
    if q.relaxed:
        node.update(xplo=to_dev(dev, c.xplo), xphi=to_dev(dev, c.xphi), shared=to_dev(dev, q.shared), ra=q.ra,
                    tau=q.tau)
    pool, cand_buf, counters = bufs
    hip.split_level(pairs=to_dev(dev, q.pairs), values=to_dev(dev, q.values), pa=q.pa, norient=q.norient,
                    status=state["status"], part_nodes=state["part_nodes"], nodes_start=state["nodes_start"],
                    prev_start=state["prev_start"], lvl_open=state["lvl_open"], part_open=state["part_open"],
                    pbudget=state["pbudget"], prob=state["prob"], budget=c.budget, budget2=c.budget2, m=c.m,
                    target=c.target, cap=c.cap, cand_cap=c.cand_cap, pool=pool, cand_buf=cand_buf, counters=counters,
                    settle=settle, **node)
    torch.cuda.synchronize(dev)


def host(t):
    return None if t is None else t.cpu().numpy()


def read(c, state, bufs):
    """-> (pool rows [cap + guard, part | lo | hi (| plo | phi)], candidate rows [cand_cap + guard, x | x' |
    part], counters, state) on the host, as float64 / int arrays."""
    pool, cand_buf, counters = bufs
    q = c.q
    cols = [host(pool["opart"]).astype(np.float64)[:, None], host(pool["oxlo"]), host(pool["oxhi"])]
    if q.relaxed:
        cols += [host(pool["oxplo"]), host(pool["oxphi"])]
    rows = np.concatenate([a.astype(np.float64) for a in cols], 1) + 0.0
    cb = host(cand_buf)
    last = cb[:, 2 * q.n0:].copy()                   # the partition id as int bits, or the guard value still
    ids = np.where(last == GUARD, GUARD, last.view(np.int32)).astype(np.float64)
    recs = np.concatenate([cb[:, :2 * q.n0].astype(np.float64), ids], 1) + 0.0
    return rows, recs, host(counters), {k: host(v) for k, v in state.items()}


def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def untouched(rows, n):
    """Rows n.. of a buffer still hold the guard value."""
    return bool(np.all(rows[n:] == GUARD))


def check_contiguous(c, o, rows):
    """Every node's children sit in consecutive pool rows, in child order."""
    at = {}
    for i, r in enumerate(rows):
        at.setdefault(r.tobytes(), []).append(i)
    for n in range(c.Nn):
        kids = [sc.child_row(c.q, ch) + 0.0 for ch in o.children[n]]
        if not kids:
            continue
        starts = at.get(kids[0].tobytes(), [])
        assert any(i + len(kids) <= len(rows) and all(np.array_equal(rows[i + j], k) for j, k in enumerate(kids))
                   for i in starts), "children of node %d are not contiguous in child order" % n


def check_state(got, o, c, what=("status", "part_nodes", "lvl_open", "prob")):
    for k in what:
        want = getattr(o, k)
        if want is None:
            continue
        assert np.array_equal(got[k], want), (k, np.nonzero(got[k] != want)[0][:8], got[k][:16], want[:16])
    assert np.array_equal(got["nodes_start"], c.nodes_start) and np.array_equal(got["prev_start"], c.prev_start)


def run_and_check(dev, c, o=None):
    """One launch of the whole level with room for everything: pool, candidates, counters and the
    per-partition state against the oracle.  -> (pool rows, candidate rows, state)."""
    o = o or sc.split_oracle(c)
    assert c.cap >= o.n_children and c.cand_cap >= o.n_cands
    state, bufs = dev_state(dev, c), new_buffers(dev, c)
    launch(dev, c, state, bufs)
    rows, recs, counters, got = read(c, state, bufs)
    assert counters.tolist() == [o.n_children, o.n_cands]
    check_state(got, o, c)
    assert np.all(got["part_open"] == GUARD)                      # only the level end writes it
    want_rows, want_recs, _ = sc.in_order(c, o)
    assert untouched(rows, o.n_children) and untouched(recs, o.n_cands)
    assert np.array_equal(sort_rows(rows[:o.n_children]), sort_rows(want_rows))
    assert np.array_equal(sort_rows(recs[:o.n_cands]), sort_rows(want_recs))
    check_contiguous(c, o, rows[:o.n_children])
    return rows[:o.n_children], recs[:o.n_cands], got


QUERIES = {
    5: lambda: sc.query(5, (2,), (1,)),                                  # group kernel, npa = 1, V = 2
    13: lambda: sc.query(13, (12,), (1,), ra=(0, 3), tau=1),             # group kernel, relaxed, two RA dims
    16: lambda: sc.query(16, (7,), (2,)),                                # exactly 32 scores
    20: lambda: sc.query(20, (2,), (1,), ra=(1,), tau=5),                # 40 scores: the one-wave kernel only
    40: lambda: sc.query(40, (4,), (1,), ra=(30, 39), tau=1),            # x' scores 70 and 79: the lane's second
}


def random_part(Nn, P, rng, maxlen=9):
    """Runs of 1..maxlen nodes of random partitions: a partition comes back in runs that are not
    adjacent."""
    out = []
    while len(out) < Nn:
        out += [int(rng.integers(P))] * int(rng.integers(1, maxlen + 1))
    return np.array(out[:Nn], np.int32)


@functools.lru_cache(maxsize=None)
def boundary_case(n0, Nn):
    q = QUERIES[n0]()
    P = max(3, Nn // 5)
    c = sc.make_level(q, random_part(Nn, P, np.random.default_rng(Nn)), P, 100 * n0 + Nn)
    return c, sc.split_oracle(c)


# ------------------------------------------------------------------------------ workgroup boundaries
@pytest.mark.parametrize("Nn", [1, 7, 8, 9, 31, 32, 33, 64, 65, 257])
@pytest.mark.parametrize("n0", [5, 13, 16])
def test_workgroup_boundaries(cuda, kernel, n0, Nn):
    """Block sizes 8 (one wave per node) and 32 (groups): full, partial and several workgroups; about half
    the nodes closed, partitions of every status, leaves mixed in."""
    c, o = boundary_case(n0, Nn)
    run_and_check(cuda, c, o)


@pytest.mark.parametrize("Nn", [1, 7, 8, 9, 31, 32, 33, 64, 65, 257])
@pytest.mark.parametrize("n0", [20, 40])
def test_wide_inputs_take_the_wave_kernel_whatever_the_switch(cuda, monkeypatch, n0, Nn):
    """2 n0 > 32: both settings of the switch give the oracle's result and the same buffers."""
    c, o = boundary_case(n0, Nn)
    res = {}
    for groups in ("1", "0"):
        monkeypatch.setenv("FAIRIFY_SPLIT_GROUPS", groups)
        rows, recs, got = run_and_check(cuda, c, o)
        res[groups] = (sort_rows(rows), sort_rows(recs), got)
    assert np.array_equal(res["1"][0], res["0"][0]) and np.array_equal(res["1"][1], res["0"][1])
    for k, v in res["1"][2].items():
        assert v is None or np.array_equal(v, res["0"][2][k]), k


def test_boundary_cases_reach_the_paths_they_are_for():
    """The random cases above hold what they are meant to: second scores per lane, x' dims as best score,
    sparse feasibility masks that are no prefix, nodes whose children are all infeasible, nodes without
    a splittable dim and with fewer than the split count, NaN / -0.5 scores and ties at the top."""
    c, o = boundary_case(40, 257)
    assert any(d >= 64 for dims in o.dims for d in dims)
    seen = dict(xp_best=0, sparse=0, none_feasible=0, no_dim=0, few_dims=0, tie=0, nan=0, half=0, leaf_recs=0)
    for n0 in (5, 13, 16, 20, 40):
        for Nn in (65, 257):
            c, o = boundary_case(n0, Nn)
            for n in np.nonzero(c.open)[0]:
                p = c.part[n]
                if c.status[p] not in (ST_RUNNING, ST_STOPPING):
                    continue
                if o.is_leaf[n]:
                    seen["leaf_recs"] += len(o.cands[n]) > 0
                    continue
                dims, fm = o.dims[n], o.fmask[n]
                mreq = sc.mreq_of(c.nodes_start[p] - c.prev_start[p], c.m, c.target)
                seen["no_dim"] += not dims
                seen["few_dims"] += 0 < len(dims) < mreq
                if not dims:
                    continue
                row = c.scores[n]
                seen["xp_best"] += dims[0] >= c.q.n0
                seen["tie"] += np.sum(row == row[dims[0]]) > 1
                seen["nan"] += bool(np.any(np.isnan(row)))
                seen["half"] += bool(np.any(row == F(-0.5)))
                seen["none_feasible"] += fm == 0
                seen["sparse"] += fm != 0 and (fm & (fm + 1)) != 0
    assert all(v > 0 for v in seen.values()), seen


# ---------------------------------------------------------------------------- many nodes per wave
def spread_open(Nn, n_open, rng):
    """About n_open open nodes: both ends of random 64-node blocks, and runs of 2..12 that cross a block
    boundary."""
    op = np.zeros(Nn, np.uint8)
    blocks = rng.choice(Nn // 64, n_open // 4, replace=False)
    for b in blocks[: len(blocks) // 2]:
        op[64 * b] = op[64 * b + 63] = 1
    for b in blocks[len(blocks) // 2:]:
        a = 64 * b - int(rng.integers(1, 7))
        op[max(a, 0):64 * b + int(rng.integers(1, 7))] = 1
    return op


@functools.lru_cache(maxsize=None)
def big_case(Nn):
    rng = np.random.default_rng(Nn)
    q = QUERIES[5]()
    P = 400
    runs, n = [], 0
    while n < Nn:                                    # partitions in order, runs of 1..400 nodes
        k = int(rng.choice([1, 2, 63, 64, 65, 200, 400]))
        runs.append((len(runs) % P, min(k, Nn - n)))
        n += runs[-1][1]
    w = np.where(rng.random(P) < 0.1, 3, rng.integers(100, 129, P))       # mostly binary splits
    c = sc.make_level(q, sc.runs_to_part(runs), P, Nn, open_frac=0.0, leaf_frac=0.1, w=w, cap=0, cand_cap=0)
    c.open = spread_open(Nn, 2000, rng)
    o = sc.split_oracle(c)
    c.cap, c.cand_cap = o.n_children + 11, o.n_cands + 11
    return c, o


@pytest.mark.parametrize("Nn", [33000, 66000])
def test_many_nodes_per_wave(cuda, kernel, Nn):
    """66 000 nodes: eight nodes per wave (npw = 8) and two passes per group wave (npp = 2); 33 000: npw =
    4.  Some 2 000 nodes are open, at both ends of the 64-node blocks and in runs across them."""
    c, o = big_case(Nn)
    assert 1500 < int(c.open.sum()) < 4000 and o.n_children > 1000
    run_and_check(cuda, c, o)


# ------------------------------------------------------------------------------- segmented counters
@functools.lru_cache(maxsize=None)
def runs_case(offset):
    rng = np.random.default_rng(offset)
    lengths = [1, 2, 63, 64, 65, 200, 1, 65, 2, 64, 63, 1, 1, 200]
    P = 6
    runs = [(int(rng.integers(P)), offset)] if offset else []
    last = runs[0][0] if runs else -1
    for k in lengths:                                 # a partition comes back after other partitions' runs
        p = int(rng.choice([x for x in range(P) if x != last]))
        runs.append((p, k))
        last = p
    c = sc.make_level(sc.query(5, (2,), (1,)), sc.runs_to_part(runs), P, offset, open_frac=0.9, leaf_frac=0.1,
                      status=[ST_RUNNING] * 5 + [ST_STOPPING], w=rng.integers(90, 129, P))
    return c, sc.split_oracle(c)


@pytest.mark.parametrize("offset", [0, 5, 37])
def test_segmented_counters(cuda, kernel, offset):
    """Partition runs of 1, 2, 63, 64, 65 and 200 nodes from arbitrary offsets, partitions in runs that
    are not adjacent: part_nodes and lvl_open are exact."""
    c, o = runs_case(offset)
    assert len(set(c.part.tolist())) == 6
    run_and_check(cuda, c, o)


# ------------------------------------------------------------------------------------ branching rule
@functools.lru_cache(maxsize=None)
def branching_case(m, relaxed):
    q = sc.query(13, (12,), (1,), ra=(0, 3), tau=1) if relaxed else sc.query(13, (12,), (1,))
    P, per = 8, 6
    part = np.repeat(np.arange(P, dtype=np.int32), per)
    w = [1, 3, 100, 128, 1, 4, 5, 64]                 # target 256: 6, 6, 1, 1, 6, 6, 5, 2 split dims
    c = sc.make_level(q, part, P, 7 + m + 10 * relaxed, open_frac=1.0, leaf_frac=0.0, status=[ST_RUNNING] * P, w=w,
                      wmax=5, m=m, target=256, odd=0.12)
    c.scores[0] = sc.fix_scores(q, np.full((1, 26), 2.0, F), c.xlo[:1], c.xhi[:1], c.xplo[:1], c.xphi[:1])[0]  # tied
    c.scores[1] = -1.0                                # no splittable dim: open, no children
    c.scores[2, :] = [np.nan, -0.5] * 13              # the same, with NaN and scores exactly -0.5
    keep = sc.pick_dims(c.scores[3], 2)               # two splittable dims, whatever the split count
    c.scores[3, [d for d in range(26) if d not in keep]] = -1.0
    o = sc.split_oracle(c)
    c.cap = o.n_children + 9
    return c, o


@pytest.mark.parametrize("relaxed", [0, 1], ids=["plain", "relaxed"])
@pytest.mark.parametrize("m", [6, 3, 1])
def test_branching_rule(cuda, kernel, m, relaxed):
    """target 256 with w = 1 (64 children: four ballot rounds of the group kernel), 3, 100, 128; a.m below
    6; fewer splittable dims than the split count; none at all; ties, NaN and -0.5."""
    c, o = branching_case(m, relaxed)
    nd = [len(d) for d in o.dims]
    assert max(nd) == m and not o.children[1] and not o.children[2] and o.lvl_open[0] >= c.lvl_open[0] + 6
    if m == 6:
        assert any(len(k) == 64 for k in o.children) or relaxed
        assert nd[3] == 2                                            # fewer splittable dims than asked for
    run_and_check(cuda, c, o)


# ------------------------------------------------------------------------------------ child geometry
def test_child_geometry(cuda, kernel):
    """Negative coordinates and odd widths, width-1 dims, every dim split at once."""
    q = sc.query(5, (2,), (1,))
    lo = F([[-3, -339603, 0, -1, 7], [-3, -3, 0, -2, -2], [0, 0, 0, 0, 0], [-8388000, 5, 0, -7, -1]])
    hi = F([[-2, -339503, 1, 0, 8], [-2, -2, 1, -1, -1], [1, 1, 1, 1, 1], [-8387001, 6, 1, 6, 0]])
    c = sc.make_level(q, np.zeros(4, np.int32), 1, 3, open_frac=1.0, leaf_frac=0.0, status=[ST_RUNNING], w=[1],
                      boxes=(lo, hi, lo, hi))
    c.scores[:] = sc.fix_scores(q, np.tile(F([3, 2, 9, 1, 1, 9, 9, 9, 9, 9]), (4, 1)), lo, hi, lo, hi)
    o = sc.split_oracle(c)
    assert [len(k) for k in o.children] == [16] * 4
    c.cap = o.n_children
    rows, _, _ = run_and_check(cuda, c, o)
    assert [-3, -339603, 0, -1, 7] + [-3, -339553, 1, -1, 7] in rows[:, 1:].tolist()


@functools.lru_cache(maxsize=None)
def relaxed_case(tau):
    q = sc.query(6, (5,), (1,), ra=(1, 4), tau=tau)
    c = sc.make_level(q, random_part(90, 7, np.random.default_rng(tau), 20), 7, 40 + tau, open_frac=0.9, leaf_frac=0.1,
                      status=[ST_RUNNING] * 7, w=[1, 2, 9, 20, 40, 100, 3], wmax=3 if tau == 1 else 9, odd=0.05)
    return c, sc.split_oracle(c)


@pytest.mark.parametrize("tau", [1, 5])
def test_relaxed_children(cuda, kernel, tau):
    """Two RA dims: splits on the x and the x' side and of shared dims, children emptied by the coupling
    (feasibility masks that are no prefix), nodes all of whose children are empty."""
    c, o = relaxed_case(tau)
    q = c.q
    inner = [n for n in range(c.Nn) if o.dims[n]]
    assert any((o.fmask[n] & (o.fmask[n] + 1)) != 0 for n in inner)                  # sparse, not a prefix
    assert any(o.fmask[n] == 0 for n in inner)                                       # every child infeasible
    assert any(d >= q.n0 for n in inner for d in o.dims[n])                          # x' side
    assert any(d < q.n0 and q.shared[d] for n in inner for d in o.dims[n])           # shared dim, x side
    assert any(bin(o.fmask[n]).count("1") > 16 for n in inner)                      # more than one ballot round
    run_and_check(cuda, c, o)


# -------------------------------------------------------------------------------------------- leaves
LEAF_QUERIES = {
    "npa1_V2": lambda: sc.query(5, (2,), (1,)),
    "npa2_V12": lambda: sc.query(5, (2, 0), (2, 3)),                       # 132 tests: nine rounds of 16, three of 64
    "npa2_V12_relaxed": lambda: sc.query(5, (2, 0), (2, 3), ra=(3,), tau=1),    # both orientations: 264 tests
    "odd_pairs": lambda: sc.query(5, (2, 0), (2, 3), npairs=37),
}


@functools.lru_cache(maxsize=None)
def leaf_case(name):
    q = LEAF_QUERIES[name]()
    c = sc.make_level(q, random_part(70, 5, np.random.default_rng(5)), 5, 11, open_frac=0.8, leaf_frac=0.7,
                      status=[ST_RUNNING, ST_RUNNING, ST_STOPPING, ST_UNSAT, ST_RUNNING])
    c.olb[c.olb == 1] = -1                            # two thirds of the bounds on the possible side, zeros kept
    c.oubp[c.oubp == -1] = 1
    o = sc.split_oracle(c)
    c.cap, c.cand_cap = o.n_children + 4, o.n_cands + 4
    return c, sc.split_oracle(c)


@pytest.mark.parametrize("name", sorted(LEAF_QUERIES))
def test_leaves(cuda, kernel, name):
    """One record per possible (orientation, pair) in t order with the PA values substituted; bounds of
    exactly 0 are not possible violations."""
    c, o = leaf_case(name)
    assert c.q.norient == (2 if "relaxed" in name else 1)
    leaves = [n for n in range(c.Nn) if o.is_leaf[n]]
    assert len(leaves) > 20 and (c.q.Pp < 132 or any(len(o.cands[n]) > 64 for n in leaves))
    assert np.any(c.olb == 0) and np.any(c.oubp == 0)
    state, bufs = dev_state(cuda, c), new_buffers(cuda, c)
    launch(cuda, c, state, bufs)
    rows, recs, counters, got = read(c, state, bufs)
    assert counters.tolist() == [o.n_children, o.n_cands]
    # a leaf's records are consecutive and in t order: find each leaf's first record
    for n in leaves:
        want = np.array(o.cands[n]).reshape(-1, recs.shape[1])
        if len(want) == 0:
            continue
        hits = np.nonzero(np.all(recs[:o.n_cands] == want[0], 1))[0]
        assert any(i + len(want) <= o.n_cands and np.array_equal(recs[i:i + len(want)], want) for i in hits), n
    run_and_check(cuda, c, o)


# -------------------------------------------------------------------------------------------- budget
@pytest.mark.parametrize("escalate,budget2", [(False, 64), (True, 64), (True, 30), (True, 20)])
def test_budget_rule(cuda, kernel, escalate, budget2):
    """nodes_start = budget - 1, budget, budget + 1, with and without the probation flags, budget >=
    budget2 (no probation), and partitions STOPPING on entry below and over their budget."""
    q = QUERIES[5]()
    B = 30
    ns = [B - 1, B, B + 1, B - 1, B + 1, 0, B, B]
    status = [ST_RUNNING] * 3 + [ST_STOPPING, ST_STOPPING, ST_RUNNING, ST_SAT, ST_RUNNING]
    c = sc.make_level(q, random_part(120, 8, np.random.default_rng(2), 12), 8, 21, open_frac=0.8, leaf_frac=0.1,
                      status=status, w=[8] * 8, nodes_start=ns, budget=B, budget2=budget2, escalate=escalate)
    if escalate:
        c.pbudget[7] = max(B, budget2) + 5           # this partition's own budget is further out
    o = sc.split_oracle(c)
    c.cap, c.cand_cap = o.n_children + 5, o.n_cands + 5
    if escalate and budget2 > B:
        assert o.prob.tolist() == [0, 1, 1, 0, 1, 0, 0, 0] and o.status.tolist() == status
    else:
        want = [ST_RUNNING, ST_STOPPING, ST_STOPPING, ST_STOPPING, ST_STOPPING, ST_RUNNING, ST_SAT,
                ST_RUNNING if escalate else ST_STOPPING]
        assert o.status.tolist() == want
        assert any(o.children[n] for n in range(c.Nn) if c.part[n] == 3)          # STOPPING on entry: splits
    run_and_check(cuda, c, o)


# --------------------------------------------------------------------------- capacity, one workgroup
@functools.lru_cache(maxsize=None)
def small_case(relaxed):
    q = sc.query(5, (2, 0), (2, 3), ra=(3,), tau=1) if relaxed else sc.query(5, (2, 0), (2, 3))
    part = np.array([0, 0, 1, 1, 2, 3, 3, 4], np.int32)
    c = sc.make_level(q, part, 5, 4, open_frac=1.0, leaf_frac=0.0, status=[ST_RUNNING] * 5,
                      w=[64, 64, 128, 64, 100], wmax=4)
    c.leaf[[1, 5]] = 1
    c.olb[:], c.oubp[:] = -1, 1                       # every pair of a leaf is possible
    c.pe_lb[:], c.pe_ub[:] = -1, 1                    # every inner node has a candidate
    o = sc.split_oracle(c)
    assert all(len(o.children[n]) >= 2 for n in (0, 2, 3, 4, 6, 7)), [len(k) for k in o.children]
    return c, o


def capacity_points(c, o):
    """(cap, cand_cap) pairs: the pool cut inside node 3's children (the later nodes then start past the
    end), inside the first node's, at 0; the candidate buffer cut inside leaf 1's records, at the slot of
    inner node 2's candidate (dropped), at 0; and one of each together."""
    k = [len(x) for x in o.children]
    q = [len(x) for x in o.cands]
    big, cbig = o.n_children + 3, o.n_cands + 3
    cut3 = sum(k[:3]) + 1
    in_leaf1 = q[0] + q[1] // 2
    at_node2 = q[0] + q[1]
    return [(cut3, cbig), (1, cbig), (0, cbig), (big, in_leaf1), (big, at_node2), (big, at_node2 + 1), (big, 0),
            (cut3, at_node2), (sum(k[:3]), sum(q[:5]) + 1)]


@pytest.mark.parametrize("point", range(9))
@pytest.mark.parametrize("relaxed", [0, 1], ids=["plain", "relaxed"])
def test_capacity_single_workgroup(cuda, kernel, relaxed, point):
    """Eight nodes: one workgroup in both kernels, so slots follow node order and everything is
    determined.  Truncated partitions are STOPPING, the slots below the capacity hold the parent (opart
    set), nothing is written at or past a capacity, and the counters hold the planned totals."""
    c0, o = small_case(relaxed)
    c = sc.SimpleNamespace(**vars(c0))
    c.cap, c.cand_cap = capacity_points(c0, o)[point]
    want_rows, want_recs, want_status = sc.in_order(c, o)
    state, bufs = dev_state(cuda, c), new_buffers(cuda, c)
    launch(cuda, c, state, bufs)
    rows, recs, counters, got = read(c, state, bufs)
    assert counters.tolist() == [o.n_children, o.n_cands]            # planned, not written
    assert np.array_equal(got["status"], want_status), (got["status"], want_status)
    assert np.array_equal(got["part_nodes"], o.part_nodes) and np.array_equal(got["lvl_open"], o.lvl_open)
    nw, nc = min(o.n_children, c.cap), min(o.n_cands, c.cand_cap)
    assert len(want_rows) == nw and len(want_recs) == nc
    assert np.array_equal(rows[:nw], want_rows)
    assert untouched(rows, nw)
    # an inner node's dropped candidate leaves its slot unwritten: compare the written slots only
    assert np.array_equal(recs[:nc], want_recs) and untouched(recs, nc)
    if point == 4:      # the candidate of inner node 2 is the first one past the end: dropped, partition 1 goes on
        assert want_status[1] == ST_RUNNING and want_status[0] == ST_RUNNING
    if point == 3:
        assert want_status[0] == ST_STOPPING


# ------------------------------------------------------------------------ capacity, many workgroups
@pytest.mark.parametrize("relaxed", [0, 1], ids=["plain", "relaxed"])
def test_capacity_many_workgroups(cuda, kernel, relaxed):
    """Which partition stops when several workgroups overflow depends on the order the atomics were
    served in: properties only."""
    q = QUERIES[13]() if relaxed else QUERIES[5]()
    P = 12
    c = sc.make_level(q, random_part(300, P, np.random.default_rng(8), 30), P, 17 + relaxed, open_frac=0.8,
                      leaf_frac=0.15, status=[ST_RUNNING] * 10 + [ST_UNSAT, ST_STOPPING], w=[30] * P)
    o = sc.split_oracle(c)
    c.cap, c.cand_cap = o.n_children // 2 + 1, o.n_cands // 2 + 1
    state, bufs = dev_state(cuda, c), new_buffers(cuda, c)
    launch(cuda, c, state, bufs)
    rows, recs, counters, got = read(c, state, bufs)
    assert counters.tolist() == [o.n_children, o.n_cands]
    assert np.array_equal(got["part_nodes"], o.part_nodes) and np.array_equal(got["lvl_open"], o.lvl_open)
    assert untouched(rows, c.cap) and untouched(recs, c.cand_cap)
    status = got["status"]
    assert np.all((status == o.status) | ((status == ST_STOPPING) & np.isin(o.status, (ST_RUNNING, ST_STOPPING))))
    key = lambda r: (r + 0.0).tobytes()                                                  # noqa: E731
    genuine, parents = {}, set()
    for n in range(c.Nn):
        for ch in o.children[n]:
            genuine[key(sc.child_row(q, ch))] = genuine.get(key(sc.child_row(q, ch)), 0) + 1
        if o.children[n]:
            parents.add(key(sc.child_row(q, (c.part[n], c.xlo[n], c.xhi[n], c.xplo[n], c.xphi[n]))))
    written = {}
    for r in rows[:c.cap]:
        k, p = key(r), int(r[0])
        assert k in genuine or (k in parents and status[p] == ST_STOPPING), r
        written[k] = written.get(k, 0) + 1
    lost_child = set()
    for n in range(c.Nn):
        for ch in o.children[n]:
            k = key(sc.child_row(q, ch))
            if written.get(k, 0) < genuine[k]:
                lost_child.add(int(c.part[n]))
    assert lost_child and all(status[p] == ST_STOPPING for p in lost_child)
    # candidates: every written record is genuine; a partition that lost a leaf record has stopped
    want = {}
    for n in range(c.Nn):
        for r in o.cands[n]:
            want.setdefault(key(r), []).append(n)
    have = {}
    for r in recs[:c.cand_cap]:
        assert key(r) in want, r
        have[key(r)] = have.get(key(r), 0) + 1
    lost_leaf = {int(c.part[n]) for k, ns in want.items() if have.get(k, 0) < len(ns) for n in ns if o.is_leaf[n]}
    assert lost_leaf and all(status[p] == ST_STOPPING for p in lost_leaf)


# ------------------------------------------------------------------------ sub-batches and level end
def settle_inputs(c, got_state, counters, esc):
    return sc.SimpleNamespace(status=got_state["status"], lvl_open=got_state["lvl_open"],
                              part_open=got_state["part_open"], part_nodes=got_state["part_nodes"],
                              nodes_start=got_state["nodes_start"], prev_start=got_state["prev_start"],
                              pbudget=got_state["pbudget"], prob=got_state["prob"], budget2=c.budget2,
                              max_open=esc["max_open"], esc_budget=esc["esc_budget"], esc_open=esc["esc_open"],
                              counters_cur=counters)


def check_settled(got, counters_next, host_counts, done, want):
    for k in ("status", "part_open", "lvl_open", "prev_start", "nodes_start", "pbudget", "prob", "part_nodes"):
        w = getattr(want, k)
        assert w is None or np.array_equal(got[k], w), (k, got[k], w)
    assert np.all(got["lvl_open"] == 0) and (got["prob"] is None or np.all(got["prob"] == 0))
    assert host(host_counts).tolist() == want.host_counts.tolist()
    assert host(counters_next).tolist() == [0, 0]
    assert done is None or host(done).tolist() == [0]


@functools.lru_cache(maxsize=None)
def settle_case(escalate):
    q = QUERIES[5]()
    B, P = 30, 9
    ns = [B - 1, B, B + 1, 45, 70, 3, B, 62, 41]
    status = [ST_RUNNING] * 5 + [ST_STOPPING, ST_UNSAT, ST_RUNNING, ST_RUNNING]
    c = sc.make_level(q, random_part(100, P, np.random.default_rng(3), 7), P, 33, open_frac=0.7, leaf_frac=0.1,
                      status=status, w=[6] * P, nodes_start=ns, budget=B, budget2=90, escalate=escalate)
    if escalate:
        c.pbudget[:] = [B, B, B, 40, 60, B, B, 60, 40]       # partitions at different escalation steps
    c.lvl_open[:] = 0
    c.part_nodes[:] = c.nodes_start
    return c


ESC = {0: dict(esc_budget=(), esc_open=()), 1: dict(esc_budget=(40,), esc_open=(0,)),
       2: dict(esc_budget=(40, 60), esc_open=(0, 0))}      # budget 30 -> ... -> budget2 90


@pytest.mark.parametrize("how", ["separate", "fused_second", "fused_single"])
@pytest.mark.parametrize("escalate,esc_n,side", [(False, 0, 0)] + [(True, n, s) for n in (0, 1, 2) for s in (0, 1)],
                         ids=["stop"] + ["esc%d_%s" % (n, s) for n in (0, 1, 2) for s in ("at_limit", "over_limit")])
def test_sub_batches_and_settle(cuda, kernel, escalate, esc_n, side, how):
    """One level as two launches into the same pool and counters, ended by a separate settle, by the
    settle fused into the second launch, or by one launch with the fused settle: the same state either
    way.  Each step's frontier limit is the largest open count of the probation partitions at that step
    (all continue) or one below (those end UNKNOWN), for 0, 1 and 2 escalation steps between the budgets."""
    c = settle_case(escalate)
    cut = 37
    subs = [c] if how == "fused_single" else [sc.sub_level(c, 0, cut), sc.sub_level(c, cut, c.Nn)]
    # oracle: the launches one after the other on the running state
    run = sc.SimpleNamespace(**vars(c))
    n_children = n_cands = 0
    all_rows, all_recs = [], []
    for s in subs:
        now = {k: getattr(run, k) for k in ("status", "part_nodes", "lvl_open", "prob")}
        s = sc.SimpleNamespace(**{**vars(s), **now})
        o = sc.split_oracle(s)
        r, k, _ = sc.in_order(s, o, 1 << 30, 1 << 30)
        all_rows.append(r)
        all_recs.append(k)
        n_children, n_cands = n_children + o.n_children, n_cands + o.n_cands
        run.status, run.part_nodes, run.lvl_open, run.prob = o.status, o.part_nodes, o.lvl_open, o.prob
    c.cap, c.cand_cap = n_children + 3, n_cands + 3
    esc = dict(ESC[esc_n])
    if escalate:
        # limits from the frontier of the probation partitions, by the step each one is at
        on = [p for p in range(c.P) if run.prob[p] and run.status[p] == ST_RUNNING]
        assert len(on) >= 3
        step = {p: sum(1 for b in esc["esc_budget"] if b <= c.pbudget[p]) for p in on}
        assert set(step.values()) == set(range(esc_n + 1)), step
        lim = [max(int(run.lvl_open[p]) for p in on if step[p] == k) - side for k in range(esc_n + 1)]
        esc["max_open"], esc["esc_open"] = lim[0], tuple(lim[1:])
    else:
        esc["max_open"] = 2
    before = dict(status=run.status, lvl_open=run.lvl_open, part_open=np.full(c.P, GUARD, np.int32),
                  part_nodes=run.part_nodes, nodes_start=c.nodes_start, prev_start=c.prev_start, pbudget=c.pbudget,
                  prob=run.prob)
    want = sc.settle_oracle(settle_inputs(c, before, np.array([n_children, n_cands], np.int32), esc))
    if escalate:
        ended = [p for p in on if want.status[p] == ST_UNKNOWN]
        assert (len(ended) > 0) == bool(side) and (side or all(want.pbudget[p] > c.pbudget[p] for p in on))
    # device
    state, bufs = dev_state(cuda, c), new_buffers(cuda, c)
    nxt = torch.full((2,), 99, dtype=torch.int32, device=cuda)
    hc = torch.full((2,), GUARD, dtype=torch.int32, device=cuda)
    done = torch.zeros(1, dtype=torch.int32, device=cuda)
    fused = dict(counters_next=nxt, host_counts=hc, done=done, **esc)
    for i, s in enumerate(subs):
        s.cap, s.cand_cap = c.cap, c.cand_cap
        launch(cuda, s, state, bufs, settle=fused if (how != "separate" and i == len(subs) - 1) else None)
    if how == "separate":
        out = hip.settle(counters_cur=bufs[2], counters_next=nxt, host_counts=hc, budget2=c.budget2,
                         **{k: state[k] for k in ("status", "lvl_open", "part_open", "part_nodes", "nodes_start",
                                                  "prev_start", "pbudget", "prob")}, **esc)
        assert out is hc
        torch.cuda.synchronize(cuda)
    rows, recs, counters, got = read(c, state, bufs)
    assert counters.tolist() == [n_children, n_cands]
    check_settled(got, nxt, hc, None if how == "separate" else done, want)
    assert np.array_equal(sort_rows(rows[:n_children]), sort_rows(np.concatenate(all_rows)))
    assert np.array_equal(sort_rows(recs[:n_cands]), sort_rows(np.concatenate(all_recs)))
    assert untouched(rows, n_children) and untouched(recs, n_cands)
    if how != "fused_single":       # the second launch's children come after all of the first one's
        assert np.array_equal(sort_rows(rows[:len(all_rows[0])]), sort_rows(all_rows[0]))


@pytest.mark.parametrize("esc_n", [0, 1, 2])
def test_settle_kernel_on_many_partitions(cuda, esc_n):
    """The level end on 700 partitions (three workgroups) of every status, on and off probation, at every
    escalation step, with frontiers on both sides of each limit."""
    rng = np.random.default_rng(esc_n)
    P, i32 = 700, np.int32
    budgets = [10] + list(ESC[esc_n]["esc_budget"])
    esc = dict(esc_budget=ESC[esc_n]["esc_budget"], esc_open=tuple(range(7, 7 + 2 * esc_n, 2)), max_open=5)
    s = sc.SimpleNamespace(status=rng.integers(0, 5, P).astype(np.int8), lvl_open=rng.integers(3, 13, P).astype(i32),
                           part_open=np.full(P, GUARD, i32), part_nodes=rng.integers(50, 90, P).astype(i32),
                           nodes_start=rng.integers(20, 50, P).astype(i32),
                           prev_start=rng.integers(0, 20, P).astype(i32),
                           pbudget=rng.choice(budgets + [12, 90], P).astype(i32),
                           prob=rng.integers(0, 2, P).astype(np.uint8),
                           budget2=90, counters_cur=np.array([123, 45], i32), **esc)
    want = sc.settle_oracle(s)
    on = (s.prob == 1) & (s.status == ST_RUNNING)
    assert np.any(on & (want.status == ST_UNKNOWN)) and np.any(on & (want.status == ST_RUNNING))
    assert set(np.unique(want.pbudget[on & (want.status == ST_RUNNING)])) >= set(budgets[1:] + [90])
    d = {k: to_dev(cuda, getattr(s, k)) for k in ("status", "lvl_open", "part_open", "part_nodes", "nodes_start",
                                                  "prev_start", "pbudget", "prob", "counters_cur")}
    nxt = torch.full((2,), 99, dtype=torch.int32, device=cuda)
    hc = hip.settle(counters_next=nxt, budget2=90, **d, **esc)
    torch.cuda.synchronize(cuda)
    check_settled({k: host(v) for k, v in d.items()}, nxt, hc, None, want)
    assert host(d["counters_cur"]).tolist() == [123, 45]


# ------------------------------------------------------------------------------- two levels chained
@pytest.mark.parametrize("relaxed", [0, 1], ids=["plain", "relaxed"])
def test_two_levels_chained(cuda, kernel, relaxed):
    """Level 1's output pool is level 2's input, with fresh synthetic certificates: prev_start /
    nodes_start handed over by the fused level end decide each partition's split count in level 2."""
    q = QUERIES[13]() if relaxed else QUERIES[5]()
    P = 5
    c1 = sc.make_level(q, np.arange(P, dtype=np.int32), P, 50 + relaxed, open_frac=1.0, leaf_frac=0.0,
                       status=[ST_RUNNING] * 4 + [ST_UNSAT], w=[1] * P, nodes_start=[0] * P, wmax=6, target=16,
                       odd=0.05)
    c1.part_nodes[:], c1.lvl_open[:] = 0, 0
    for p in range(4):                                # partition p splits along p + 1 dims
        c1.scores[p, sc.pick_dims(c1.scores[p], 4)[p + 1:]] = -1.0
    o1 = sc.split_oracle(c1)
    c1.cap, c1.cand_cap = o1.n_children, o1.n_cands
    state, bufs = dev_state(cuda, c1), new_buffers(cuda, c1)
    counters2 = torch.full((2,), 99, dtype=torch.int32, device=cuda)
    hc = torch.zeros(2, dtype=torch.int32, device=cuda)
    done = torch.zeros(1, dtype=torch.int32, device=cuda)
    launch(cuda, c1, state, bufs, settle=dict(counters_next=counters2, host_counts=hc, done=done, max_open=0))
    rows, _, _, got = read(c1, state, bufs)
    n1 = o1.n_children
    assert host(hc).tolist() == [n1, o1.n_cands] and n1 > 8
    kids = np.bincount(rows[:n1, 0].astype(int), minlength=P)
    assert np.array_equal(got["nodes_start"] - got["prev_start"], kids)              # w of level 2
    assert len(set(kids[:4].tolist())) > 1                                           # different split counts
    # level 2 on the pool as the device holds it
    n0 = q.n0
    boxes = [rows[:n1, 1 + k * n0:1 + (k + 1) * n0].astype(F) for k in range(4 if relaxed else 2)]
    if not relaxed:
        boxes += boxes
    c2 = sc.make_level(q, rows[:n1, 0].astype(np.int32), P, 60, open_frac=0.8, leaf_frac=0.0, status=got["status"],
                       target=16, boxes=boxes, odd=0.05)
    for k in ("nodes_start", "prev_start", "part_nodes", "lvl_open"):
        setattr(c2, k, got[k].copy())
    o2 = sc.split_oracle(c2)
    c2.cap, c2.cand_cap = o2.n_children + 2, o2.n_cands + 2
    for p in range(4):
        mine = [len(o2.dims[n]) for n in range(c2.Nn) if c2.part[n] == p and o2.dims[n]]
        assert not mine or max(mine) <= sc.mreq_of(kids[p], 6, 16)
    bufs2 = new_buffers(cuda, c2)
    bufs2 = (bufs2[0], bufs2[1], counters2)           # the slot level 1's end cleared
    launch(cuda, c2, state, bufs2)
    rows2, recs2, counters, got2 = read(c2, state, bufs2)
    assert counters.tolist() == [o2.n_children, o2.n_cands]
    check_state(got2, o2, c2, ("status", "part_nodes", "lvl_open"))
    want_rows, want_recs, _ = sc.in_order(c2, o2)
    assert np.array_equal(sort_rows(rows2[:o2.n_children]), sort_rows(want_rows))
    assert np.array_equal(sort_rows(recs2[:o2.n_cands]), sort_rows(want_recs))
    check_contiguous(c2, o2, rows2[:o2.n_children])


# ------------------------------------------------------------------- init, finish, mark and status
@pytest.mark.parametrize("relaxed", [False, True], ids=["plain", "relaxed"])
@pytest.mark.parametrize("escalate", [False, True], ids=["stop", "probation"])
@pytest.mark.parametrize("P", [1, 6, 7, 300])
def test_bab_init(cuda, P, escalate, relaxed):
    """The staged block with P not a multiple of 4 (padding), n_run < P; x' = x widened by tau on the RA
    dims only; every per-partition word and the five counters initialised."""
    rng = np.random.default_rng(P)
    n0, ra, tau = 5, (1, 3), 2
    st = rng.integers(0, 4, P).astype(np.int8)
    st[0] = ST_RUNNING
    run = np.nonzero(st == ST_RUNNING)[0].astype(np.int32)
    assert P == 1 or len(run) < P
    lo = rng.integers(-9, 10, (len(run), n0)).astype(F)
    hi = lo + rng.integers(0, 5, (len(run), n0)).astype(F)
    s = {k: host(v) for k, v in hip.bab_init(st, run, lo, hi, budget=77, ra=ra, tau=tau, relaxed=relaxed,
                                             escalate=escalate).items()}
    assert np.array_equal(s["status"], st) and np.array_equal(s["part"], run)
    for k in ("nodes", "open_left", "lvl_open", "nodes_start"):
        assert np.all(s[k] == 0), k
    assert np.all(s["prev_start"] == -1) and s["counters"].tolist() == [0] * 5
    assert np.array_equal(s["xlo"], lo) and np.array_equal(s["xhi"], hi)
    assert ("xplo" in s) == relaxed and ("pbudget" in s) == escalate
    if relaxed:
        wide = np.zeros(n0, F)
        wide[list(ra)] = tau
        assert np.array_equal(s["xplo"], lo - wide) and np.array_equal(s["xphi"], hi + wide)
    if escalate:
        assert np.all(s["pbudget"] == 77) and np.all(s["prob"] == 0)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 700])
def test_bab_finish_mark_unknown_and_set_status(cuda, P):
    rng = np.random.default_rng(P)
    st = rng.integers(0, 5, P).astype(np.int8)
    nodes, left = rng.integers(0, 1000, P).astype(np.int32), rng.integers(0, 99, P).astype(np.int32)
    d_st = to_dev(cuda, st)
    out = host(hip.bab_finish(d_st, to_dev(cuda, nodes), to_dev(cuda, left)))
    assert np.array_equal(out, np.stack([st.astype(np.int32), nodes, left]))
    # set_status on an index list: only those entries change
    idx = rng.choice(P, max(1, P // 3), replace=False).astype(np.int32)
    hip.set_status(to_dev(cuda, idx), d_st, ST_SAT)
    want = st.copy()
    want[idx] = ST_SAT
    assert np.array_equal(host(d_st), want)
    # mark_unknown over a node list with repeats: RUNNING / STOPPING partitions among them only
    part = rng.choice(P, max(1, P // 2)).astype(np.int32)
    hip.mark_unknown(to_dev(cuda, part), d_st)
    hit = np.zeros(P, bool)
    hit[part] = True
    want2 = np.where(hit & np.isin(want, (ST_RUNNING, ST_STOPPING)), ST_UNKNOWN, want).astype(np.int8)
    assert np.array_equal(host(d_st), want2)
    assert P < 200 or (np.any(want2 != want) and np.any(~hit & np.isin(want, (ST_RUNNING, ST_STOPPING))))


def test_bindings_reject_unknown_and_missing_keys(cuda):
    from fairify_amd.ops import ext

    with pytest.raises(TypeError, match="unexpected keyword argument 'bogus'"):
        ext().mark_unknown(part=1, n=0, status=1, stream=0, bogus=1)
    with pytest.raises(TypeError, match="missing required keyword argument"):
        ext().settle(P=3, stream=0)
    with pytest.raises(TypeError, match="missing required keyword argument"):
        ext().split_level(Nn=1, n0=5, stream=0)
    c, _ = boundary_case(5, 7)
    state, bufs = dev_state(cuda, c), new_buffers(cuda, c)
    state["status"] = state["status"].to(torch.int32)
    with pytest.raises(ValueError, match="status"):
        launch(cuda, c, state, bufs)
