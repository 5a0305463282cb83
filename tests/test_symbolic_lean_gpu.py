"""The lean row body of the register-resident symbolic kernel (csrc/symbolic.hip): the mask-free row
loop, the row prologue under node-row expansion and the status filter, the lane-parallel store of
the logit forms, and the per-instance launch geometry.  Everything is compared bitwise, never to a
tolerance.  The prefetching row loop exists only in the shaped instances, so every prologue case is
compared with the same launch under FAIRIFY_SYM_SHAPED=0: the run-time-shape kernel, whose plain loop
loads each row's box when the row starts.  An error in which row's box or status is fetched ahead
cannot cancel there.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import ext
from fairify_amd.ops import hip as H
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
WIDE = (13, [100, 100])        # AC-4: shaped 7-tile instance, one 512-thread workgroup per CU
MID = (13, [50])               # AC-3: shaped 4-tile instance, 256-thread workgroups
TINY = (13, [17, 3])           # partial tiles, no shaped instance


def _boxes(n0, R, seed, fold, span=6):
    g = np.random.default_rng(seed)
    lo = g.integers(-5, 20, size=(R, n0)).astype(np.float32)
    hi = lo + g.integers(0, span, size=(R, n0)).astype(np.float32)
    for d in fold:
        hi[:, d] = lo[:, d]
    return torch.from_numpy(lo), torch.from_numpy(hi)


def _outs(r):
    return dict(out_lb=r.out_lb, out_ub=r.out_ub, Lc=r.Lc, Uc=r.Uc, L0=r.L0, U0=r.U0, Le=r.Le, Ue=r.Ue,
                lay_lb=r.lay_lb_full, lay_ub=r.lay_ub_full)


def _same(a, b, rows=None):
    for k, x in _outs(a).items():
        y = _outs(b)[k]
        if rows is not None:
            x, y = x[rows], y[rows]
        assert torch.equal(x, y), k


@contextlib.contextmanager
def _plain_loop():
    """Launches inside take the run-time-shape kernels (read per launch)."""
    old = os.environ.get("FAIRIFY_SYM_SHAPED")
    os.environ["FAIRIFY_SYM_SHAPED"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["FAIRIFY_SYM_SHAPED"]
        else:
            os.environ["FAIRIFY_SYM_SHAPED"] = old


_BE = {}


def _backend(cuda, n0, hidden):
    key = (n0, tuple(hidden))
    if key not in _BE:
        _BE[key] = Backend(random_mlp(n0, hidden, seed=n0 + len(hidden), bias_scale=0.3), cuda)
    return _BE[key]


# ------------------------------------------------------------------------------------------------
# mask-free row loop
@pytest.mark.parametrize("n0,hidden", [(13, [100, 100]), (13, [64, 32, 16, 8, 4]), (13, [50]), TINY])
def test_launch_without_masks_is_the_masked_launch_with_an_empty_mask(cuda, monkeypatch, n0, hidden):
    fold = (8,)
    be = _backend(cuda, n0, hidden)
    lo, hi = _boxes(n0, 700, 9, fold)
    lo, hi = lo.to(cuda), hi.to(cuda)
    free = H.bounds(be, lo, hi, keep_layers=True, fold=fold, dead_out=False)
    assert free.dead is None
    zero = torch.zeros(700, be.n_hidden, dtype=torch.bool, device=cuda)
    masked = H.bounds(be, lo, hi, keep_layers=True, fold=fold, dead=zero)
    _same(free, masked)
    # a real mask: the masked path is the run-time-shape kernel's, shaped or not
    dm = (torch.rand(700, be.n_hidden, generator=torch.Generator().manual_seed(1)) < 0.2).to(cuda)
    res = []
    for shaped in ("1", "0"):
        monkeypatch.setenv("FAIRIFY_SYM_SHAPED", shaped)
        res.append(H.bounds(be, lo, hi, keep_layers=True, fold=fold, dead=dm))
    _same(res[0], res[1])
    assert torch.equal(res[0].dead_u8, res[1].dead_u8)
    assert not torch.equal(res[0].out_ub, masked.out_ub)      # the mask does act


# ------------------------------------------------------------------------------------------------
# row prologue: node-row expansion, row counts around one grid sweep, status filter
def _sweep(be, fold):
    g = ext().sym_geometry(H._net(be), H._fold_mask(fold, be.n0))
    assert g is not None
    return g["cus"] * g["blocks_per_cu"] * g["rows_per_block"]


def _expanded(lo, hi, pa, values):
    """The V rows of every box written out: row b * V + v is box b with its PA dims at values[v]."""
    V = values.shape[0]
    lo2 = lo.repeat_interleave(V, dim=0).clone()
    hi2 = hi.repeat_interleave(V, dim=0).clone()
    for k, d in enumerate(pa):
        col = values[:, k].repeat(lo.shape[0])
        lo2[:, d] = col
        hi2[:, d] = col
    return lo2, hi2


PA_CASES = [((8,), [[0.0], [1.0]]), ((3, 8), [[0.0, 0.0], [1.0, 2.0]])]
_ROWS = {}


def _case(cuda, shape, pa_case, nodes):
    """Boxes, their expansion and the unfiltered bounds of `nodes` nodes, from the shaped instance
    and from the run-time-shape kernel: computed once per case."""
    key = (shape[0], tuple(shape[1]), pa_case, nodes)
    if key not in _ROWS:
        pa, vals = PA_CASES[pa_case]
        be = _backend(cuda, *shape)
        lo, hi = _boxes(shape[0], nodes, 3 + nodes % 7, ())
        values = torch.tensor(vals, dtype=torch.float32)
        lo2, hi2 = _expanded(lo, hi, pa, values)
        lo, hi, values = lo.to(cuda), hi.to(cuda), values.to(cuda)
        full = H.bounds(be, lo, hi, keep_layers=True, dead_out=False, V=values.shape[0], pa=pa, values=values,
                        fill=SENTINEL)
        with _plain_loop():
            plain = H.bounds(be, lo, hi, keep_layers=True, dead_out=False, V=values.shape[0], pa=pa, values=values,
                             fill=SENTINEL)
        _ROWS[key] = (be, pa, values, lo, hi, lo2.to(cuda), hi2.to(cuda), full, plain)
    return _ROWS[key]


@pytest.mark.parametrize("pa_case", [0, 1])
@pytest.mark.parametrize("shape,nodes", [(TINY, 1), (TINY, 2), (TINY, 3), (WIDE, 1), (WIDE, 3), (MID, 2), (TINY, None),
                                         (WIDE, None), (MID, None)])
def test_node_row_expansion_is_the_explicit_rows(cuda, shape, nodes, pa_case):
    """V rows per node with the PA dims taken from `values`: bitwise the plain loop's launch and the
    launch of the rows written out, for 2, 4 and 6 rows and for more than two grid sweeps (a wave
    bounds at least three rows, two of them from prefetched boxes)."""
    be = _backend(cuda, *shape)
    pa, vals = PA_CASES[pa_case]
    V = len(vals)
    if nodes is None:
        nodes = (2 * _sweep(be, pa) + 5 * V) // V + 1
    be, pa, values, lo, hi, lo2, hi2, full, plain = _case(cuda, shape, pa_case, nodes)
    assert full.out_lb.shape[0] == nodes * V
    assert ext().sym_shaped(H._net(be), H._fold_mask(pa, be.n0)) == (shape != TINY)
    _same(full, plain)
    explicit = H.bounds(be, lo2, hi2, keep_layers=True, dead_out=False, fold=pa)
    _same(full, explicit)
    for t in _outs(full).values():
        assert not bool((t == SENTINEL).any())


@pytest.mark.parametrize("shape", [WIDE, MID])
@pytest.mark.parametrize("rows", [1, 2, 3, None])
def test_plain_rows_are_the_plain_loops(cuda, shape, rows):
    """No node-row expansion (V = 0): 1, 2, 3 rows and an odd count above two grid sweeps, shaped
    instance against the run-time-shape kernel."""
    fold = (8,)
    be = _backend(cuda, *shape)
    if rows is None:
        rows = 2 * _sweep(be, fold) + 3
    lo, hi = _boxes(shape[0], rows, 11, fold)
    lo, hi = lo.to(cuda), hi.to(cuda)
    new = H.bounds(be, lo, hi, keep_layers=True, dead_out=False, fold=fold, fill=SENTINEL)
    with _plain_loop():
        old = H.bounds(be, lo, hi, keep_layers=True, dead_out=False, fold=fold, fill=SENTINEL)
    _same(new, old)
    for t in _outs(new).values():
        assert not bool((t == SENTINEL).any())


def _patterns(nodes, sweep_nodes):
    run = {}
    run["none"] = np.zeros(nodes, bool)
    run["all"] = np.ones(nodes, bool)
    run["alternating"] = np.arange(nodes) % 2 == 0
    run["first"] = np.arange(nodes) == 0
    run["last"] = np.arange(nodes) == nodes - 1
    run["first_skipped"] = np.arange(nodes) != 0
    run["last_skipped"] = np.arange(nodes) != nodes - 1
    long = np.ones(nodes, bool)
    long[3:3 + sweep_nodes + 2] = False            # a skipped run longer than one sweep, live rows around it
    run["long_run"] = long
    return run


@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "first", "last", "first_skipped", "last_skipped",
                                     "long_run"])
@pytest.mark.parametrize("shape", [TINY, WIDE, MID])
def test_status_filter_skips_rows_and_leaves_the_others_alone(cuda, shape, pattern):
    pa_case = 0
    V = 2
    be = _backend(cuda, *shape)
    sweep_nodes = _sweep(be, PA_CASES[pa_case][0]) // V
    nodes = 2 * sweep_nodes + 11
    be, pa, values, lo, hi, _, _, _, plain = _case(cuda, shape, pa_case, nodes)
    running = _patterns(nodes, sweep_nodes)[pattern]
    # one partition per node, plus statuses of both "bounded" kinds (3, 4) and of decided ones
    g = np.random.default_rng(5)
    status = np.where(running, g.choice([3, 4], size=nodes), g.choice([0, 1, 2, 5], size=nodes)).astype(np.int8)
    part = g.permutation(nodes).astype(np.int32)
    st = torch.from_numpy(status[np.argsort(part)]).to(cuda)      # status[part[node]] = status of the node
    res = H.bounds(be, lo, hi, keep_layers=True, dead_out=False, V=V, pa=pa, values=values, fill=SENTINEL,
                   skip_status=st, skip_part=torch.from_numpy(part).to(cuda))
    rows = torch.from_numpy(np.repeat(running, V)).to(cuda)
    _same(res, plain, rows)          # running rows: the plain loop's unfiltered launch
    for k, t in _outs(res).items():
        assert bool((t[~rows] == SENTINEL).all()), k


# ------------------------------------------------------------------------------------------------
# logit forms
@pytest.mark.parametrize("n0,hidden,fold", [
    (13, [100, 100], (8,)), (13, [100, 100], (3, 8)), (13, [100], ()),       # AC-4, AC-2: n0 = 13
    (13, [64, 32, 16, 8, 4], ()),                                            # two column tiles
    (16, [64, 32, 16, 8, 4], (0,)), (16, [64, 32, 16, 8, 4], (0, 15)),       # BM-8: n0 = 16
    (16, [64, 32, 16, 8, 4], ()), (20, [50], (11,)), (13, [16, 8], (8,))])   # ... 20 inputs; the paired kernel
def test_logit_forms_are_the_run_time_shape_kernels(cuda, monkeypatch, n0, hidden, fold):
    """Both kernels store the forms with the 16-lane group, so their bitwise equality pins the shaped
    instance's column arithmetic only; what is independent of that store is the check against the
    CPU reference (1e-4: the reference rounds otherwise), the exact zeros on folded dims, and the
    sentinel (every entry written exactly by some lane)."""
    be = _backend(cuda, n0, hidden)
    lo, hi = _boxes(n0, 300, 4, fold)
    lo, hi = lo.to(cuda), hi.to(cuda)
    res = []
    for shaped in ("1", "0"):
        monkeypatch.setenv("FAIRIFY_SYM_SHAPED", shaped)
        res.append(H.bounds(be, lo, hi, fold=fold, fill=SENTINEL))
    a, b = res
    keep = [d for d in range(n0) if d not in fold]
    for x, y in ((a.Lc, b.Lc), (a.Uc, b.Uc)):
        assert torch.equal(x, y)
        assert not bool((x == SENTINEL).any())                 # every column written
        if fold:
            assert bool((x[:, list(fold)] == 0).all())
        assert bool((x[:, keep] != 0).any(dim=0).all())           # no coefficient column lost
    # the forms are the logit's: concretised over the box they enclose the reference bounds
    cpu = Backend(be.mlp, "cpu").bounds(lo.cpu(), hi.cpu(), mode="symbolic")
    kept = torch.tensor(keep)
    for C_g, C_c in ((a.Lc, cpu.Lc), (a.Uc, cpu.Uc)):
        tol = 1e-4 * float(C_c.abs().max() + 1)
        assert torch.allclose(C_g.cpu()[:, kept], C_c[:, kept], rtol=1e-4, atol=tol)


# ------------------------------------------------------------------------------------------------
# launch geometry
@pytest.mark.parametrize("n0,hidden", [(13, [100, 100]), (13, [64, 32, 16, 8, 4]), (13, [100]), (13, [64, 64]),
                                       (13, [50])])
def test_wide_shaped_instances_fit_lds_and_the_register_file(cuda, n0, hidden):
    be = _backend(cuda, n0, hidden)
    g = ext().sym_geometry(H._net(be), H._fold_mask((8,), n0))
    assert g is not None and g["shaped"]
    assert g["threads"] % 64 == 0 and g["threads"] <= 1024
    assert g["blocks_per_cu"] >= 1
    assert g["blocks_per_cu"] * g["lds_bytes"] <= 160 * 1024
    resident = -(-g["blocks_per_cu"] * (g["threads"] // 64) // 4)      # waves per SIMD of a full CU
    # the register limit (amdgpu_waves_per_eu: at least that many waves fit) is one the file can hold,
    # and the grid reaches the occupancy it was chosen for
    vgpr_limit = (512 // g["waves_per_simd"]) // 8 * 8
    assert g["waves_per_simd"] * vgpr_limit <= 512
    assert resident >= g["waves_per_simd"]
    # ... and the waves the grid places fit the file with what the instance really allocates
    if g["regs"] > 0:          # registers per lane, where the runtime reports them
        assert g["regs"] <= vgpr_limit
        assert resident * (-(-g["regs"] // 8) * 8) <= 512
