"""ReLU-phase branch-and-bound on the residue of the input-split search (stage ``relu``).

The input-split BaB (engine/bab.py) closes a node when its bounds certify it; on the narrow,
deep zero-bias networks (AC-8 13-5-5-1, AC-12 5x9 of the random-init bench) a third of the
partitions never close that way: the logit is EXACTLY 0 on a large region (every path to it
dead) and the violation needs ``N(x) < 0 < N(x')`` strictly, so any relaxation slack at the
boundary of that region -- a hypersurface through the box -- keeps nodes open however far the box
is split.  The reference decides these with Z3, whose exact simplex case-splits the ReLU
``If``s (utils/verif_utils.py:525-528, src/AC/Verify-AC.py:146-158).  This stage does the GPU
analogue:

* a node is (partition, ordered PA pair (v, v'), input box, ReLU phase of each neuron of the two
  network copies N(., v) and N(., v')); one tree per ordered pair (splits made for one pair do not
  multiply another's tree);
* bounds: forward symbolic bounds with the phases fixed (ops/reference.py:bounds ``phase``: a
  neuron fixed inactive outputs 0, one fixed active has the identity as its upper relaxation), then
  backward bounds concretised at EVERY layer with exact zeros kept (ops/reference.py:crown_phase);
* the node closes when copy v is provably >= 0 or copy v' provably <= 0 on the branch region
  (rigorous, exact zeros count), when a fixed phase contradicts the bounds (empty region), or by
  the coupled pair certificate ``min_t max_x t(-L_v(x)) + (1-t) U_v'(x) <= 0`` over the shared
  input box;
* branching: the bound (lower of N_v or upper of N_v') closest to closing, split at the unstable
  neuron whose chord intercept it pays most (BaBSR-like); when no unstable neuron is left, an
  input split (box halves) -- single lattice points are decided exactly, so the search is complete;
* every node's LP-optimal vertex pair is evaluated rigorously and confirmed exactly on the host
  (engine/exact.py): SAT answers are real counterexamples of the original network.

Every UNSAT is a proof from rigorous fp32 bounds (Higham gamma terms, outward rounding): this is
the sound replacement of the floating-point HiGHS MILP UNSAT (smt/milp.py) for these networks.
CPU measurement on the dumped residue (tools/exp/relu_proto.py): AC-8 38/40 closed with 6
nodes, AC-12 40/40 with a median of 34 nodes; AC-7 needs more (wide layers, no exact zeros).

The torch path here (state ``_PhaseSearch``; bound, certify, candidate and branch steps) is the reference
semantics (CPU tests); on the GPU the native runtime (csrc/relu_runtime.cpp + csrc/relu.hip) runs the same
algorithm.  The verdict arrays, confirmation, PA-group scatter and orientation merge are engine/search.py's.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from ..models.mlp import MLP
from ..ops import reference as ref
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from ..utils.timer import NULL, StageTimer
from . import exact
from .search import (RUNNING, UNKNOWN, UNSAT, BaBResult, Verdicts, clamp_tau, confirm_pairs, halve,
                     merge_orientations, pa_groups, pa_table, pool_overflow, solve_pa_groups, tau_apart)


@dataclass
class ReluConfig:
    node_budget: int = 2048          # nodes per partition (all its pair trees together)
    batch_nodes: int = 32768         # nodes bounded per sub-batch (torch path: per level)
    time_budget: float = 1e9         # wall-clock seconds for the whole call
    max_pool: int = 1 << 22          # live nodes (more: the partitions losing nodes end UNKNOWN)
    # native runtime: hidden-layer bounds of every node tightened by back-substitution with its
    # fixed phases (csrc/refine.hip; a refined bound contradicting a fixed phase proves the node's
    # region empty); "auto" = BaBConfig.refine's rule.  Default off: on the bench (AC-11 is the
    # only refine-eligible net the stage runs on) it decided 3 partitions per step fewer at +3-8 %
    # step time, and on the trained AC-7 residue it closed none either way
    # (profiles/r4/relu_refine.md)
    refine: str = os.environ.get("FAIRIFY_RELU_REFINE", "off")
    # relaxed queries on the native runtime: both orientations as roots of ONE search (the reverse
    # orientation's nodes read the negated logit's forms, csrc/relu.hip) with the two solves' budgets
    # pooled, instead of a second search on the negated network for the partitions the first closed
    merge_orient: bool = os.environ.get("FAIRIFY_RELU_MERGE", "1") != "0"


def supported(q: ResolvedQuery) -> bool:
    """PA-only and relaxed queries (|x_r - x'_r| <= tau on the RA dims, x' unclipped: the nodes then
    carry a second box for the x' RA coordinates, and the second orientation runs on the negated
    network; see :meth:`ReluBaBSolver.solve`)."""
    return True


def negated(mlp: MLP) -> MLP:
    """The network with its logit negated (last layer's weights and bias): N_A > 0 > N_B on ``mlp``
    is N_A < 0 < N_B on the result -- the second orientation of a relaxed query, where x' may leave
    the box so swapping the pair does not cover it."""
    ws = [w.copy() for w in mlp.weights]
    bs = [b.copy() for b in mlp.biases]
    ws[-1] = -ws[-1]
    bs[-1] = -bs[-1]
    return MLP(ws, bs, name=mlp.name + "-neg")


def certify_pair(LA_c, LA_0, MA, UB_c, UB_0, MB, lo, hi, free, unit):
    """Coupled pair certificate of nodes with one ordered pair each.

    Violation needs L_A(x) - eL <= N_A(x) < 0 and 0 < N_B(x) <= U_B(x) + eU on the shared box;
    the node is clean if some t in [0, 1] gives  max_x t (-L_A(x)) + (1 - t) U_B(x) <= 0  (forms
    given with their errors folded into the constants: LA_0 = L0 - eL, UB_0 = U0 + eU; MA / MB =
    magnitudes for the rounding margin).  Returns (g* [N], t* [N], vertex x* [N, n0])."""
    N, n0 = lo.shape
    dt = lo.dtype
    A = -LA_c * free
    A0 = -LA_0
    B = UB_c * free
    B0 = UB_0
    den = A - B
    tb = torch.where(den.abs() > 0, -B / torch.where(den.abs() > 0, den, torch.ones_like(den)),
                     torch.full_like(den, -1.0)).clamp(-1.0, 2.0)
    ts = torch.cat([torch.zeros(N, 1, dtype=dt, device=lo.device), torch.ones(N, 1, dtype=dt, device=lo.device),
                    tb], dim=1).clamp(0.0, 1.0)                                   # [N, T]
    t = ts[:, :, None]
    cs = t * A[:, None, :] + (1 - t) * B[:, None, :]                             # [N, T, n0]
    val = torch.maximum(cs * lo[:, None, :], cs * hi[:, None, :]).sum(-1)
    g = val + ts * A0[:, None] + (1 - ts) * B0[:, None]
    g = g + ref.gamma(2 * n0 + 4, unit) * (ts * MA[:, None] + (1 - ts) * MB[:, None]) + 8 * unit * (MA + MB)[:, None]
    gmin, targ = g.min(dim=1)
    tstar = ts.gather(1, targ[:, None])[:, 0]
    c = tstar[:, None] * A + (1 - tstar[:, None]) * B
    xstar = torch.where(c > 0, hi, lo)
    return gmin, tstar, xstar


def certify_pair_relaxed(LA_c, LA_0, MA, UB_c, UB_0, MB, lo, hi, plo, phi, shared, ra, unit):
    """:func:`certify_pair` for relaxed queries: copy A reads x, copy B reads x with the RA dims
    replaced by x' (their own box [plo, phi]).  Shared dims (``shared``: non-PA, non-RA) couple the
    copies as before; on an RA dim the two maxima are taken separately (x_r in [lo, hi], x'_r in
    [plo, phi]) -- the tie |x_r - x'_r| <= tau is dropped, which only loosens the bound.  Returns
    (g*, t*, x*, x'* on the RA dims)."""
    N, n0 = lo.shape
    dt = lo.dtype
    A = -LA_c
    B = UB_c
    As, Bs = A * shared, B * shared
    den = As - Bs
    tb = torch.where(den.abs() > 0, -Bs / torch.where(den.abs() > 0, den, torch.ones_like(den)),
                     torch.full_like(den, -1.0)).clamp(-1.0, 2.0)
    ts = torch.cat([torch.zeros(N, 1, dtype=dt, device=lo.device), torch.ones(N, 1, dtype=dt, device=lo.device),
                    tb], dim=1).clamp(0.0, 1.0)                                   # [N, T]
    t = ts[:, :, None]
    cs = t * As[:, None, :] + (1 - t) * Bs[:, None, :]
    val = torch.maximum(cs * lo[:, None, :], cs * hi[:, None, :]).sum(-1)
    ar = A[:, ra][:, None, :] * t                                                 # [N, T, nra]
    br = B[:, ra][:, None, :] * (1 - t)
    val = val + torch.maximum(ar * lo[:, None, ra], ar * hi[:, None, ra]).sum(-1) \
        + torch.maximum(br * plo[:, None, :], br * phi[:, None, :]).sum(-1)
    g = val + ts * LA_0[:, None].neg() + (1 - ts) * UB_0[:, None]
    g = g + ref.gamma(2 * n0 + 4, unit) * (ts * MA[:, None] + (1 - ts) * MB[:, None]) + 8 * unit * (MA + MB)[:, None]
    gmin, targ = g.min(dim=1)
    tstar = ts.gather(1, targ[:, None])[:, 0]
    c = tstar[:, None] * A + (1 - tstar[:, None]) * B
    xstar = torch.where(c > 0, hi, lo)
    xstar[:, ra] = torch.where(A[:, ra] > 0, hi[:, ra], lo[:, ra])
    xpstar = torch.where(B[:, ra] > 0, phi, plo)
    return gmin, tstar, xstar, xpstar


def _pick_form(res_c, res_0, res_e, fw_low, cr):
    """Per row, the tighter of the forward form (res_c, res_0, res_e; its bound fw_low) and the
    backward input form ``cr`` = (coef, const, err, low)."""
    lam, c, err, low = cr
    use = (low >= fw_low)[:, None]
    return (torch.where(use, lam, res_c), torch.where(use[:, 0], c, res_0), torch.where(use[:, 0], err, res_e))


class _PhaseSearch:
    """State of the torch level loop over one PA group: the PA table, the free / shared input dims, the
    verdicts and the pool, a root per (RUNNING partition, ordered pair).  A node: partition, pair, x box,
    x' box of the RA dims [N, len(ra)] (no columns unless relaxed), phases of the two copies [N, 2, Nh]."""
    POOL = ("part", "pair", "lo", "hi", "plo", "phi", "phase")

    def __init__(self, sol: "ReluBaBSolver", lo_np, hi_np, v: Verdicts, values_np, pairs_np):
        dev, dt, q = sol.dev, sol.be.dtype, sol.q
        self.v, self.lo_np, self.hi_np = v, lo_np, hi_np
        self.pa, self.relaxed, self.tau = list(q.pa_idx), q.relaxed, float(q.tau)
        self.ra = list(q.ra_idx) if q.relaxed else []
        self.values = torch.from_numpy(values_np).to(dev, dt)
        self.pairs = torch.from_numpy(pairs_np).to(dev)
        self.free = torch.ones(lo_np.shape[1], dtype=dt, device=dev)
        self.free[self.pa] = 0
        self.shared = self.free.clone()
        self.shared[self.ra] = 0
        run, Pp = np.nonzero(v.status == RUNNING)[0], pairs_np.shape[0]
        self.part = torch.from_numpy(np.repeat(run, Pp)).to(dev)
        self.pair = torch.arange(Pp, device=dev).repeat(len(run))
        self.lo = torch.from_numpy(lo_np).to(dev, dt)[self.part]
        self.hi = torch.from_numpy(hi_np).to(dev, dt)[self.part]
        # relaxed: the x' coordinates of the RA dims, unclipped, [lo - tau, hi + tau]
        none = torch.zeros(len(self.part), 0, dtype=dt, device=dev)
        self.plo = (self.lo[:, self.ra] - self.tau) if q.relaxed else none
        self.phi = (self.hi[:, self.ra] + self.tau) if q.relaxed else none
        self.phase = torch.zeros(len(self.part), 2, sol.be.n_hidden, dtype=torch.int8, device=dev)

    def keep(self, sel) -> None:
        for k in self.POOL:
            setattr(self, k, getattr(self, k)[sel])

    def running(self) -> torch.Tensor:
        return torch.from_numpy(self.v.status == RUNNING).to(self.part.device)[self.part]


class ReluBaBSolver:
    def __init__(self, backend: Backend, query: ResolvedQuery, cfg: ReluConfig, timer: StageTimer = NULL):
        self.be, self.q, self.cfg, self.tm = backend, query, cfg, timer
        self.dev = backend.device
        self.stats = {}

    def solve(self, lo_np: np.ndarray, hi_np: np.ndarray, mlp_exact: MLP,
              init_status: Optional[np.ndarray] = None) -> BaBResult:
        """Relaxed queries: orientation N(x, v) < 0 < N(x', v') on this backend's network, then, on the
        partitions it closed, N(x, v) > 0 > N(x', v') as the first orientation of the NEGATED network
        (:func:`negated`); a partition is UNSAT when both close, SAT when either finds a pair (always
        confirmed exactly on ``mlp_exact``, whose violation test is orientation-free)."""
        t0 = time.time()
        v = Verdicts(*lo_np.shape, init_status)
        if not supported(self.q):
            return v.close_running(UNKNOWN).result()
        r1 = solve_pa_groups(pa_groups(self.q, lo_np, hi_np), lo_np, hi_np, v.status, self.cfg.time_budget, t0,
                             lambda g, st, left: self._solve_group(lo_np[g], hi_np[g], mlp_exact, st, left))
        if not self.q.relaxed or getattr(self, "_second", False) or self._merged():
            return r1

        def second(st2):
            # four fields of this config only: refine and merge_orient take their environment defaults
            c = self.cfg
            cfg = ReluConfig(node_budget=c.node_budget, batch_nodes=c.batch_nodes, max_pool=c.max_pool,
                             time_budget=max(0.0, c.time_budget - (time.time() - t0)))
            neg = ReluBaBSolver(Backend(negated(self.be.mlp), device=self.dev), self.q, cfg, timer=self.tm)
            neg._second = True
            return neg.solve(lo_np, hi_np, mlp_exact, init_status=st2)

        return merge_orientations(r1, v.status, second, t0)

    def _native(self) -> bool:
        torch_rx = self.q.relaxed and os.environ.get("FAIRIFY_RELU_RELAXED_TORCH") == "1"
        return self.be.hip and os.environ.get("FAIRIFY_TORCH_BAB") != "1" and not torch_rx

    def _merged(self) -> bool:
        """Relaxed query, both orientations in the native runtime's one search."""
        return self.q.relaxed and self.cfg.merge_orient and self._native()

    # ------------------------------------------------------------------------------------------
    def _solve_group(self, lo_np, hi_np, mlp_exact, status, time_budget) -> BaBResult:
        values_np, pairs_np = pa_table(self.q, lo_np, hi_np)
        # the native runtime (csrc/relu_runtime.cpp) on the GPU, PA-only and relaxed queries alike
        # (relaxed: an x' RA box per node; the second orientation is solve()'s negated network);
        # FAIRIFY_TORCH_BAB=1: the torch orchestration (the reference semantics of the CPU tests)
        # (FAIRIFY_RELU_RELAXED_TORCH=1: relaxed queries only, the A/B of the native relaxed path)
        if self._native():
            return self._solve_native(lo_np, hi_np, mlp_exact, status, values_np, pairs_np, time_budget)
        return self._solve_torch(lo_np, hi_np, mlp_exact, status, values_np, pairs_np, time_budget)

    def _solve_torch(self, lo_np, hi_np, mlp_exact, status, values_np, pairs_np, time_budget) -> BaBResult:
        t0, cfg = time.time(), self.cfg
        v = Verdicts(*lo_np.shape, status)
        if pairs_np.shape[0] == 0:
            return v.close_running(UNSAT).result()
        s = _PhaseSearch(self, lo_np, hi_np, v, values_np, pairs_np)
        levels, timed_out = 0, False
        while s.part.numel():
            if time.time() - t0 > time_budget:
                timed_out = True
                break
            levels += 1
            alive = s.running()
            if s.relaxed:      # x_r and x'_r boxes more than tau apart: no admissible pair, node closed
                alive &= ~tau_apart(s.lo[:, s.ra], s.hi[:, s.ra], s.plo, s.phi, s.tau)
            if not bool(alive.all()):
                s.keep(alive)
                if s.part.numel() == 0:
                    break
            np.add.at(v.nodes, s.part.cpu().numpy(), 1)
            bd = self._bound(s)
            open_, tstar, xstar, xpstar = self._certify(s, bd)
            self._candidates(s, bd, torch.nonzero(open_).flatten(), xstar, xpstar, mlp_exact)
            # ---- leaves: the non-PA box (and the x' RA box) is a single lattice point -> decided
            # exactly above
            width = ((s.hi - s.lo) * s.free).amax(dim=1)
            if s.relaxed:
                width = torch.maximum(width, (s.phi - s.plo).amax(dim=1))
            grow = open_ & ~(width == 0) & s.running()
            if not bool(grow.any()):
                break       # no time-out: whatever is RUNNING has no open node left and closes UNSAT
            # ---- budget: a partition past its node budget with open nodes ends UNKNOWN
            over = torch.from_numpy(v.nodes >= cfg.node_budget).to(self.dev)[s.part] & grow
            if bool(over.any()):
                v.status[np.unique(s.part[over].cpu().numpy())] = UNKNOWN
                grow = grow & ~over
            self._branch(s, bd, torch.nonzero(grow).flatten(), tstar)
            if s.part.numel() > cfg.max_pool:
                pool_overflow(s.part, cfg.max_pool, v.status)
                s.keep(slice(cfg.max_pool))
        v.sweep(s.part.cpu().numpy() if timed_out else ())
        self.stats = {"levels": levels}         # (per group: the last group's)
        return v.result()

    def _bound(self, s: _PhaseSearch) -> SimpleNamespace:
        """Phase-fixed bounds of both copies of every node (rows 2k: copy A = N(., v), 2k + 1: copy B = N(., v')):
        logit bounds of all rows, copy A's lower and copy B's upper input form, the nodes they close."""
        be, pa, ra = self.be, s.pa, s.ra
        dt, N = be.dtype, s.part.numel()
        vA, vB = s.pairs[s.pair, 0], s.pairs[s.pair, 1]
        rlo, rhi = s.lo.repeat_interleave(2, dim=0), s.hi.repeat_interleave(2, dim=0)
        rv = torch.stack([vA, vB], dim=1).reshape(-1)
        rlo[:, pa] = s.values[rv]
        rhi[:, pa] = s.values[rv]
        if s.relaxed:          # copy B reads x' on the RA dims
            rlo[1::2, ra] = s.plo
            rhi[1::2, ra] = s.phi
        rph = s.phase.reshape(2 * N, be.n_hidden)
        with self.tm("relu.bounds"):
            res = be.bounds(rlo, rhi, mode="symbolic", keep_layers=True, phase=rph)
            pc, forms = be.crown_phase(rlo, rhi, res, rph)
        if forms is None:
            # HIP kernel: logit bounds intersected, infeasible rows set to (+inf, -inf) and the
            # tighter input forms written into ``res`` in place
            olb, oub = res.out_lb.to(dt), res.out_ub.to(dt)
            LA, UB = (res.Lc, res.L0, res.Le), (res.Uc, res.U0, res.Ue)
        else:
            olb = torch.maximum(res.out_lb.to(dt), pc.low[:, 0].to(dt))
            oub = torch.minimum(res.out_ub.to(dt), -pc.low[:, 1].to(dt))
            inf = res.infeasible
            if inf is None:
                inf = torch.zeros(2 * N, dtype=torch.bool, device=self.dev)
            olb = torch.where(inf, torch.full_like(olb, float("inf")), olb)
            oub = torch.where(inf, torch.full_like(oub, -float("inf")), oub)
            # coupled certificate on the input forms (the tighter of forward / backward per row)
            LA = _pick_form(res.Lc, res.L0, res.Le, res.out_lb, forms[1.0])
            lamU, cU, eU, lowU = forms[-1.0]
            UB = _pick_form(res.Uc, res.U0, res.Ue, -res.out_ub, (-lamU, -cU, eU, lowU))
        A, B = slice(0, None, 2), slice(1, None, 2)
        return SimpleNamespace(vA=vA, vB=vB, pc=pc, olb=olb, oub=oub, closed=(olb[A] >= 0) | (oub[B] <= 0),
                               LAc=LA[0][A], LA0=LA[1][A], LAe=LA[2][A], UBc=UB[0][B], UB0=UB[1][B], UBe=UB[2][B])

    def _certify(self, s: _PhaseSearch, bd: SimpleNamespace):
        """The coupled pair certificate: (open mask, t*, the vertex x* and, relaxed, x'* on the RA dims)."""
        pa, ra, free, values, unit = s.pa, s.ra, s.free, s.values, self.be.unit
        LAc, LA0, LAe, UBc, UB0, UBe = bd.LAc, bd.LA0, bd.LAe, bd.UBc, bd.UB0, bd.UBe
        # fold the PA coordinates (fixed per row) into the constants
        fa_A = (LAc[:, pa] * values[bd.vA]).sum(1)
        fa_B = (UBc[:, pa] * values[bd.vB]).sum(1)
        mxb = torch.maximum(s.lo.abs(), s.hi.abs())
        mxb_b = mxb.clone()
        if s.relaxed:
            mxb_b[:, ra] = torch.maximum(s.plo.abs(), s.phi.abs())
        # rounding margin over the folded PA products' magnitudes (with several PA dims their
        # sum can cancel below the products' errors)
        MA = (LAc.abs() * mxb * free).sum(1) + (LA0 - LAe).abs() + (LAc[:, pa] * values[bd.vA]).abs().sum(1)
        MB = (UBc.abs() * mxb_b * free).sum(1) + (UB0 + UBe).abs() + (UBc[:, pa] * values[bd.vB]).abs().sum(1)
        xpstar = None
        if s.relaxed:
            g, tstar, xstar, xpstar = certify_pair_relaxed(LAc * free, LA0 - LAe + fa_A, MA, UBc * free,
                                                           UB0 + UBe + fa_B, MB, s.lo, s.hi, s.plo, s.phi, s.shared,
                                                           ra, unit)
        else:
            g, tstar, xstar = certify_pair(LAc, LA0 - LAe + fa_A, MA, UBc, UB0 + UBe + fa_B, MB, s.lo, s.hi, free, unit)
        return ~bd.closed & (g > 0), tstar, xstar, xpstar

    def _candidates(self, s: _PhaseSearch, bd: SimpleNamespace, oi: torch.Tensor, xstar, xpstar, mlp_exact) -> None:
        """Candidate vertex pairs of the open nodes ``oi``: rigorous point bounds, then the exact check."""
        if not oi.numel():
            return
        xa, xb = xstar[oi].clone(), xstar[oi].clone()
        xa[:, s.pa] = s.values[bd.vA[oi]]
        xb[:, s.pa] = s.values[bd.vB[oi]]
        if s.relaxed:      # x'_r: its vertex, pulled into [x_r - tau, x_r + tau]
            xb[:, s.ra] = clamp_tau(xpstar[oi], xa[:, s.ra], s.tau)
        with self.tm("relu.cand"):
            alb, _ = self.be.point_bounds(xa)
            _, bub = self.be.point_bounds(xb)
        poss = (alb < 0) & (bub > 0)
        ci = oi[poss]
        if ci.numel():
            confirm_pairs(s.v, self.q, s.lo_np, s.hi_np, mlp_exact, s.part[ci].cpu().numpy(), xa[poss], xb[poss])

    def _branch(self, s: _PhaseSearch, bd: SimpleNamespace, gi: torch.Tensor, tstar) -> None:
        """Next level, two children per node of ``gi``: a phase split of the bound closest to closing at its
        best neuron, or, where no unstable neuron is left, an input split."""
        dev, n0, ra = self.dev, s.lo.shape[1], s.ra
        A, B = slice(0, None, 2), slice(1, None, 2)
        gapA, gapB = -bd.olb[A][gi], bd.oub[B][gi]
        sA, sB = bd.pc.split[A, 0][gi], bd.pc.split[B, 1][gi]
        useA = (sA >= 0) & ((gapA <= gapB) | (sB < 0))
        useB = ~useA & (sB >= 0)
        relu = useA | useB
        row = torch.where(useA, torch.zeros_like(sA), torch.ones_like(sA))
        neu = torch.where(useA, sA, sB)
        ri = gi[relu]
        cp, k = s.phase[ri].repeat(2, 1, 1), ri.numel()
        cp[torch.arange(2 * k, device=dev), row[relu].repeat(2), neu[relu].repeat(2)] = torch.cat(
            [torch.full((k,), -1, dtype=torch.int8, device=dev), torch.ones(k, dtype=torch.int8, device=dev)])
        # input split along the dim of largest |coefficient| x width of the certificate at t*
        # (relaxed: the x' RA dims compete as extra columns, scored by copy B's coefficient)
        ii = gi[~relu]
        c_t = tstar[ii, None] * (-bd.LAc[ii]) + (1 - tstar[ii, None]) * bd.UBc[ii]
        if s.relaxed:
            c_t[:, ra] = tstar[ii, None] * bd.LAc[ii][:, ra]
        w = (s.hi[ii] - s.lo[ii]) * s.free
        sc = torch.where(w > 0, c_t.abs() * w + 1e-9 * w, torch.full_like(w, -1.0))
        if s.relaxed:
            wp = s.phi[ii] - s.plo[ii]
            cp_ = (1 - tstar[ii, None]) * bd.UBc[ii][:, ra]
            sc = torch.cat([sc, torch.where(wp > 0, cp_.abs() * wp + 1e-9 * wp, torch.full_like(wp, -1.0))], dim=1)
        d = sc.argmax(dim=1)
        ar = torch.arange(ii.numel(), device=dev)
        onx = d < n0
        lo1, hi1, lo2, hi2 = halve(s.lo[ii], s.hi[ii], ar[onx], d[onx])
        plo1, phi1, plo2, phi2 = halve(s.plo[ii], s.phi[ii], ar[~onx], d[~onx] - n0)
        s.part = torch.cat([s.part[ri], s.part[ri], s.part[ii], s.part[ii]])
        s.pair = torch.cat([s.pair[ri], s.pair[ri], s.pair[ii], s.pair[ii]])
        s.lo, s.hi = torch.cat([s.lo[ri], s.lo[ri], lo1, lo2]), torch.cat([s.hi[ri], s.hi[ri], hi1, hi2])
        s.plo, s.phi = torch.cat([s.plo[ri], s.plo[ri], plo1, plo2]), torch.cat([s.phi[ri], s.phi[ri], phi1, phi2])
        s.phase = torch.cat([cp, s.phase[ii], s.phase[ii]])

    # ------------------------------------------------------------------------------------------
    def _runtime(self, values_np: np.ndarray, pairs_np: np.ndarray, n_root: int):
        """Native (C++/HIP) ReLU-phase runtime checked out of the backend's pool (engine/rtpool.py)."""
        from ..ops import ext
        from ..ops.hip import _net
        from .rtpool import checkout

        from .bab import refine_level

        rf = min(1, refine_level(self.cfg.refine, self.be.widths))
        ra = list(self.q.ra_idx) if self.q.relaxed else []
        tau = float(self.q.tau) if self.q.relaxed else 0.0
        no = 2 if self._merged() else 1
        key = (tuple(self.q.pa_idx), values_np.tobytes(), pairs_np.tobytes(), int(self.cfg.batch_nodes), rf,
               tuple(ra), tau, no)

        def make(cap):
            return ext().ReluRuntime(_net(self.be), self.be.flat.data_ptr(), list(self.q.pa_idx),
                                     values_np.astype(np.float32).reshape(-1).tolist(),
                                     pairs_np.astype(np.int64).reshape(-1).tolist(), int(cap),
                                     int(self.cfg.batch_nodes), float(self.be.unit), rf, ra, tau, no, self.be.flat)

        return checkout(self.be, "_relu_rt", key, max(self.cfg.max_pool, 2 * n_root), make)

    def _solve_native(self, lo_np, hi_np, mlp_exact, status, values_np, pairs_np, time_budget):
        from ..ops import ext
        from ..ops.hip import _net

        v = Verdicts(*lo_np.shape, status)
        if not ext().relu_fits(_net(self.be)):
            # the phase kernel cannot hold this network (a layer > 256 wide or > 160 KB of LDS):
            # the stage is skipped, its partitions stay UNKNOWN for the later stages
            return v.close_running(UNKNOWN).result()
        no = 2 if self._merged() else 1
        n_root = int((status == RUNNING).sum()) * max(1, pairs_np.shape[0]) * no
        if pairs_np.shape[0] == 0:
            return v.close_running(UNSAT).result()
        confirm = exact.make_confirm(mlp_exact, lo_np, hi_np, self.q)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        with self.tm("relu.native"), self._runtime(values_np, pairs_np, n_root) as rt:
            st, cx, cxp, nodes, stats = rt.solve(lo_np.astype(np.float32), hi_np.astype(np.float32), status,
                                                 int(self.cfg.node_budget) * no, float(time_budget), confirm, stream)
        self.stats = dict(stats)
        return BaBResult(np.asarray(st, dtype=np.int8), np.asarray(cx), np.asarray(cxp),
                         np.asarray(nodes, dtype=np.int64))
