"""beta-CROWN ReLU-phase branch-and-bound (stage ``beta``; bounding in ops/beta.py, csrc/beta.hip).

The residue of the wide, deep networks (trained AC-7: 64-32-16-8-4) is what the input-split BaB
(engine/bab.py) and the interval-clamping ReLU-phase stage (engine/relu_bab.py) leave: its UNSAT
partitions need ReLU case splits that act as constraints on the input region, which is how Z3
decides them in the reference (utils/verif_utils.py:525-528, src/AC/Verify-AC.py:146-158) and how
the host verified LP (smt/lpbab.py) does, at ~2 s per partition per CPU worker.  Here every node
(partition, ordered PA pair, box, phases of both copies) is bounded on the GPU by the
Lagrangian (beta) bound of ops/beta.py with optimised slopes / split multipliers, warm-started from
its parent; a rigorous fp64 re-evaluation decides.

Search: one tree per (partition, ordered PA pair) in a FIFO node pool processed in batches (the
first batch of roots with ``root_iters`` optimisation steps, the rest with ``iters``); a node
closes when its bound is >= 0 (no pair with N(x, va) < 0 < N(x, vb) in its region: f_t < 0 on any
such pair), its concretising vertex pair is screened with rigorous point bounds and confirmed exactly
on the host (SAT), a single lattice point is decided exactly, and a partition whose nodes all
closed is UNSAT.  A partition past its node budget ends UNKNOWN.

Relaxed queries (|x_r - x'_r| <= tau, x' unclipped): every node also carries x''s box on the RA
dims, split like the input dims, and its orientation: N(x, va) < 0 < N(x', vb) or the reverse (x' may
leave the box, so the swapped pair does not cover the second one); both orientations are roots of the
same search (the objective's sign per node).  CPU tests pin verdicts to brute-force enumeration
(tests/test_beta_bab.py); the GPU kernel to this module's reference (tests/test_beta_gpu.py).  ``_roots`` builds
the roots for both the native runtime and the torch loop (``_torch_level``); the host layer is engine/search.py.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from ..models.mlp import MLP
from ..ops import beta as B
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from ..utils.timer import NULL, StageTimer
from . import exact
from .relu_bab import negated
from .search import (RUNNING, UNKNOWN, UNSAT, BaBResult, Verdicts, clamp_tau, confirm_pairs, merge_orientations,
                     pa_groups, pa_table, pool_overflow, solve_pa_groups, tau_apart)


@dataclass
class BetaConfig:
    node_budget: int = 512           # nodes per partition (all its pair trees together; x Pp / 2)
    iters: int = 128                 # optimisation steps per node (warm-started from the parent); 128 over
    #                                  64: relaxed/BM BM-8 residue 48 vs 33 of 200 at 1 024 nodes with pgap
    root_iters: int = 400            # ... per root node
    lr_a: float = 0.1                # Adam step of the slopes alpha
    lr_b: float = 0.5                # ... of the split multipliers beta
    lr_t: float = 0.1                # ... of the pair weight t
    child_lr: float = 0.3            # children (warm-started at their parent's optimum): lr x this
    decay: float = 0.98              # lr decay per step
    warm_beta: bool = True           # split multiplier starts at the parent's relaxation (else 0)
    lookahead: int = 8               # filtered branching: candidates per score (0 = best gap score)
    tighten: bool = True             # children: re-bound every hidden neuron over the node's box and
    #                                  phase region (csrc/refine.hip with phases), intersected with
    #                                  the inherited bounds; an empty region closes the node
    probe_levels: int = 0            # > 0: a partition that has expanded 2 x this many nodes per pair
    #                                  tree with none of its trees closed ends UNKNOWN (a residue the
    #                                  stage does not converge on costs little; per partition, so the
    #                                  verdicts do not depend on how partitions are grouped or sharded)
    beta_pos: bool = True            # split multipliers projected >= 0 (free-signed ones, which may
    #                                  use the interval side, make Adam oscillate around 0: measured
    #                                  8 / 10 -> 0 / 10 trained AC-7 partitions closed, tools/exp)
    batch_nodes: int = 32768         # nodes per level launch
    time_budget: float = 1e9         # wall-clock seconds for the whole call
    max_pool: int = 1 << 21          # live nodes (more: the partitions losing nodes end UNKNOWN)
    branch: str = "pgap"             # "pgap": the verified LP's rule (largest primal gap h - relu(z)) at the
    #                                  averaged primal iterate of the node's optimisation (kernel-side;
    #                                  with lookahead > 0 it supplies the first candidate list);
    #                                  "kernel": |lambda| x relaxation gap at the vertex x* (round 5);
    #                                  "lpgap" (experiment): the chord slack at the vertex x* / x'*
    pgap_weights: int = 1            # branch "pgap": iterate weights of the primal average (1 uniform, 2 it + 1,
    #                                  3 second half of the steps)
    input_every: int = 0             # > 0 (experiment): every this many levels of a tree, split the
    #                                  widest input dim (x, or x''s RA dims) instead of the kernel's choice
    native: bool = True              # HIP device: the level loop in the native runtime (csrc/beta_runtime.cpp,
    #                                  device-resident pool / budgets / probe); FAIRIFY_TORCH_BETA=1 or the
    #                                  experiments (lpgap, input_every, merge_orient off): this module's loop
    feas_iters: int = int(os.environ.get("FAIRIFY_BETA_FEAS", "64"))
    #                                  > 0: children left open after their optimisation get an infeasibility
    #                                  pass of this many steps (the phase constraints' Lagrangian alone,
    #                                  ops/beta.py:feasibility_ref) -- the verified LP closes most of its
    #                                  tree as infeasible regions two or three phase splits deep
    batched: bool = os.environ.get("FAIRIFY_BETA_BATCHED", "0") == "1"
    #                                  HIP device: the two-phase level -- the optimisation steps on MFMA, 16
    #                                  nodes per wave (csrc/beta_opt16.hip), then the per-node kernel at
    #                                  iters = 0 (rigorous bound, branching).  Used when the network fits
    #                                  the batched kernel (a static choice per network and config, never per
    #                                  level: verdicts do not depend on grouping); the infeasibility pass
    #                                  stays per node (unless batched_feas); the CPU backend runs the torch
    #                                  reference unchanged
    batched_feas: bool = os.environ.get("FAIRIFY_BETA_BATCHED_FEAS", "0") == "1"
    #                                  with ``batched`` in effect: the infeasibility pass in two phases too --
    #                                  the feas mode of the batched optimiser proposes the phase multipliers,
    #                                  16 nodes per wave, and the per-node kernel at iters = 0 closes a node
    #                                  when the rigorous fp64 value at them is > 0 (sound whatever is
    #                                  proposed).  Static per (network, config) like ``batched``
    trees: tuple = ()                # experiment: only the trees (ordered-pair row, orientation) listed
    sign_prune: bool = True          # close the (pair, orientation) trees a per-value logit sign test settles
    #                                  before their roots are bounded
    merge_orient: bool = True        # relaxed: both orientations as roots of ONE search (per-node sign of
    #                                  the objective, ops/beta.py:evaluate osg) instead of a second solve on
    #                                  the negated network for the partitions the first one closed


def supported(q: ResolvedQuery) -> bool:
    """PA-only and relaxed queries (x' RA box per node, second orientation on the negated net)."""
    return True


def fits(be: Backend) -> bool:
    """The kernel's shape limits (inputs <= 64, weights within LDS); the torch reference has none."""
    if not be.hip:
        return True
    from ..ops import ext
    from ..ops.hip import _net

    return bool(ext().beta_fits(_net(be)))


class BetaBaBSolver:
    def __init__(self, backend: Backend, query: ResolvedQuery, cfg: BetaConfig, timer: StageTimer = NULL):
        self.be, self.q, self.cfg = backend, query, cfg
        # the kernels' flags word holds the weights in two bits (ops/hip.py:beta_flags): a larger value
        # would read as the infeasibility pass's bit
        if not 0 <= int(cfg.pgap_weights) <= 3:
            raise ValueError(f"BetaConfig.pgap_weights must be 0, 1, 2 or 3, got {cfg.pgap_weights!r}")
        self.tm = timer
        self.dev = backend.device
        self.stats = {}

    def solve(self, lo_np: np.ndarray, hi_np: np.ndarray, mlp_exact: MLP,
              init_status: Optional[np.ndarray] = None) -> BaBResult:
        """Relaxed queries: N(x, v) < 0 < N(x', v') on this backend's network, then, on the partitions
        that closed, N(x, v) > 0 > N(x', v') as the same search on the network with its logit
        negated (x' may leave the box, so swapping the pair does not cover it); UNSAT when both
        close, SAT when either finds a pair (confirmed on ``mlp_exact``, orientation-free)."""
        t0 = time.time()
        v = Verdicts(*lo_np.shape, init_status)
        if not supported(self.q) or self.be.n_hidden == 0 or not fits(self.be):
            return v.close_running(UNKNOWN).result()     # before either orientation is solved
        self.stats = {"levels": 0, "nodes": 0}
        r1 = solve_pa_groups(pa_groups(self.q, lo_np, hi_np), lo_np, hi_np, v.status, self.cfg.time_budget, t0,
                             lambda g, st, left: self._solve_group(lo_np[g], hi_np[g], mlp_exact, st, left))
        if not self.q.relaxed or getattr(self, "_second", False) or self.cfg.merge_orient:
            return r1

        def second(st2):
            # this config with the time left; the second solver's nodes and levels count as this one's
            neg = BetaBaBSolver(Backend(negated(self.be.mlp), device=self.dev), self.q,
                                replace(self.cfg, time_budget=max(0.0, self.cfg.time_budget - (time.time() - t0))),
                                timer=self.tm)
            neg._second = True
            r2 = neg.solve(lo_np, hi_np, mlp_exact, init_status=st2)
            self.stats["nodes"] += neg.stats.get("nodes", 0)
            self.stats["levels"] += neg.stats.get("levels", 0)
            return r2

        return merge_orientations(r1, v.status, second, t0)

    # ------------------------------------------------------------------------------------------
    def _root_bounds(self, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor, widen: bool = False):
        """Rigorous per-layer pre-activation bounds [P * V, NH] of every (partition, PA value) row
        (the verified LP's bounds, smt/milp.py:layer_bounds_rows, kept on the device); ``widen``:
        the x' rows of a relaxed query (RA dims widened by tau, unclipped)."""
        be, q = self.be, self.q
        P, n0 = lo.shape
        V = values.shape[0]
        pa = list(q.pa_idx)
        rlo = lo.repeat_interleave(V, dim=0)
        rhi = hi.repeat_interleave(V, dim=0)
        vv = values.repeat(P, 1)
        rlo[:, pa] = vv
        rhi[:, pa] = vv
        if widen and q.relaxed:
            ra = list(q.ra_idx)
            rlo[:, ra] -= q.tau
            rhi[:, ra] += q.tau
        rf = len(be.widths) - 1 >= 2        # refined hidden bounds: every relaxation above layer 0 tightens
        res = be.bounds(rlo, rhi, mode="symbolic", keep_layers=True, crown=rf, refine=rf)
        NH = be.n_hidden
        lb = torch.cat([t.float() for t in res.layer_lb], 1)[:, :NH].contiguous()
        ub = torch.cat([t.float() for t in res.layer_ub], 1)[:, :NH].contiguous()
        self._logit = (res.out_lb, res.out_ub)          # [P * V] rigorous logit bounds of the rows
        return lb, ub

    def _solve_group(self, lo_np, hi_np, mlp_exact, status, time_budget) -> BaBResult:
        t0 = time.time()
        v = Verdicts(*lo_np.shape, status)
        s = self._roots(lo_np, hi_np, mlp_exact, v)
        if s is None:
            return v.result()
        if self._use_native(s.O):
            return self._solve_native(s, max(0.0, time_budget - (time.time() - t0)))
        levels, timed_out = 0, False         # the torch loop; stats accumulate over the groups of a call
        while s.pool["part"].numel():
            if time.time() - t0 > time_budget:
                timed_out = True
                break
            # drop nodes of decided / over-budget partitions, and (relaxed) nodes whose x and x'
            # RA boxes are more than tau apart (no admissible pair left)
            pool, ra = s.pool, s.ra
            alive = torch.from_numpy(v.status == RUNNING).to(self.dev)[pool["part"]]
            if s.relaxed:
                alive &= ~tau_apart(pool["lo"][:, ra], pool["hi"][:, ra], pool["plo"][:, ra], pool["phi"][:, ra], s.tau)
            if not bool(alive.all()):
                s.pool = {kk: t[alive] for kk, t in pool.items()}
                if not s.pool["part"].numel():
                    break
            levels += 1
            self._torch_level(s)
        v.sweep(s.pool["part"].cpu().numpy() if timed_out else ())
        self.stats["levels"] = self.stats.get("levels", 0) + levels
        self.stats["nodes"] = self.stats.get("nodes", 0) + int(v.nodes.sum())
        return v.result()

    def _roots(self, lo_np, hi_np, mlp_exact, v: Verdicts) -> Optional[SimpleNamespace]:
        """Root construction of one PA group, for the native and the torch path: PA table, root bounds, sign
        prune, the ``pool`` (a root per running partition, ordered pair, orientation), ``tree_run`` /
        ``pre_closed`` for the probe, ``budget``.  None: the group is decided without a search (in ``v``)."""
        be, q, cfg, dev = self.be, self.q, self.cfg, self.dev
        (P, n0), NH = lo_np.shape, be.n_hidden
        values_np, pairs_np = pa_table(q, lo_np, hi_np)
        run, Pp = np.nonzero(v.status == RUNNING)[0], pairs_np.shape[0]
        if Pp == 0:
            v.close_running(UNSAT)
        if Pp == 0 or run.size == 0:
            return None
        relaxed, tau = q.relaxed, float(q.tau)
        ra = list(q.ra_idx) if relaxed else []
        ram = torch.zeros(n0, dtype=torch.bool, device=dev)
        ram[ra] = True
        f32 = dict(dtype=torch.float32, device=dev)
        values = torch.from_numpy(values_np.astype(np.float32)).to(dev)
        V = values.shape[0]
        # orientations per ordered pair: relaxed queries with merge_orient carry both as roots
        O = 2 if (relaxed and cfg.merge_orient) else 1
        lo_r = torch.from_numpy(lo_np[run].astype(np.float32)).to(dev)
        hi_r = torch.from_numpy(hi_np[run].astype(np.float32)).to(dev)
        with self.tm("beta.roots"):
            rlb, rub = self._root_bounds(lo_r, hi_r, values)
            olx = self._logit
            rlbp, rubp = self._root_bounds(lo_r, hi_r, values, widen=True) if relaxed else (rlb, rub)
            olp = self._logit if relaxed else olx
        # one root per (running partition, ordered pair, orientation)
        k = torch.arange(run.size, device=dev).repeat_interleave(Pp * O)
        pr = torch.from_numpy(pairs_np.astype(np.int64)).to(dev).repeat_interleave(O, dim=0).repeat(run.size, 1)
        osg = torch.tensor([1, -1][:O], dtype=torch.int8, device=dev).repeat(run.size * Pp)
        ia, ib = k * V + pr[:, 0], k * V + pr[:, 1]
        # the loop this group runs on (tests / logs)
        self.stats.update(native=self._use_native(O), batched=self._batched(), batched_feas=self._batched_feas())
        if cfg.trees:        # experiment: one tree at a time (tools/exp/beta_vs_lp.py)
            jj = torch.arange(Pp, device=dev).repeat_interleave(O).repeat(run.size)
            sel = torch.zeros_like(k, dtype=torch.bool)
            for j_, o_ in cfg.trees:
                sel |= (jj == j_) & (osg == o_)
            k, pr, osg, ia, ib = k[sel], pr[sel], osg[sel], ia[sel], ib[sel]
        pre_closed = np.zeros(P, dtype=np.int32)
        if cfg.sign_prune:
            # per-value sign tests from the rows' rigorous logit bounds (the verified LP's shared sign
            # tests, smt/lpbab.py:solve_partition): a tree whose copy A can never have the sign its
            # orientation needs (N(x, va) < 0, or > 0 for the reverse) or whose copy B can never have
            # the opposite one is closed before its root is bounded -- a race query has 20 ordered
            # pairs x 2 orientations, most of them settled by one of 2 V such tests
            pos = osg > 0
            dead = torch.where(pos, (olx[0][ia] >= 0) | (olp[1][ib] <= 0), (olx[1][ia] <= 0) | (olp[0][ib] >= 0))
            keep = ~dead
            # the probe counts these trees as closed (progress on the partition)
            pre_closed = np.bincount(run[k[dead].cpu().numpy()], minlength=P).astype(np.int32)
            k, pr, osg, ia, ib = k[keep], pr[keep], osg[keep], ia[keep], ib[keep]
            self.stats["sign_pruned"] = self.stats.get("sign_pruned", 0) + int(dead.sum())
            if k.numel() == 0:
                v.status[run] = UNSAT
                return None
        R0, plo, phi = k.numel(), lo_r[k].clone(), hi_r[k].clone()
        if relaxed:                 # x' on the RA dims: [lo - tau, hi + tau], unclipped
            plo[:, ra] -= tau
            phi[:, ra] += tau
        pool = {
            "part": torch.from_numpy(run).to(dev)[k],
            "lo": lo_r[k].clone(), "hi": hi_r[k].clone(), "plo": plo, "phi": phi,
            "va": values[pr[:, 0]].clone(), "vb": values[pr[:, 1]].clone(),
            "LBA": rlb[ia], "UBA": rub[ia], "LBB": rlbp[ib], "UBB": rubp[ib],
            "phA": torch.zeros(R0, NH, dtype=torch.int8, device=dev),
            "phB": torch.zeros(R0, NH, dtype=torch.int8, device=dev),
            "alA": torch.full((R0, NH), 0.5, **f32), "alB": torch.full((R0, NH), 0.5, **f32),
            "beA": torch.zeros(R0, NH, **f32), "beB": torch.zeros(R0, NH, **f32),
            "t": torch.full((R0,), 0.5, **f32),
            "root": torch.ones(R0, dtype=torch.bool, device=dev),
            "depth": torch.zeros(R0, dtype=torch.int32, device=dev),
            # relaxed: Lagrange multipliers of the tie |x_r - x'_r| <= tau (RA dims)
            "gP": torch.zeros(R0, n0, **f32), "gM": torch.zeros(R0, n0, **f32),
            "tree": torch.arange(R0, device=dev),        # the (partition, ordered pair, orientation) root
            "osg": osg,
        }
        # node budget per partition, scaled with its ordered pairs (a multi-valued PA -- race: 20 pairs -- gets
        # the budget a binary one gets per pair) and orientations.  The probe (per partition: no verdict depends on
        # which partitions share the call): past 2 probe_levels nodes per pair tree, only if a tree has closed
        return SimpleNamespace(v=v, lo_np=lo_np, hi_np=hi_np, mlp_exact=mlp_exact, pool=pool, R0=R0, O=O, NH=NH,
                               pa=list(q.pa_idx), relaxed=relaxed, ra=ra, tau=tau, ram=ram,
                               tree_run=run[k.cpu().numpy()], pre_closed=pre_closed,
                               budget=int(cfg.node_budget * max(1.0, Pp / 2.0) * O),
                               probe_at=2 * cfg.probe_levels * Pp * O, probed=np.zeros(P, dtype=bool))

    def _level(self, s: SimpleNamespace, nd, is_root: bool, osg, **kw):
        """The bound kernel's call on the nodes ``nd`` (their parameters are updated in place)."""
        cfg = self.cfg
        sc = 1.0 if is_root else cfg.child_lr
        rx = (s.ram, nd["plo"], nd["phi"], s.tau, nd["gP"], nd["gM"]) if s.relaxed else None
        return self.be.beta_level(nd["lo"], nd["hi"], s.pa, nd["va"], nd["vb"], nd["LBA"], nd["UBA"], nd["LBB"],
                                  nd["UBB"], nd["phA"], nd["phB"], nd["alA"], nd["alB"], nd["beA"], nd["beB"], nd["t"],
                                  cfg.root_iters if is_root else cfg.iters, cfg.lr_a * sc, cfg.lr_b * sc,
                                  cfg.lr_t * sc, cfg.decay, cfg.lookahead, cfg.beta_pos, rx,
                                  pgap=cfg.pgap_weights if cfg.branch == "pgap" else 0, osg=osg, **kw)

    def _torch_level(self, s: SimpleNamespace) -> None:
        """One level on the pool's front batch: roots first (their own iteration count), then FIFO."""
        cfg, pool, v = self.cfg, s.pool, s.v
        nb = min(cfg.batch_nodes, pool["part"].numel())
        is_root = bool(pool["root"][0])
        if is_root:
            nb = min(nb, int(pool["root"].sum()))
        cur, rest = {kk: t[:nb] for kk, t in pool.items()}, {kk: t[nb:] for kk, t in pool.items()}
        np.add.at(v.nodes, cur["part"].cpu().numpy(), 1)
        lev, closed = self._bound(s, cur, is_root)
        self._candidates(s, cur, lev, torch.nonzero(~closed).flatten())
        kids = self._branch(s, cur, lev, closed)
        pool = {kk: torch.cat([rest[kk], kids[kk]]) for kk in pool}
        if cfg.probe_levels:
            self._probe(pool, v.nodes, s.probed, s.probe_at, s.R0, s.tree_run, v.status, s.pre_closed)
        if pool["part"].numel() > cfg.max_pool:
            lost = pool_overflow(pool["part"], cfg.max_pool, v.status)
            self.stats["pool_lost"] = self.stats.get("pool_lost", 0) + lost
            pool = {kk: t[:cfg.max_pool] for kk, t in pool.items()}
        s.pool = pool

    def _bound(self, s: SimpleNamespace, cur, is_root: bool):
        """The batch's bounds (children: after tightening their hidden bounds): level record, closed nodes."""
        cfg = self.cfg
        empty = None
        if cfg.tighten and not is_root:
            with self.tm("beta.tighten"):
                empty = self._tighten(cur, s.pa, s.ram if s.relaxed else None)
        with self.tm("beta.level"):
            lev = self._level(s, cur, is_root, cur["osg"] if s.O > 1 else None,
                              feas_iters=0 if is_root else cfg.feas_iters, feas_lr=(cfg.lr_a, cfg.lr_b, cfg.lr_t),
                              batched=self._batched(), batched_feas=self._batched_feas())
        if empty is not None:
            lev.bound = torch.where(empty, torch.full_like(lev.bound, float("inf")), lev.bound)
        nan = torch.isnan(lev.bound)
        if bool(nan.any()):
            # a node without a bound cannot close its tree: its partition stops (UNKNOWN), as in the
            # native loop (csrc/beta_bab.hip split kernel)
            bad = np.unique(cur["part"][nan].cpu().numpy())
            self.stats["nan_nodes"] = self.stats.get("nan_nodes", 0) + int(nan.sum())
            s.v.status[bad[s.v.status[bad] == RUNNING]] = UNKNOWN
        return lev, lev.bound >= 0

    def _candidates(self, s: SimpleNamespace, cur, lev, cand: torch.Tensor) -> None:
        """Vertex pairs of the nodes left open (and the lattice leaves): rigorous point screen, exact check."""
        if not cand.numel():
            return
        be, pa, ra = self.be, s.pa, s.ra
        xa = lev.xstar[cand].clone()
        xb = (lev.xpstar[cand] if lev.xpstar is not None else lev.xstar[cand]).clone()
        if s.relaxed:         # x'_r: its vertex, pulled into [x_r - tau, x_r + tau]
            xb[:, ra] = clamp_tau(xb[:, ra], xa[:, ra], s.tau)
        xa[:, pa] = cur["va"][cand]
        xb[:, pa] = cur["vb"][cand]
        with self.tm("beta.cand"):
            alb, aub = be.point_bounds(xa)
            blb, bub = be.point_bounds(xb)
        poss = (alb < 0) & (bub > 0)
        if s.O > 1:       # orientation -1: N(x, va) > 0 > N(x', vb)
            poss = torch.where(cur["osg"][cand] > 0, poss, (aub > 0) & (blb < 0))
        ci = cand[poss]
        if ci.numel():
            confirm_pairs(s.v, self.q, s.lo_np, s.hi_np, s.mlp_exact, cur["part"][ci].cpu().numpy(), xa[poss], xb[poss])

    def _branch(self, s: SimpleNamespace, cur, lev, closed: torch.Tensor):
        """Children of the open non-leaf nodes of running partitions within budget (past it: UNKNOWN)."""
        cfg, v, n0 = self.cfg, s.v, cur["lo"].shape[1]
        grow = ~closed & ~(lev.split == B.LEAF(n0))
        grow &= torch.from_numpy(v.status == RUNNING).to(self.dev)[cur["part"]]
        over = torch.from_numpy(v.nodes >= s.budget).to(self.dev)[cur["part"]] & grow
        if bool(over.any()):
            ob = np.unique(cur["part"][over].cpu().numpy())
            self.stats["over_budget"] = self.stats.get("over_budget", 0) + int((v.status[ob] == RUNNING).sum())
            v.status[ob] = UNKNOWN
            grow &= ~over
        gi = torch.nonzero(grow).flatten()
        bi = lev.binit[gi] if cfg.warm_beta else torch.zeros_like(lev.binit[gi])
        split = lev.split[gi]
        if cfg.branch == "lpgap" and gi.numel():
            ns = self._lp_gap_split(cur, gi, lev, s.pa, s.ra, s.tau, s.NH)
            moved = (split >= 0) & (ns >= 0) & (ns != split)
            split = torch.where(moved, ns, split)
            bi = torch.where(moved[:, None], torch.zeros_like(bi), bi)   # new neuron: beta from 0
        if cfg.input_every > 0 and gi.numel():
            split = self._force_input(cur, gi, split, s.pa, s.ra, n0, cfg.input_every)
        return self._children({kk: t[gi] for kk, t in cur.items()}, split, bi, s.NH, n0)

    def _batched(self) -> bool:
        """The two-phase level (BetaConfig.batched): on, a HIP device, and the network fits."""
        if not (self.cfg.batched and self.be.hip):
            return False
        from ..ops import hip

        return hip.beta_batched_fits(self.be)

    def _batched_feas(self) -> bool:
        """The two-phase infeasibility pass (BetaConfig.batched_feas): on, the two-phase level in effect
        and an infeasibility pass to run."""
        return bool(self.cfg.batched_feas and self.cfg.feas_iters > 0 and self._batched())

    def _use_native(self, O: int) -> bool:

        cfg = self.cfg
        return (self.be.hip and cfg.native and os.environ.get("FAIRIFY_TORCH_BETA") != "1"
                and cfg.branch in ("kernel", "pgap") and cfg.input_every == 0
                and (O == 2 or not self.q.relaxed))

    def _solve_native(self, s: SimpleNamespace, time_budget: float) -> BaBResult:
        """The level loop on the device (csrc/beta_runtime.cpp), started from the roots of ``s.pool``."""
        from ..ops import ext
        from ..ops.hip import _beta_wt, _net
        from .rtpool import checkout

        be, q, cfg = self.be, self.q, self.cfg
        pool, R0, status, lo_np, hi_np = s.pool, s.R0, s.v.status, s.lo_np, s.hi_np
        P = len(lo_np)
        relaxed, ra, tau = s.relaxed, s.ra, (s.tau if s.relaxed else 0.0)
        i32 = lambda x: x.to(torch.int32).contiguous()  # noqa: E731
        f32 = lambda x: x.to(torch.float32).contiguous()  # noqa: E731
        arrs = [i32(pool["part"]), pool["osg"].to(torch.int8).contiguous(), f32(pool["lo"]), f32(pool["hi"]),
                f32(pool["plo"]), f32(pool["phi"]), f32(pool["va"]), f32(pool["vb"]), f32(pool["LBA"]),
                f32(pool["UBA"]), f32(pool["LBB"]), f32(pool["UBB"]),
                torch.stack([pool["phA"], pool["phB"]], 1).to(torch.int8).contiguous(),
                torch.stack([pool["alA"], pool["alB"], pool["beA"], pool["beB"]], 1).contiguous(),
                f32(pool["t"]), torch.stack([pool["gP"], pool["gM"]], 1).contiguous()]
        ptrs = [a.data_ptr() for a in arrs]
        if not relaxed:
            ptrs[4] = ptrs[5] = ptrs[15] = 0
        tree_part = pool["part"].to(torch.int32).cpu().numpy()
        cfgd = {"iters": int(cfg.iters), "root_iters": int(cfg.root_iters), "lr_a": float(cfg.lr_a),
                "lr_b": float(cfg.lr_b), "lr_t": float(cfg.lr_t), "child_lr": float(cfg.child_lr),
                "decay": float(cfg.decay), "lookahead": int(cfg.lookahead), "beta_pos": int(bool(cfg.beta_pos)),
                "stall": 1, "pgap": int(cfg.pgap_weights) if cfg.branch == "pgap" else 0, "warm_beta": int(bool(cfg.warm_beta)),
                "tighten": int(bool(cfg.tighten)), "feas_iters": int(cfg.feas_iters),
                "batched": int(self._batched()), "batched_feas": int(self._batched_feas())}

        confirm = exact.make_confirm(s.mlp_exact, lo_np, hi_np, q)
        cap = int(max(cfg.max_pool, 2 * R0))
        batch = int(min(cfg.batch_nodes, 32768))
        key = (tuple(q.pa_idx), tuple(ra), tau, batch)

        def make(c):
            wt = _beta_wt(be)
            return ext().BetaRuntime(_net(be), be.flat.data_ptr(), wt.data_ptr(), list(q.pa_idx), ra, tau, int(c),
                                     batch, (be.flat, wt))

        stream = torch.cuda.current_stream(self.dev).cuda_stream
        with self.tm("beta.native"), checkout(be, "_beta_rt", key, cap, make) as rt:
            st, cx, cxp, nodes, stats = rt.solve(ptrs, int(R0), status.astype(np.int8), tree_part,
                                                 lo_np.astype(np.float32), hi_np.astype(np.float32), int(s.budget),
                                                 int(s.probe_at), float(time_budget), cfgd, confirm, stream,
                                                 s.pre_closed)
        stats = dict(stats)
        if os.environ.get("FAIRIFY_BETA_CHECK") and int(stats["levels"]) == 1 and \
                int((np.asarray(st) == UNSAT).sum()) == int((status == RUNNING).sum()) > 0:
            # diagnostics of a whole group closed at the root level (tools: exp W/X)
            c = lambda x: x.detach().cpu()  # noqa: E731
            lba, uba, lbb, ubb = c(pool["LBA"]), c(pool["UBA"]), c(pool["LBB"]), c(pool["UBB"])
            print(f"[beta-check] P={P} R0={R0} osg={np.unique(c(pool['osg']).numpy()).tolist()} "
                  f"ph_nnz={int((c(pool['phA']) != 0).sum() + (c(pool['phB']) != 0).sum())} "
                  f"crossedA={int((lba > uba).sum())} crossedB={int((lbb > ubb).sum())} "
                  f"nan={int(torch.isnan(lba).sum() + torch.isnan(uba).sum())} "
                  f"t={np.unique(c(pool['t']).numpy())[:4].tolist()} "
                  f"box_w={float((c(pool['hi']) - c(pool['lo'])).sum(1).min())} stats={stats}",
                  file=sys.stderr, flush=True)
            # the same roots through the loop's kernel call, fresh parameters (relaxed implies RA dims: mask s.ram)
            fresh = {**pool, **{kk: pool[kk].clone() for kk in ("alA", "alB", "beA", "beB", "t", "gP", "gM")}}
            lev = self._level(s, fresh, True, pool["osg"])
            b = lev.bound.cpu()
            print(f"[beta-check] torch-call root bounds: closed {int((b >= 0).sum())} of {b.numel()}, "
                  f"min {float(b.min()):.4g}", file=sys.stderr, flush=True)
        del arrs
        self.stats["levels"] = self.stats.get("levels", 0) + int(stats["levels"])
        self.stats["nodes"] = self.stats.get("nodes", 0) + int(stats["nodes"])
        for key in ("probe_stop", "nan_nodes", "root_skip_status", "root_skip_tau", "unclosed", "dev_next"):
            if stats.get(key):
                self.stats[key] = self.stats.get(key, 0) + int(stats[key])
        return BaBResult(np.asarray(st, dtype=np.int8), np.asarray(cx), np.asarray(cxp),
                         np.asarray(nodes, dtype=np.int64))

    def _probe(self, pool, nodes_np, probed, probe_at: int, R0: int, tree_run, status, pre_closed=None) -> None:
        """Partitions past the probe point with no closed pair tree end UNKNOWN (their nodes are
        dropped at the next level)."""
        cand = np.nonzero((nodes_np >= probe_at) & ~probed & (status == RUNNING))[0]
        if not cand.size:
            return
        probed[cand] = True
        alive = np.zeros(R0, dtype=bool)
        if pool["tree"].numel():
            alive[pool["tree"].cpu().numpy()] = True
        closed = np.bincount(tree_run[~alive], minlength=status.shape[0])
        if pre_closed is not None:
            closed = closed + pre_closed
        stop = cand[closed[cand] == 0]
        if stop.size:
            status[stop] = UNKNOWN
            self.stats["probe_stop"] = self.stats.get("probe_stop", 0) + int(stop.size)

    def _tighten(self, cur, pa, ram=None):
        """Phase-aware bounds of the batch's nodes (both copies in one launch pair; copy B over x',
        i.e. its RA dims over [plo, phi] when ``ram``), intersected in place with the bounds they
        inherited; returns the nodes whose region is empty."""
        R = cur["lo"].shape[0]
        loB, hiB = cur["lo"], cur["hi"]
        if ram is not None:
            loB = torch.where(ram[None], cur["plo"], cur["lo"])
            hiB = torch.where(ram[None], cur["phi"], cur["hi"])
        lo = torch.cat([cur["lo"], loB])
        hi = torch.cat([cur["hi"], hiB])
        v = torch.cat([cur["va"], cur["vb"]])
        lo[:, pa] = v
        hi[:, pa] = v
        ph = torch.cat([cur["phA"], cur["phB"]])
        lb, ub, inf = self.be.phase_layer_bounds(lo, hi, ph)
        lb, ub = lb.float(), ub.float()
        for k, (a, b) in (("LBA", (0, R)), ("LBB", (R, 2 * R))):
            cur[k].copy_(torch.maximum(cur[k], lb[a:b]))
        for k, (a, b) in (("UBA", (0, R)), ("UBB", (R, 2 * R))):
            cur[k].copy_(torch.minimum(cur[k], ub[a:b]))
        empty = torch.zeros(R, dtype=torch.bool, device=lo.device)
        if inf is not None:
            empty = inf[:R] | inf[R:]
        return empty

    @staticmethod
    def _children(nd, split, binit, NH: int, n0: int):
        """Two children per node: a phase split (split >= 0: copy A neuron split, copy B NH + j)
        inheriting the parent's parameters (the new multiplier from ``binit``: the child starts at
        the parent's bound), or an input split (split = -1 - d) halving x's dim d (d < n0) or x''s
        RA dim d - n0."""
        R = split.numel()
        dev = split.device
        rep = torch.arange(R, device=dev).repeat_interleave(2)
        kid = {kk: v[rep].clone() for kk, v in nd.items()}
        kid["root"][:] = False
        if "depth" in kid:
            kid["depth"] += 1
        if R == 0:
            return kid
        sp = split[rep]
        side = torch.arange(2 * R, device=dev) % 2             # 0: lower child, 1: upper child
        r_ = torch.arange(2 * R, device=dev)
        neu = sp >= 0
        sgn = torch.where(side == 0, -1, 1).to(torch.int8)
        inA = neu & (sp < NH)
        inB = neu & (sp >= NH)
        bi = binit[rep].gather(1, side[:, None])[:, 0]
        if bool(inA.any()):
            kid["phA"][r_[inA], sp[inA]] = sgn[inA]
            kid["beA"][r_[inA], sp[inA]] = bi[inA]
        if bool(inB.any()):
            kid["phB"][r_[inB], sp[inB] - NH] = sgn[inB]
            kid["beB"][r_[inB], sp[inB] - NH] = bi[inB]
        inp = ~neu
        for lk, hk, sel in (("lo", "hi", inp & (-1 - sp < n0)), ("plo", "phi", inp & (-1 - sp >= n0))):
            if not bool(sel.any()):
                continue
            d = (-1 - sp[sel]) % n0
            ri = r_[sel]
            lo_d = kid[lk][ri, d]
            hi_d = kid[hk][ri, d]
            mid = torch.floor((lo_d + hi_d) / 2)
            low_child = side[sel] == 0
            kid[hk][ri[low_child], d[low_child]] = mid[low_child]
            kid[lk][ri[~low_child], d[~low_child]] = mid[~low_child] + 1
        # (plo / phi are read on the RA dims only; x' shares x's box everywhere else)
        return kid

    def _lp_gap_split(self, cur, gi, lev, pa, ra, tau: float, NH: int):
        """Per node: the unfixed unstable neuron (either copy) with the largest chord slack
        u (z - l) / (u - l) - relu(z) at the node's vertex pair (x*, x'* on copy B's RA dims) -- the
        LP-BaB's branching rule evaluated at beta's concretising point; -1 if none."""
        be = self.be
        xa = lev.xstar[gi].clone().to(be.dtype)
        xb = (lev.xpstar[gi] if lev.xpstar is not None else lev.xstar[gi]).clone().to(be.dtype)
        if ra:
            xb[:, ra] = clamp_tau(xb[:, ra], xa[:, ra], tau)
        xa[:, pa] = cur["va"][gi].to(be.dtype)
        xb[:, pa] = cur["vb"][gi].to(be.dtype)
        scores = []
        for x, ph, LB, UB in ((xa, cur["phA"][gi], cur["LBA"][gi], cur["UBA"][gi]),
                              (xb, cur["phB"][gi], cur["LBB"][gi], cur["UBB"][gi])):
            h, off, sc = x, 0, []
            for W, b in zip(be.ws[:-1], be.bs[:-1]):
                z = h @ W + b
                w = z.shape[1]
                p_ = ph[:, off:off + w]
                l_, u_ = LB[:, off:off + w].to(z.dtype), UB[:, off:off + w].to(z.dtype)
                unst = (l_ < 0) & (u_ > 0) & (p_ == 0)
                chord = u_ * (z - l_) / torch.where(unst, u_ - l_, torch.ones_like(u_))
                sc.append(torch.where(unst, (chord - torch.relu(z)).clamp(min=0), torch.full_like(z, -1.0)))
                h = torch.where(p_ < 0, torch.zeros_like(z), torch.where(p_ > 0, z, torch.relu(z)))
                off += w
            scores.append(torch.cat(sc, 1))
        S = torch.cat(scores, 1)                       # [n, 2 NH]: copy A neurons, then copy B
        best, j = S.max(dim=1)
        return torch.where(best > 0, j, torch.full_like(j, -1)).to(lev.split.dtype)

    @staticmethod
    def _force_input(cur, gi, split, pa, ra, n0: int, every: int):
        """Nodes at depth = every - 1 (mod every) split their widest input dim: x's (code -1 - d)
        or x''s RA dims (code -1 - (n0 + d)); a node with no dim wider than a point keeps its split."""
        dep = cur["depth"][gi]
        sel = (dep % every) == (every - 1)
        if not bool(sel.any()):
            return split
        w = (cur["hi"][gi] - cur["lo"][gi]).clone()
        if pa:
            w[:, pa] = -1.0
        cols = [w]
        if ra:
            wp = torch.full_like(w, -1.0)
            wp[:, ra] = (cur["phi"][gi] - cur["plo"][gi])[:, ra]
            cols.append(wp)
        W = torch.cat(cols, dim=1)
        best, d = W.max(dim=1)
        use = sel & (best >= 1.0)
        return torch.where(use, (-1 - d).to(split.dtype), split)
