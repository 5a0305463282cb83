"""One group of a chunk's partitions (they share their protected-attribute range) on its way through
the verification stages: the state the stages share (:class:`GroupState`) and one function per stage.

``_verify_group`` is the sequence of the stage calls; ``engine/pipeline.py`` keeps the configuration,
the records and the chunk / model drivers.  Every stage takes the state and the configuration; the
order of the device calls, the synchronisations and the timer labels are the pipeline's contract
with the worker streams and the profile reports (docs/DESIGN.md, "Pipeline stages").
"""
from __future__ import annotations

import os
import sys
import time
from contextlib import contextmanager
from dataclasses import dataclass, replace
from typing import Dict, List, Optional

import numpy as np
import torch

from ..models.mlp import MLP
from ..ops import hip as H
from ..ops.reference import sample_points
from ..smt import lpbab, milp
from ..smt import solver as smt_solver
from ..smt.host import HostSMT
from ..utils import faults
from ..utils.timer import StageTimer
from . import exact
from . import prune as P_
from .bab import RUNNING, SAT, UNKNOWN, UNSAT, BaBConfig, BaBSolver
from .beta_bab import BetaBaBSolver, BetaConfig
from .beta_bab import supported as _beta_supported
from .falsify import residual_falsify
from .relu_bab import ReluBaBSolver, ReluConfig
from .relu_bab import supported as _relu_supported
from .search import pa_table
from .sim import simulate

# node expansions per stage (core["stage_nodes"] columns): input-split BaB with its escalation, the
# ReLU-phase BaB, the fixed beta pass, every anytime round, the heuristic retry
STAGE_NODE_COLS = ("bab", "relu", "beta", "anytime", "heuristic")
_HOST_SMT: Dict[tuple, object] = {}
_VERBOSE_ANYTIME = os.environ.get("FAIRIFY_VERBOSE_ANYTIME") == "1"


class GroupState:
    """What the stages of one partition group share: the boxes (host and device), the PA table, the
    verdict arrays the stages write, the node accounting and the clocks.

    On the GPU the device boxes are decoded from the ids by ``fa_decode_kernel`` (K1); the host
    keeps its own decode (``lo_np``/``hi_np``) for the exact confirmation of candidates."""

    def __init__(self, be, mlp: MLP, q, ids: np.ndarray, lo_np: np.ndarray, hi_np: np.ndarray, grid=None,
                 timer: Optional[StageTimer] = None):
        self.be, self.mlp, self.q = be, mlp, q
        self.tm = timer if timer is not None else StageTimer()
        self.t_start = time.time()
        self.ids, self.lo_np, self.hi_np = ids, lo_np, hi_np
        dev = self.dev = be.device
        self.sync = (lambda: torch.cuda.current_stream(dev).synchronize()) if dev.type == "cuda" else (lambda: None)
        self.values_np, self.pairs_np = pa_table(q, lo_np, hi_np)
        self.values = torch.from_numpy(self.values_np).to(dev)
        self.pairs = torch.from_numpy(self.pairs_np).to(dev)
        self.pids = torch.from_numpy(ids).to(dev)
        if be.hip and grid is not None:
            self.lo, self.hi = H.decode(grid, self.pids)
        else:
            self.lo = torch.from_numpy(lo_np).to(dev, torch.float32)
            self.hi = torch.from_numpy(hi_np).to(dev, torch.float32)
        Pn, n = lo_np.shape
        self.Pn, self.Nh = Pn, int(sum(mlp.hidden))
        self.status = np.full(Pn, RUNNING, dtype=np.int8)
        self.stage = np.array([""] * Pn, dtype=object)
        self.cex_x = np.zeros((Pn, n), dtype=np.int64)
        self.cex_xp = np.zeros((Pn, n), dtype=np.int64)
        self.nodes = np.zeros(Pn, dtype=np.int64)
        self.stage_nodes = np.zeros((Pn, len(STAGE_NODE_COLS)), dtype=np.int64)
        self.open_left: Optional[np.ndarray] = None     # open nodes the first pass left (native runtime)
        self.forced = np.zeros(Pn, dtype=bool)          # fault injection: solver "timeouts"
        self.budget = 0.0                               # BaB wall budget in seconds (first_pass sets it)
        self.times = dict(sim=0.0, prune=0.0, bab=0.0, heur=0.0, replay=0.0)
        # set by first_pass: which residue stages run, and the budget the input splitting has reached
        self.relu_on = self.beta_on = self.esc_after_relu = self.inline = False
        self.prev_budget = 0

    def unknown(self, with_forced: bool = False) -> np.ndarray:
        """Indices of the UNKNOWN partitions; the fault-injected ones only ``with_forced``."""
        return np.nonzero(self.status == UNKNOWN if with_forced else (self.status == UNKNOWN) & ~self.forced)[0]

    def left(self) -> float:
        """Seconds of the BaB wall budget still unspent."""
        return max(0.0, self.budget - (time.time() - self.t_start))

    def confirm(self, idx: np.ndarray, X: np.ndarray, XP: np.ndarray, stage_name: str) -> np.ndarray:
        """Candidate pairs (row k belongs to partition ``idx[k]``), rounded to the lattice: the ones
        that satisfy the pair constraints in their box and flip the network exactly become that
        partition's SAT verdict, witness and stage.  Returns the confirmed partitions."""
        X, XP = X.round().astype(np.int64), XP.round().astype(np.int64)
        q = self.q
        ok = exact.check_pair_constraints(X, XP, self.lo_np[idx], self.hi_np[idx], q.pa_idx, q.ra_idx, q.tau)
        viol = exact.is_violation(self.mlp, X, XP) & ok
        hit = idx[viol]
        self.status[hit] = SAT
        self.cex_x[hit], self.cex_xp[hit] = X[viol], XP[viol]
        self.stage[hit] = stage_name
        return hit

    def confirm_found(self, res, idx: np.ndarray, stage_name: str) -> None:
        """:meth:`confirm` for the device witnesses of a simulation / falsifier result over ``idx``."""
        found = res.found.cpu().numpy()
        if found.any():
            fi = np.nonzero(found)[0]
            self.confirm(idx[fi], res.wit_x[fi].cpu().numpy(), res.wit_xp[fi].cpu().numpy(), stage_name)

    def absorb(self, idx: np.ndarray, res, stage_name: str, open_left: bool = False) -> int:
        """Merge the ``BaBResult`` of a sub-solve on the partitions ``idx``: decided verdicts, their
        stage, SAT witnesses and the nodes of all of ``idx``; ``open_left``: also the frontier sizes
        (the escalation's gate).  Returns how many partitions it decided."""
        dec = np.isin(res.status, (SAT, UNSAT))
        hit = idx[dec]
        self.status[hit] = res.status[dec]
        self.stage[hit] = stage_name
        sat = res.status == SAT
        self.cex_x[idx[sat]] = res.cex_x[sat]
        self.cex_xp[idx[sat]] = res.cex_xp[sat]
        self.nodes[idx] += res.nodes
        if open_left and self.open_left is not None and res.open_left is not None:
            self.open_left = self.open_left.copy()
            self.open_left[idx] = res.open_left
        return int(dec.sum())

    @contextmanager
    def charging(self, col: int):
        """Charge the nodes expanded inside the block to column ``col`` of ``stage_nodes``."""
        before = self.nodes.copy()
        yield
        self.stage_nodes[:, col] += (self.nodes - before).astype(np.int64)

    @contextmanager
    def clock(self, name: str, sync: bool = True):
        """Add the block's wall time, to the end of its device work, to ``times[name]``."""
        t0 = time.time()
        yield
        if sync:
            self.sync()
        self.times[name] += time.time() - t0


@dataclass
class PruneStats:
    """Stage 2's outputs.  ``fused``: the HIP mask algebra ran (``code``); otherwise the PyTorch
    masks (``cand``, ``s_cand``, ``st_dead``).  The IBP layer bounds are None without sound_prune_stats."""
    fused: bool
    b_cnt: np.ndarray
    s_cnt: np.ndarray
    st_cnt: np.ndarray
    code: Optional[torch.Tensor] = None
    ibp_lb: Optional[torch.Tensor] = None
    ibp_ub: Optional[torch.Tensor] = None
    cand: Optional[torch.Tensor] = None
    s_cand: Optional[torch.Tensor] = None
    st_dead: Optional[torch.Tensor] = None


def sim_stage(s: GroupState, cfg):
    """Stage 1: simulation (profile + falsify); witnesses are confirmed exactly."""
    with s.clock("sim"):
        with s.tm("sim"):
            sim = simulate(s.be, s.q, s.lo, s.hi, s.pids, cfg.sim_size, cfg.seed, s.values, s.pairs, cfg.bisect_pairs,
                           cfg.bisect_steps)
        with s.tm("sim.confirm"):
            s.confirm_found(sim, np.arange(s.Pn), "sim")
    return sim


def prune_stage(s: GroupState, cfg, sim) -> PruneStats:
    """Stage 2: sound pruning statistics (IBP + symbolic on the partition box)."""
    be, widths, Nh = s.be, s.mlp.widths, s.Nh
    # stage 2 / 4 mask algebra in HIP kernels (FAIRIFY_FUSED_PRUNE=0: the PyTorch path, for A/B tests)
    fused = be.hip and cfg.sound_prune_stats and os.environ.get("FAIRIFY_FUSED_PRUNE", "1") != "0"
    with s.clock("prune"):
        if fused:
            with s.tm("prune.bounds"):
                ibp = be.bounds(s.lo, s.hi, mode="ibp", keep_layers=True)
                sym = be.bounds(s.lo, s.hi, mode="symbolic")
                code, pcnt = H.prune_masks(be, sim.counts, ibp.lay_ub_full, sym.dead_u8)
                pcnt_np = pcnt.cpu().numpy().astype(np.int64)
            return PruneStats(True, pcnt_np[:, 0], pcnt_np[:, 1], pcnt_np[:, 2], code=code, ibp_lb=ibp.lay_lb_full,
                              ibp_ub=ibp.lay_ub_full)
        cand, _ = P_.candidates_from_counts(sim.counts, cfg.sim_size)
        b_dead = torch.zeros(s.Pn, s.mlp.n_neurons, dtype=torch.bool, device=s.dev)
        s_dead = torch.zeros_like(b_dead)
        st_dead = torch.zeros_like(b_dead)
        s_cand = cand.clone()
        ibp_lb = ibp_ub = None
        if cfg.sound_prune_stats:
            with s.tm("prune.bounds"):
                ibp = be.bounds(s.lo, s.hi, mode="ibp", keep_layers=True)
                ibp_lb = torch.cat(ibp.layer_lb, dim=1)
                ibp_ub = torch.cat(ibp.layer_ub, dim=1)
                b_dead, b_rem = P_.bound_dead(cand, ibp_ub[:, :Nh], widths)
                b_dead = P_.ensure_one_alive(b_dead, widths)
                sym = be.bounds(s.lo, s.hi, mode="symbolic")
                s_hid = b_rem[:, :Nh] & sym.dead
                s_dead = torch.zeros_like(b_dead)
                s_dead[:, :Nh] = s_hid
                s_cand = b_rem.clone()
                s_cand[:, :Nh] = b_rem[:, :Nh] & ~s_hid
                st_dead = P_.ensure_one_alive(P_.merge(b_dead, s_dead), widths)
        cnt = [d.sum(dim=1).cpu().numpy().astype(np.int64) for d in (b_dead, s_dead, st_dead)]
        return PruneStats(False, *cnt, ibp_lb=ibp_lb, ibp_ub=ibp_ub, cand=cand, s_cand=s_cand, st_dead=st_dead)


def first_pass(s: GroupState, cfg, time_budget: Optional[float]):
    """Stage 3: branch and bound on the original network.  Decides which residue stages run
    (``s.relu_on`` ...), caps the escalation for them and returns the configuration every later
    stage sees."""
    be, mlp, q = s.be, s.mlp, s.q
    with s.clock("bab"):
        s.budget = cfg.soft_timeout if time_budget is None else min(cfg.soft_timeout, time_budget)
        width = max(mlp.hidden or [0])
        s.relu_on = cfg.relu_budget > 0 and width <= cfg.relu_max_width and _relu_supported(q)
        s.beta_on = cfg.beta_budget > 0 and _beta_supported(q) and cfg.beta_min_width <= width <= cfg.beta_max_width
        esc_cap = cfg.relu_escalate_cap if s.relu_on else (cfg.beta_escalate_cap if s.beta_on else 0)
        if esc_cap > 0 and cfg.escalate_budget > esc_cap:
            # the residue of these networks goes to the relu / beta stage: stop the input-split escalation early
            cap = max(esc_cap, cfg.node_budget)
            cfg = replace(cfg, escalate_budget=cap if cap > cfg.node_budget else 0,
                          escalate_probation=tuple(st for st in cfg.escalate_probation if st[0] < cap))
        # relu_first: the escalation pass (one budget, open-frontier gate) runs after stage 3r
        s.esc_after_relu = s.relu_on and cfg.relu_first and cfg.escalate_budget > cfg.node_budget and \
            os.environ.get("FAIRIFY_RELU_FIRST", "1") != "0"
        # inline escalation (native runtime): the first escalation stage runs inside the first pass --
        # partitions that reach node_budget with a small frontier continue instead of restarting from
        # the root in a second solve (FAIRIFY_INLINE_ESCALATE=0: the two-pass schedule)
        inline = s.inline = (be.hip and cfg.inline_escalate and cfg.escalate_budget > cfg.node_budget
                             and cfg.escalate_max_open > 0 and not s.esc_after_relu
                             and os.environ.get("FAIRIFY_INLINE_ESCALATE", "1") != "0"
                             and os.environ.get("FAIRIFY_TORCH_BAB") != "1")
        s.prev_budget = cfg.escalate_budget if inline else cfg.node_budget
        solver = BaBSolver(be, q, BaBConfig(node_budget=cfg.node_budget, batch_nodes=cfg.batch_nodes,
                                            time_budget=s.budget,
                                            escalate_budget=cfg.escalate_budget if inline else 0,
                                            escalate_max_w=cfg.escalate_max_open if inline else 0,
                                            escalate_steps=tuple(cfg.escalate_probation) if inline else ()),
                           timer=s.tm)
        with s.tm("bab"):
            res = solver.solve(s.lo_np, s.hi_np, mlp, init_status=s.status)
        newly_sat = (res.status == SAT) & (s.status != SAT)
        s.stage[newly_sat] = "bab"
        s.stage[(res.status == UNSAT)] = "bab"
        s.cex_x[newly_sat] = res.cex_x[newly_sat]
        s.cex_xp[newly_sat] = res.cex_xp[newly_sat]
        s.status = res.status.copy()
        s.nodes = res.nodes.copy()
        s.stage_nodes[:, 0] = res.nodes
        s.open_left = res.open_left
        s.forced = forced = faults.forced_unknown(s.ids) & (s.stage == "bab")
        if forced.any():
            s.status[forced] = UNKNOWN
            s.stage[forced] = ""
            s.cex_x[forced] = 0
            s.cex_xp[forced] = 0
    return cfg


def falsify(s: GroupState, unk: np.ndarray, seed: int, n_samples: int, k_starts: int, iters: int) -> None:
    """Residual falsifier (heavy sampling + lattice local search) on the partitions ``unk``;
    candidates are confirmed exactly (stage ``falsify``)."""
    ut = torch.from_numpy(unk).to(s.dev)
    fr = residual_falsify(s.be, s.q, s.lo[ut], s.hi[ut], s.pids[ut], s.values, s.pairs, seed, n_samples=n_samples,
                          k_starts=k_starts, iters=iters)
    s.confirm_found(fr, unk, "falsify")


def falsify_stage(s: GroupState, cfg) -> None:
    """Stage 3a: the falsifier on the partitions the BaB left UNKNOWN (the forced ones too)."""
    if cfg.residual_samples <= 0:
        return
    unk = s.unknown(with_forced=True)
    if unk.size:
        with s.clock("bab"), s.tm("falsify"):
            falsify(s, unk, cfg.seed, cfg.residual_samples, cfg.residual_starts, cfg.residual_iters)


def escalate(s: GroupState, cfg) -> None:
    """Stage 3b: escalated sound BaB passes on what is still UNKNOWN (the cheap first pass decides
    the bulk; only residue partitions whose open frontier stayed small -- the ones a deeper search
    can still close -- pay for the deep budgets).  relu_first: after 3r."""
    steps = []
    if cfg.escalate_budget > cfg.node_budget and not s.inline:
        steps.append((cfg.escalate_budget, cfg.escalate_max_open))
    steps += [tuple(st) for st in cfg.escalate_stages]
    with s.charging(0):
        for e_budget, e_open in steps:
            if e_budget <= s.prev_budget:
                continue
            s.prev_budget = e_budget
            want = (s.status == UNKNOWN) & ~s.forced
            if e_open > 0 and s.open_left is not None:
                want &= s.open_left <= e_open
            unk = np.nonzero(want)[0]
            if not unk.size:
                continue
            with s.clock("bab"):
                esolver = BaBSolver(s.be, s.q, BaBConfig(node_budget=e_budget, batch_nodes=cfg.batch_nodes,
                                                         time_budget=s.left()), timer=s.tm)
                with s.tm("bab.escalate"):
                    eres = esolver.solve(s.lo_np[unk], s.hi_np[unk], s.mlp)
                s.absorb(unk, eres, "bab", open_left=True)


def relu_solve(s: GroupState, idx: np.ndarray, cfg, budget: int, time_budget: float) -> int:
    """ReLU-phase BaB on the partitions ``idx``; returns how many it decided (stage ``relu``)."""
    rsolver = ReluBaBSolver(s.be, s.q, ReluConfig(node_budget=budget, batch_nodes=cfg.batch_nodes,
                                                  time_budget=time_budget), timer=s.tm)
    with s.tm("relu"):
        rres = rsolver.solve(s.lo_np[idx], s.hi_np[idx], s.mlp)
    return s.absorb(idx, rres, "relu")


def relu_stage(s: GroupState, cfg) -> None:
    """Stage 3r: ReLU-phase branch-and-bound on the residue (rigorous GPU bounds with neuron-phase
    splits: the exact-zero partitions input splitting cannot close)."""
    unk = s.unknown()
    if unk.size:
        with s.charging(1), s.clock("bab"):
            relu_solve(s, unk, cfg, cfg.relu_budget, s.left())


def _beta_round(s: GroupState, unk: np.ndarray, budget: int, time_budget: float, cfg, anytime: bool = False) -> int:
    """beta-CROWN BaB (engine/beta_bab.py) on the partitions ``unk``; returns how many it decided
    (sound SAT / UNSAT, stage ``beta``).  The fixed pass probes: a partition gives up once it has
    expanded 2 x ``beta_probe_levels`` nodes per pair tree with none of its trees closed (BetaConfig)."""
    branch, iters = cfg.beta_branch, cfg.beta_iters
    if branch == "auto":
        _, pairs = pa_table(s.q, s.lo_np[unk[:1]], s.hi_np[unk[:1]])
        branch, iters = ("pgap", cfg.beta_iters) if pairs.shape[0] <= 2 else ("kernel", 64)
    bs = BetaBaBSolver(s.be, s.q, BetaConfig(
        node_budget=budget, batch_nodes=min(cfg.batch_nodes, 32768), time_budget=time_budget,
        probe_levels=0 if anytime else cfg.beta_probe_levels, branch=branch, iters=iters,
        root_iters=max(200, 3 * iters), lookahead=cfg.beta_lookahead, decay=cfg.beta_decay,
        feas_iters=max(cfg.beta_feas_iters, 64) if anytime else cfg.beta_feas_iters, batched=cfg.beta_batched),
        timer=s.tm)
    t0 = time.time()
    br = bs.solve(s.lo_np[unk], s.hi_np[unk], s.mlp)
    ndec = s.absorb(unk, br, "beta")
    if os.environ.get("FAIRIFY_BETA_LOG"):
        print(f"[beta] {unk.size} partitions, budget {budget}: decided {ndec} in "
              f"{time.time() - t0:.2f} s, {bs.stats}", file=sys.stderr, flush=True)
    return ndec


def beta_stage(s: GroupState, cfg) -> None:
    """Stage 3b': beta-CROWN phase-split BaB on the residue (the wide nets' UNSAT partitions need
    phase splits as constraints on the region: Lagrangian split multipliers)."""
    unk = s.unknown()
    if unk.size:
        with s.clock("bab"), s.charging(2), s.tm("beta"):
            _beta_round(s, unk, cfg.beta_budget, s.left(), cfg)


def _milp_round(s: GroupState, unk: np.ndarray, limit: float, cfg, deadline: Optional[float] = None) -> None:
    """HiGHS MILP on the partitions ``unk`` (per-partition time limit ``limit``, nothing starts
    after ``deadline``); exactly confirmed SAT verdicts are written into the state.  An UNSAT
    answer (floating-point dual bound) is only recorded as stage ``milp`` on a partition that
    stays UNKNOWN, unless ``cfg.trust_milp`` (then it is an UNSAT verdict of stage ``milp``)."""
    mlp = s.mlp
    futs = milp.submit(s.be, mlp, s.q, s.lo_np[unk], s.hi_np[unk], s.values_np, s.pairs_np, limit,
                       workers=cfg.smt_workers, deadline=deadline)
    cand_k, cand_x, cand_xp = [], [], []
    t_note = time.time()
    for i, (k, f) in enumerate(zip(unk, futs)):
        verdict, pair = f.result()
        if _VERBOSE_ANYTIME and time.time() - t_note > 30.0:
            t_note = time.time()
            print(f"[milp] {mlp.name}: {i + 1}/{len(unk)} partitions, limit {limit:.1f}s", flush=True)
        if verdict == "unsat":
            s.stage[k] = "milp"
            if cfg.trust_milp:
                s.status[k] = UNSAT
        elif verdict == "sat" and pair is not None:
            cand_k.append(k)
            cand_x.append(pair[0])
            cand_xp.append(pair[1])
    if cand_k:
        s.confirm(np.asarray(cand_k), np.asarray(cand_x, dtype=np.int64), np.asarray(cand_xp, dtype=np.int64), "milp")


def _lp_submit(s: GroupState, unk: np.ndarray, budget: int, limit: float, cfg, deadline: Optional[float] = None):
    """Start the verified-LP searches (smt/lpbab.py) of ``unk`` in the worker processes: HiGHS
    solves, a rigorous weak-duality bound from its multipliers closes nodes, lattice points and LP
    optima are checked exactly.  Returns [(k, future)]."""
    futs = lpbab.submit(s.be, s.mlp, s.q, s.lo_np[unk], s.hi_np[unk], s.values_np, s.pairs_np, budget, limit,
                        workers=cfg.smt_workers, deadline=deadline)
    return list(zip(unk, futs))


def _lp_collect(s: GroupState, pending, budget: int) -> None:
    """Wait for the LP searches of :func:`_lp_submit` (UNSAT and SAT are both sound, stage ``lp``);
    a partition another stage decided meanwhile keeps that verdict (both are sound)."""
    status = s.status
    t_note = time.time()
    # searches of partitions another stage decided meanwhile: not started ones are dropped, so the
    # shared worker pool is not kept busy for nothing (running ones finish and are ignored)
    for k, f in pending:
        if status[k] != UNKNOWN:
            f.cancel()
    for i, (k, f) in enumerate(pending):
        if f.cancelled():
            continue
        verdict, pair, _ = f.result()
        if _VERBOSE_ANYTIME and time.time() - t_note > 30.0:
            t_note = time.time()
            print(f"[lp] {s.mlp.name}: {i + 1}/{len(pending)} partitions, budget {budget}", flush=True)
        if status[k] != UNKNOWN:
            continue
        if verdict == "unsat":
            status[k], s.stage[k] = UNSAT, "lp"
        elif verdict == "sat" and pair is not None:
            status[k], s.stage[k] = SAT, "lp"
            s.cex_x[k], s.cex_xp[k] = pair[0], pair[1]


def _lp_available() -> bool:
    """The verified-LP stage drives HiGHS through SciPy's private ``_highspy._core`` bindings (SciPy
    >= 1.15); without them the stage is off and the MILP stage runs instead of an aborting worker."""
    try:
        from scipy.optimize._highspy import _core  # noqa: F401
    except ImportError:
        return False
    return True


def _use_lp(cfg) -> bool:
    return cfg.lp_budget > 0 and not cfg.trust_milp and _lp_available()


def _host_smt(cfg):
    """Host SMT pool for the residue (cached per configuration; inactive without a back-end)."""
    key = (cfg.smt_backend, cfg.smt_workers, cfg.smt_timeout or cfg.soft_timeout, cfg.smt_fork_params)
    if key not in _HOST_SMT:
        _HOST_SMT[key] = HostSMT(cfg.smt_backend, cfg.smt_workers, key[2], cfg.smt_fork_params)
    return _HOST_SMT[key]


def host_solver_stage(s: GroupState, cfg, pr: PruneStats) -> None:
    """Stage 3c: exact host solver on the residue (the reference's Z3 check,
    src/AC/Verify-AC.py:145-158): Z3 when installed, else the verified LP or the HiGHS MILP fed the
    GPU's rigorous layer bounds (smt/milp.py); no-op with "none".  Its time counts as BaB time."""
    if cfg.smt_backend == "none":
        return
    backend = smt_solver.resolve(cfg.smt_backend)
    unk = s.unknown()
    limit = cfg.smt_timeout or cfg.soft_timeout
    if backend == "milp" and unk.size and cfg.anytime_seconds <= 0:   # anytime: rounds inside 3d
        with s.clock("bab", sync=False):
            if _use_lp(cfg):
                with s.tm("lp"):
                    _lp_collect(s, _lp_submit(s, unk, cfg.lp_budget, limit, cfg), cfg.lp_budget)
            else:
                with s.tm("milp"):
                    _milp_round(s, unk, limit, cfg)
    elif backend != "milp" and unk.size and _host_smt(cfg).active:
        hs = _host_smt(cfg)
        with s.clock("bab", sync=False), s.tm("smt"):
            ut = torch.from_numpy(unk).to(s.dev)
            st_mask = ((pr.code[ut][:, :s.Nh] & H.PM_ST) != 0) if pr.fused else pr.st_dead[ut][:, :s.Nh]
            futs = hs.submit(s.mlp, s.q, s.lo_np[unk], s.hi_np[unk], st_mask)
            for k, f in zip(unk, futs):
                verdict, pair = f.result()
                if verdict == "unsat":
                    s.status[k], s.stage[k] = UNSAT, "smt"
                elif verdict == "sat" and pair is not None:
                    s.confirm(np.array([k]), np.array([pair[0]], dtype=np.int64),
                              np.array([pair[1]], dtype=np.int64), "smt")


class _Anytime:
    """Round state of the anytime loop: the growing budgets and which stages still yield."""

    def __init__(self, s: GroupState, cfg):
        self.deadline = time.time() + cfg.anytime_seconds
        self.rounds = 0
        self.e_budget = max(s.prev_budget, cfg.node_budget)
        self.n_samp = max(cfg.residual_samples, 1)
        self.use_milp = cfg.smt_backend != "none" and smt_solver.resolve(cfg.smt_backend) == "milp"
        self.milp_limit = cfg.anytime_milp_seconds
        # x growth per round; the first round at budget / 4: trained AC-7's UNSAT partitions need
        # 100-5 000 LP nodes (profiles/r4/lp_tree_sizes_ac7_trained.jsonl), and every round restarts
        # its searches from the root
        lp_div = cfg.anytime_lp_div or (1 if len(s.pairs_np) > 2 else 4)
        self.lp_budget = max(1, cfg.lp_budget // lp_div)
        self.relu_any = _relu_supported(s.q) and cfg.relu_budget > 0   # any layer width
        self.r_budget = max(cfg.relu_budget, 1) if s.relu_on else 64   # x growth before the first round
        self.bab_live, self.relu_live = True, True                     # stages still yielding
        self.beta_live = cfg.anytime_beta > 0 and _beta_supported(s.q)  # any width in the anytime rounds
        self.b_budget = (max(cfg.beta_budget, cfg.anytime_beta) if s.beta_on
                         else max(cfg.anytime_beta // cfg.anytime_growth, 1))

    def left(self) -> float:
        return self.deadline - time.time()


def _anytime_groups(s: GroupState, cfg, a: _Anytime, budget: int, solve) -> bool:
    """``solve(group, seconds left)`` over the residue in groups that fit the node pool, until the
    deadline or a yield below ``anytime_min_yield``; True if the stage should not run again."""
    unk = s.unknown()
    G = max(1, cfg.anytime_pool // max(1, budget))
    n_try = n_dec = 0
    for g0 in range(0, unk.size, G):
        left = a.left()
        if left <= 0:
            break
        grp = unk[g0:g0 + G]
        n_try += grp.size
        n_dec += solve(grp, left)
        if n_try >= 256 and n_dec < cfg.anytime_min_yield * n_try:
            break                                   # not converging: stop the round early
    return bool(n_try) and n_dec < cfg.anytime_min_yield * n_try


def _anytime_bab(s: GroupState, cfg, a: _Anytime, grp: np.ndarray, left: float) -> int:
    asolver = BaBSolver(s.be, s.q, BaBConfig(node_budget=a.e_budget, batch_nodes=cfg.batch_nodes, time_budget=left,
                                             max_pool=cfg.anytime_pool), timer=s.tm)
    return s.absorb(grp, asolver.solve(s.lo_np[grp], s.hi_np[grp], s.mlp), "bab")


def anytime_stage(s: GroupState, cfg) -> None:
    """Stage 3d: anytime escalation on the residue (sound; before the heuristic): rounds of growing
    budgets until the residue is empty, the deadline passes or no stage can still decide."""
    if cfg.anytime_seconds <= 0:
        return
    with s.charging(3), s.clock("bab"), s.tm("anytime"):
        a = _Anytime(s, cfg)
        while True:
            unk = s.unknown()
            if not unk.size or time.time() >= a.deadline:
                break
            a.rounds += 1
            # (b) beta-CROWN phase-split BaB with a growing budget first: it closes the wide nets'
            # UNSAT residue on the GPU in a few dozen nodes per partition, before the host LP
            # is handed what is left
            if a.beta_live:
                a.b_budget *= cfg.anytime_growth
                left = a.left()
                if left > 0:
                    # at most half of what is left: where it does not converge (random-init
                    # residue) the other stages keep their time
                    with s.tm("beta"):
                        ndec = _beta_round(s, unk, a.b_budget, 0.5 * left, cfg, anytime=True)
                    if ndec < cfg.anytime_min_yield * unk.size:
                        a.beta_live = False
                unk = s.unknown()
                if not unk.size:
                    break
            # (e, started first) verified-LP branch-and-bound on the host workers with a growing
            # node budget, CONCURRENT with this round's GPU stages (collected at the round's end):
            # on a residue the GPU stages do not converge on (trained AC-7) the round costs
            # max(GPU, LP) instead of their sum
            lp_pending = None
            if a.use_milp and _use_lp(cfg):
                left = a.left()
                with s.tm("lp.submit"):
                    lp_pending = _lp_submit(s, unk, a.lp_budget, min(a.milp_limit * 4, left), cfg, deadline=a.deadline)
            # (a) fresh samples + boundary walk + local search, new seed every round
            a.n_samp = min(a.n_samp * cfg.anytime_growth, cfg.anytime_max_samples)
            falsify(s, unk, cfg.seed + 7919 * a.rounds, a.n_samp, 2 * cfg.residual_starts, 2 * cfg.residual_iters)
            # (c) deeper sound BaB, in groups that fit the node pool
            a.e_budget *= cfg.anytime_growth
            if a.e_budget > cfg.anytime_max_budget:
                a.bab_live = False
            if not (a.bab_live or (a.relu_any and a.relu_live) or a.use_milp or a.beta_live):
                break                                       # nothing left that can still decide
            if _VERBOSE_ANYTIME:
                print(f"[anytime] {s.mlp.name} round {a.rounds}: {s.unknown().size} unknown after falsify "
                      f"({a.n_samp} samples), BaB budget {a.e_budget}, {a.left():.1f}s left", flush=True)
            if a.bab_live and _anytime_groups(s, cfg, a, a.e_budget, lambda g, t: _anytime_bab(s, cfg, a, g, t)):
                a.bab_live = False
            # (d) ReLU-phase BaB with a growing budget, any layer width (the anytime budget pays
            # for the wide nets too; it re-proves partitions the MILP only claims)
            if a.relu_any and a.relu_live:
                a.r_budget *= cfg.anytime_growth
                if _anytime_groups(s, cfg, a, a.r_budget, lambda g, t: relu_solve(s, g, cfg, a.r_budget, t)):
                    a.relu_live = False
            # (e) collect the verified-LP searches started with the round (sound UNSAT and SAT),
            # or -- trust_milp / lp_budget 0 -- the HiGHS MILP with a growing time limit
            if lp_pending is not None:
                with s.tm("lp"):
                    _lp_collect(s, lp_pending, a.lp_budget)
                a.lp_budget *= cfg.anytime_growth
                a.milp_limit *= cfg.anytime_growth
            elif a.use_milp:
                # partitions the MILP already claimed UNSAT (unverified) are not re-solved
                unk = np.nonzero((s.status == UNKNOWN) & ~s.forced & (s.stage != "milp"))[0]
                left = a.left()
                if unk.size and left > 0:
                    with s.tm("milp"):
                        _milp_round(s, unk, min(a.milp_limit, left), cfg, deadline=a.deadline)
                a.milp_limit *= cfg.anytime_growth


@dataclass
class HeuristicResult:
    """Stage 4's outputs: the attempt / success flags, the dead counts, the merged heuristic mask
    of every retried partition (``masked``: partition -> [N] bool) and, on the fused path, the
    device masks ``hm_t`` of the retried partitions ``unk``."""
    h_attempt: np.ndarray
    h_success: np.ndarray
    h_cnt: np.ndarray
    t_cnt: np.ndarray
    masked: Dict[int, np.ndarray]
    unk: np.ndarray
    hm_t: Optional[torch.Tensor] = None


class _LazyMasked:
    """Per-partition heuristically pruned networks, materialised only when a SAT candidate of
    that partition needs exact confirmation."""

    def __init__(self, mlp: MLP, masks: List[np.ndarray], widths):
        self.mlp, self.masks, self.sls = mlp, masks, P_.layer_slices(widths)
        self.cache: Dict[int, MLP] = {}

    def __getitem__(self, k: int) -> MLP:
        if k not in self.cache:
            self.cache[k] = self.mlp.masked([self.masks[k][sl] for sl in self.sls])
        return self.cache[k]

    def __len__(self) -> int:
        return len(self.masks)


def heuristic_stage(s: GroupState, cfg, pr: PruneStats) -> HeuristicResult:
    """Stage 4: heuristic retry for UNKNOWN partitions, the forced ones too (unsound, flagged)."""
    be, mlp, q, Nh, widths = s.be, s.mlp, s.q, s.Nh, s.mlp.widths
    unk = s.unknown(with_forced=True)
    h_attempt, h_success, h_cnt = (np.zeros(s.Pn, dtype=np.int64) for _ in range(3))
    h = HeuristicResult(h_attempt, h_success, h_cnt, pr.st_cnt.copy(), {}, unk)
    if not (cfg.heuristic and unk.size and pr.ibp_ub is not None):
        return h
    with s.clock("heur"), s.charging(4):
        h.h_attempt[unk] = 1
        with s.tm("heuristic.masks"):
            ut = torch.from_numpy(unk).to(s.dev)
            if pr.fused:
                _, h.hm_t, hc_t = H.heuristic(be, ut, pr.ibp_lb, pr.ibp_ub, pr.code, cfg.heuristic_p)
                md_np = h.hm_t.cpu().numpy().astype(bool)
                hc_np = hc_t.cpu().numpy().astype(np.int64)
                h.h_cnt[unk], h.t_cnt[unk] = hc_np[:, 0], hc_np[:, 1]
                dead_t = h.hm_t[:, :Nh].contiguous()
            else:
                hd_t, md_t = P_.heuristic_prune_batch(pr.ibp_lb[ut], pr.ibp_ub[ut], pr.cand[ut], pr.s_cand[ut],
                                                      pr.st_dead[ut], widths, cfg.heuristic_p)
                md_np = md_t.cpu().numpy()
                h.h_cnt[unk] = hd_t.sum(dim=1).cpu().numpy()
                h.t_cnt[unk] = md_np.sum(axis=1)
                dead_t = torch.from_numpy(md_np[:, :Nh]).to(s.dev)
            for k, p in enumerate(unk):
                h.masked[p] = md_np[k]
        # partitions whose heuristic mask equals the sound mask would re-run the same query
        exact_models = _LazyMasked(mlp, [h.masked[p] for p in unk], widths)
        hsolver = BaBSolver(be, q, BaBConfig(node_budget=cfg.heuristic_node_budget, batch_nodes=cfg.batch_nodes,
                                             time_budget=s.budget), dead=dead_t, timer=s.tm)
        with s.tm("heuristic.bab"):
            hres = hsolver.solve(s.lo_np[unk], s.hi_np[unk], mlp, exact_models=exact_models)
        s.absorb(unk, hres, "heuristic")
        h.h_success[unk[s.status[unk] != UNKNOWN]] = 1      # all of unk was UNKNOWN before the merge
        hs = unk[hres.status == SAT]
        if hs.size:
            # a heuristic SAT pair was confirmed on the MASKED net; one that also flips the original
            # network (the reference's V-accurate replay, src/AC/Verify-AC.py:225-258) is a sound
            # counterexample: stage "heuristic-confirmed"
            X, XP = s.cex_x[hs], s.cex_xp[hs]
            ok = exact.check_pair_constraints(X, XP, s.lo_np[hs], s.hi_np[hs], q.pa_idx, q.ra_idx, q.tau)
            s.stage[hs[exact.is_violation(mlp, X, XP) & ok]] = "heuristic-confirmed"
    return h


def final_mask_bits(s: GroupState, pr: PruneStats, h: HeuristicResult) -> np.ndarray:
    """K6: [Pn, ceil(N/8)] uint8 (numpy.packbits order) final dead masks: the sound-prune mask
    (ST = B ∪ S with one neuron kept alive per layer), replaced by the merged heuristic mask for
    the partitions of the heuristic retry -- the mask whose popcount is the CSV's T-compression
    numerator.  On the GPU the mask algebra codes are packed by ``fa_pack_masks_kernel``."""
    N = s.mlp.n_neurons
    if pr.fused:
        fm = ((pr.code & H.PM_ST) != 0).to(torch.uint8)
        if h.hm_t is not None and len(h.unk):
            fm[torch.from_numpy(np.asarray(h.unk)).to(fm.device)] = (h.hm_t != 0).to(torch.uint8)
        bits, _ = H.pack_masks(fm)
        return bits.cpu().numpy()
    m = pr.st_dead.cpu().numpy().astype(bool)
    for p, mk in h.masked.items():
        m[p] = np.asarray(mk, dtype=bool)[:N]
    return np.packbits(m, axis=1)


def replay_stage(s: GroupState, cfg, masked: Dict[int, np.ndarray]) -> Dict[str, np.ndarray]:
    """Stage 5: replay / fidelity (batched on the device): the c_check / v_accurate flags of the SAT
    pairs and the Pruned-acc / Pruned-F1 counts of the masked (``pruned_metrics``: all) partitions."""
    be, mlp, Pn, Nh, dev = s.be, s.mlp, s.Pn, s.Nh, s.dev
    cex_x, cex_xp = s.cex_x, s.cex_xp
    with s.clock("replay", sync=False), s.tm("replay"):
        sat_idx = np.nonzero(s.status == SAT)[0]
        c_check = np.zeros(Pn, dtype=np.int64)
        v_acc = np.zeros(Pn, dtype=np.int64)
        if sat_idx.size:
            xo = mlp.predict(cex_x[sat_idx])
            xpo = mlp.predict(cex_xp[sat_idx])
            v_acc[sat_idx] = (xo != xpo).astype(np.int64)
            dmask = np.zeros((sat_idx.size, Nh), dtype=bool)
            for k, p in enumerate(sat_idx):
                if p in masked:
                    dmask[k] = masked[p][:Nh]
            xt = torch.from_numpy(np.concatenate([cex_x[sat_idx], cex_xp[sat_idx]])).to(dev, torch.float32)
            dt_ = torch.from_numpy(np.concatenate([dmask, dmask])).to(dev)
            zp = be.forward(xt, dt_).cpu().numpy()
            c1 = (zp[:sat_idx.size] > 0).astype(np.int64)
            c2 = (zp[sat_idx.size:] > 0).astype(np.int64)
            c_check[sat_idx] = ((c1 == xo) & (c2 == xpo)).astype(np.int64)
        agree = np.full(Pn, cfg.sim_size, dtype=np.int64)     # Pruned-acc numerator
        tp = np.zeros(Pn, dtype=np.int64)                      # Pruned-F1 counts (pruned_metrics)
        fp = np.zeros(Pn, dtype=np.int64)
        if masked or cfg.pruned_metrics:
            # pruned_metrics: every partition (unmasked ones with their sound-pruned net, which
            # equals the original on the box: mask of zeros) for the experiment drivers' F1
            hp = np.arange(Pn) if cfg.pruned_metrics else np.array(sorted(masked))
            dm_np = np.zeros((hp.size, Nh), dtype=np.uint8)
            for k, p in enumerate(hp):
                if p in masked:
                    dm_np[k] = masked[p][:Nh]
            dm = torch.from_numpy(dm_np).to(dev)
            ag = None
            if be.hip and os.environ.get("FAIRIFY_FUSED_PRUNE", "1") != "0":
                ag = H.agree(be, torch.from_numpy(hp).to(dev), s.lo, s.hi, s.pids, dm, cfg.sim_size, cfg.seed)
            if ag is not None:
                ag_np = ag.cpu().numpy().astype(np.int64)
                agree[hp], tp[hp], fp[hp] = ag_np[:, 0], ag_np[:, 1], ag_np[:, 2]
            else:
                X = sample_points(s.lo[hp], s.hi[hp], s.pids[hp], cfg.sim_size, cfg.seed)
                z0 = be.forward(X)
                z1 = be.forward(X, dm.bool()[:, None, :].expand(-1, X.shape[1], -1))
                agree[hp] = ((z0 > 0) == (z1 > 0)).sum(dim=1).cpu().numpy()
                tp[hp] = ((z0 > 0) & (z1 > 0)).sum(dim=1).cpu().numpy()
                fp[hp] = ((z0 <= 0) & (z1 > 0)).sum(dim=1).cpu().numpy()
    return dict(agree=agree, tp=tp, fp=fp, c_check=c_check, v_accurate=v_acc)


def records(s: GroupState, pr: PruneStats, h: HeuristicResult, r: Dict[str, np.ndarray]):
    """(core columns, segment): dead-neuron counts, work, per-chunk stage times (the per-partition
    time columns are apportioned from these by derive_columns, here and after a gather)."""
    verdict = np.where(s.status == SAT, "sat", np.where(s.status == UNSAT, "unsat", "unknown"))
    stage_f = np.where(s.stage == "", np.where(verdict != "unknown", "bab", ""), s.stage)
    core = dict(
        grid_id=np.asarray(s.ids, dtype=np.int64), verdict=verdict, stage=stage_f.astype(object),
        h_attempt=h.h_attempt, h_success=h.h_success,
        b_cnt=pr.b_cnt, s_cnt=pr.s_cnt, st_cnt=pr.st_cnt, h_cnt=h.h_cnt, t_cnt=h.t_cnt, agree=r["agree"], tp=r["tp"],
        fp=r["fp"], nodes=s.nodes.astype(np.int64), c_check=r["c_check"], v_accurate=r["v_accurate"], cex_x=s.cex_x,
        cex_xp=s.cex_xp, stage_nodes=s.stage_nodes)
    t = s.times
    return core, (s.Pn, t["sim"] + t["prune"] + t["bab"], t["bab"], t["heur"], t["replay"])


def _verify_group(s: GroupState, cfg, time_budget: Optional[float]):
    """All stages on one group of partitions: (core columns, segment)."""
    sim = sim_stage(s, cfg)
    pr = prune_stage(s, cfg, sim)
    cfg = first_pass(s, cfg, time_budget)       # caps the escalation of relu / beta networks
    falsify_stage(s, cfg)
    if not s.esc_after_relu:
        escalate(s, cfg)
    if s.relu_on:
        relu_stage(s, cfg)
    if s.beta_on:
        beta_stage(s, cfg)
    if s.esc_after_relu:                        # relu_first: the escalation on what the relu stage left
        escalate(s, cfg)
    host_solver_stage(s, cfg, pr)
    anytime_stage(s, cfg)
    h = heuristic_stage(s, cfg, pr)
    mask_bits = None
    if cfg.keep_masks:
        with s.tm("masks"):
            mask_bits = final_mask_bits(s, pr, h)
    core, seg = records(s, pr, h, replay_stage(s, cfg, h.masked))
    if mask_bits is not None:
        core["mask_bits"] = mask_bits
    return core, seg
