"""Per-model verification pipeline over a stream of partition chunks.

Re-design of the per-partition loop of the reference drivers (``src/GC/Verify-GC.py:106-315``):
sound prune -> SMT query -> heuristic prune + re-query on ``unknown`` -> counterexample replay
-> one CSV row per partition -> hard timeout.  Here a *chunk* of partitions (thousands) goes
through each stage at once on the device:

  decode ids -> simulate/profile/falsify (K3+K8) -> IBP bounds (K2, B-compression) ->
  symbolic bounds (K4, S-compression) -> branch-and-bound (K9) -> [heuristic masks (K5) +
  BaB on the masked nets for UNKNOWN partitions] -> replay (K7) -> records.

Per-partition timings are the chunk's stage times apportioned by each partition's share of
the work (BaB node expansions), so the 24 CSV columns keep their meaning.
"""
from __future__ import annotations

import contextlib
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..models.mlp import MLP
from ..ops.backend import Backend
from ..ops.reference import sample_points
from ..parallel.balance import host_threads
from ..partition import Grid
from ..spec import ResolvedQuery
from ..utils.timer import StageTimer
from .bab import pa_groups
from .chunk_group import STAGE_NODE_COLS, GroupState, _lp_available, _verify_group  # noqa: F401  (re-exported)


@dataclass
class VerifyConfig:
    sim_size: int = 1000                 # reference sim_size (src/AC/Verify-AC.py:115)
    seed: int = 0
    chunk: int = 4096                    # partitions per device batch
    soft_timeout: float = 100.0          # seconds (caps one chunk's BaB wall time)
    hard_timeout: float = 30 * 60.0      # seconds per model (checked after each chunk)
    node_budget: int = 4096              # BaB expansions per partition
    escalate_budget: int = 0             # second sound BaB pass on the residue with this node
                                         # budget (0 = off); runs after the residual falsifier
    escalate_max_open: int = 0           # only escalate partitions that left at most this many
                                         # open nodes in the first pass (0 = all; native BaB only)
    escalate_stages: Tuple[Tuple[int, int], ...] = ()
    # inline escalation steps between node_budget and escalate_budget: (budget, max frontier) --
    # a partition continues past each step's budget only if its open frontier at that level is at
    # most the limit (the first step uses escalate_max_open)
    escalate_probation: Tuple[Tuple[int, int], ...] = ()
    inline_escalate: bool = True         # native BaB: run the escalate_budget stage inside the first
                                         # pass (escalate_max_open then bounds the frontier size)
                                         # further (budget, max_open) passes after the escalated one,
                                         # each on the residue the previous pass left
    batch_nodes: int = 65536             # BaB nodes per sub-batch launch
    heuristic: bool = True               # reference behaviour: heuristic retry on unknown
    heuristic_p: float = 5.0             # HEURISTIC_PRUNE_THRESHOLD
    heuristic_node_budget: int = 4096
    bisect_pairs: int = 16
    bisect_steps: int = 0                # boundary walk in the sim stage; 0 = off (the residual
                                         # falsifier finds the same witnesses: A/B 87.32 vs 87.32 %)
    sound_prune_stats: bool = True       # compute B/S compression (reference parity columns)
    residual_samples: int = 2048         # residual falsifier on BaB-UNKNOWN partitions (0 = off)
    residual_starts: int = 16            # local-search starts per partition
    residual_iters: int = 12             # coordinate-ascent rounds
    smt_backend: str = "auto"            # exact host solver on the BaB residue: auto (Z3 if installed,
                                         # else the HiGHS MILP back-end) | z3py | z3bin | milp | none
    # host solver processes (LP / MILP / SMT): the rank's CPUs, at most 15 (a one-GPU share of 16
    # CPUs less the GPU driver thread; trained AC-7 at 120 s: 12 workers 74.5 / 85.2 % sound,
    # 15 workers 78.3 / 87.8 %); FAIRIFY_SMT_WORKERS overrides
    smt_workers: int = field(default_factory=lambda: int(os.environ.get("FAIRIFY_SMT_WORKERS", "0"))
                             or host_threads(15, 1))
                                         # host solver threads: this rank's CPUs (its node slice when
                                         # several ranks share a node, parallel/balance.py), at most 12
    smt_timeout: Optional[float] = None  # per query; defaults to soft_timeout
    smt_fork_params: bool = False        # Z3 seed/restart/phase options of the fork's drivers
    # anytime mode: after the fixed passes, keep growing the node budget (x anytime_growth per
    # round) and the residual falsifier's sample count on the sound-UNKNOWN residue until it is
    # empty or this chunk's share of the model's wall budget is spent (the reference spends up to
    # its hard timeout per model, src/AC/Verify-AC.py:318-320).  0 = off.
    anytime_seconds: float = 0.0
    pruned_metrics: bool = False         # Pruned-F1 counts for every partition (the experiment
                                         # drivers' per-partition metrics CSV)
    anytime_growth: int = 4
    anytime_max_budget: int = 1 << 22
    anytime_pool: int = 1 << 24          # live BaB nodes per group: group size = pool / budget
    anytime_max_samples: int = 16384
    anytime_milp_seconds: float = 1.0    # first MILP round's per-partition limit (x growth per round)
    # a GPU stage (input-split / ReLU-phase BaB) whose anytime round decides less than this fraction
    # of the partitions it attempted is not run in later rounds: its next budget (x growth) would
    # spend the remaining time where it does not converge (trained AC-7: 1.6 G input-split nodes in
    # 110 s for 424 proofs) -- the other stages get it
    anytime_min_yield: float = 0.01
    # the first anytime round's verified-LP node budget is lp_budget / this (x growth per round);
    # 0 = by the PA table: a binary PA (2 ordered pairs) starts at 1/4 -- many cheap attempts first
    # (trained AC-7/sex at 120 s: 78.8 % vs 72.8 % at the full budget) --, a multi-valued PA at the
    # full budget, where the per-value sign tests need it (AC-7/race: 99.8 % vs 87.8 %)
    anytime_lp_div: int = int(os.environ.get("FAIRIFY_ANYTIME_LP_DIV", "0"))
    relu_budget: int = 2048              # ReLU-phase BaB (stage "relu", engine/relu_bab.py) on the
                                         # input-split residue: nodes per partition (0 = off)
    relu_max_width: int = 16             # ... only for networks whose hidden layers are at most this
                                         # wide (the narrow zero-bias shapes it closes; on the wide AC
                                         # shapes it spends its budget without deciding: tools/diag_relu.py)
    relu_escalate_cap: int = 0           # networks the relu stage runs on: cap the input-split
                                         # escalation budget at this (their residue goes to the cheaper
                                         # relu stage instead of deep input splitting; 0 = no cap)
    relu_first: bool = True              # relu-covered networks: the (capped) input-split escalation
                                         # runs AFTER the relu stage, on what it left, instead of inline
                                         # in the first pass -- most of their escalated partitions are
                                         # zero-logit boxes the relu stage closes in a few nodes
                                         # (profiles/r3/shard/diag_models_bench_config.jsonl: 38 % of a
                                         # bench step's nodes were AC-8 / AC-12 escalation spent on
                                         # partitions the relu stage then decided)
    beta_budget: int = int(os.environ.get("FAIRIFY_BETA_BUDGET", "128"))
                                         # beta-CROWN phase-split BaB (stage "beta", engine/beta_bab.py)
                                         # on the residue: nodes per partition (0 = off); the trained
                                         # AC-7 residue closes in 10-60 nodes, the random-init bench
                                         # residue mostly does not (512 nodes: +3.4 s per step for 147
                                         # verdicts, gpurun_out/s5_c); 128 with probe 8 over 64 with
                                         # probe 4: targeted/AC AC-7 97.29 -> 98.30 % for +7 % time
                                         # (profiles/r5/s5_u/); the anytime rounds grow it x
                                         # anytime_growth per round
    anytime_beta: int = 64               # anytime rounds: beta BaB nodes per partition of the first round
                                         # (x anytime_growth per round; 0 = off), independent of the
                                         # fixed-pass beta_budget
    # fixed pass: a partition gives up once it has expanded 2 x this many nodes per pair tree with none
    # of its trees closed (0 = never)
    beta_probe_levels: int = int(os.environ.get("FAIRIFY_BETA_PROBE", "8"))
    beta_min_width: int = 17             # ... on networks whose widest hidden layer is at least this
                                         # (the narrower ones go to the relu stage, whose exact-zero
                                         # concretisation their zero logits need)
    beta_max_width: int = 256            # ... and at most this (fixed pass only).  BM-4's 150-wide layer ran in
                                         # round 5 with its weights staged in LDS (2 waves per CU) and decided
                                         # 1.5 % of its residue; with the weights read from L2 (7 waves per
                                         # CU) and primal-gap branching relaxed/BM BM-4 goes 11 118 -> 8 532
                                         # UNKNOWN (98.89 -> 99.15 %) for 49.8 -> 68.3 s (profiles/r6/); a
                                         # static rule, so verdicts stay independent of the sharding
    beta_branch: str = os.environ.get("FAIRIFY_BETA_BRANCH", "auto")
                                         # BetaConfig.branch: "pgap" = the verified LP's primal-gap rule
                                         # at the averaged primal iterate (relaxed/BM BM-8 residue: 33 vs
                                         # 5 of 200 decided at 1 024 nodes, profiles/r6/), "kernel" =
                                         # |lambda| x gap at the vertex x* (round 5); "auto": pgap with
                                         # beta_iters steps for a binary PA (2 ordered pairs), kernel with
                                         # 64 for a multi-valued one -- measured per query at the fixed
                                         # pass's budget: relaxed/BM BM-8 17 866 vs 22 785 UNKNOWN (pgap /
                                         # kernel), stress/AC AC-7 4 466 vs 4 668, but relaxed/AC AC-7
                                         # (race, 20 pairs) 1 840 vs 1 755 at 27.3 vs 18.9 s (profiles/r6/)
    beta_iters: int = int(os.environ.get("FAIRIFY_BETA_ITERS", "128"))
                                         # optimisation steps per child node (root: x 3); 128 over 64:
                                         # 48 vs 33 of 200 at 1 024 nodes (a converged dual gives the
                                         # primal average its meaning)
    beta_lookahead: int = 8              # filtered look-ahead candidates per score list
    beta_decay: float = float(os.environ.get("FAIRIFY_BETA_DECAY", "0.98"))
                                         # step-size decay per optimisation step (BetaConfig.decay)
    beta_feas_iters: int = int(os.environ.get("FAIRIFY_BETA_FEAS", "0"))
                                         # infeasibility pass steps on open children (BetaConfig.feas_iters)
                                         # in the fixed pass: off -- at its 128-node budget with the probe
                                         # it decided nothing more (relaxed/BM BM-8 17 866 vs 18 234 UNKNOWN,
                                         # profiles/r6/); the anytime rounds (growing budgets) run 64 steps
    beta_batched: bool = os.environ.get("FAIRIFY_BETA_BATCHED", "0") == "1"
                                         # two-phase beta level: the optimisation on MFMA, 16 nodes per wave
                                         # (BetaConfig.batched, csrc/beta_opt16.hip); opt-in
    beta_escalate_cap: int = int(os.environ.get("FAIRIFY_BETA_ESC_CAP", "0"))
                                         # networks the beta fixed pass runs on: cap the input-split
                                         # escalation budget at this (their residue goes to beta instead
                                         # of deep input splitting; 0 = no cap)
    lp_budget: int = 4096                # verified-LP branch-and-bound (stage "lp", smt/lpbab.py) in
                                         # place of the untrusted MILP: LP nodes per partition (x growth
                                         # per anytime round); 0 = the round-2 MILP stage
    trust_milp: bool = False             # HiGHS MILP UNSAT rests on a floating-point dual bound: by
                                         # default it is recorded (stage "milp") but the partition
                                         # stays UNKNOWN for the rigorous stages; True = round-2
                                         # behaviour (UNSAT, stage "milp", excluded from sound counts)
    keep_masks: bool = False             # K6: keep every partition's final dead-neuron mask (sound
                                         # prune, or the heuristic mask of a retried partition) as a
                                         # packed bitset (core["mask_bits"], ceil(N/8) B) for the
                                         # rank-0 gather, dedup and pruned-subnet export

    def __post_init__(self):
        # the rank-0 wire records (parallel/wire.py) carry the agree / tp / fp counts of the
        # simulation points as uint16: reject a sample count they cannot hold here, before any
        # rank has done GPU work (a late OverflowError would leave the other ranks in the gather)
        if not 0 < int(self.sim_size) <= 65535:
            raise ValueError(f"sim_size must be in 1..65535 (got {self.sim_size})")


@dataclass
class PartitionRecord:
    partition_id: int                    # 1-based position in processing order (reference)
    grid_id: int
    verdict: str
    h_attempt: int = 0
    h_success: int = 0
    b_comp: float = 0.0
    s_comp: float = 0.0
    st_comp: float = 0.0
    h_comp: float = 0.0
    t_comp: float = 0.0
    sv_time: float = 0.0
    s_time: float = 0.0
    hv_time: float = 0.0
    h_time: float = 0.0
    total_time: float = 0.0
    c_check: int = 0
    v_accurate: int = 0
    orig_acc: Optional[float] = None
    pruned_acc: float = 1.0
    c1: Optional[np.ndarray] = None
    c2: Optional[np.ndarray] = None
    nodes: int = 0
    stage: str = ""                      # which stage decided: sim / bab / heuristic


@dataclass
class ModelRun:
    model: str
    records: List[PartitionRecord] = field(default_factory=list)
    attempted: int = 0
    wall: float = 0.0
    stopped_by_hard_timeout: bool = False

    def counts(self) -> Dict[str, int]:
        c = {"sat": 0, "unsat": 0, "unknown": 0}
        for r in self.records:
            c[r.verdict] += 1
        return c


def _amortize(total: float, work: np.ndarray) -> np.ndarray:
    w = work.astype(np.float64) + 1.0
    return total * w / w.sum()


def verify_chunk(be: Backend, mlp: MLP, q: ResolvedQuery, grid: Grid, ids: np.ndarray, cfg: VerifyConfig,
                 orig_acc: Optional[float] = None, time_budget: Optional[float] = None,
                 timer: Optional[StageTimer] = None) -> "ChunkRecords":
    """Decide one chunk of partitions; returns its per-partition records (no cumulative columns).

    The kernels share one table of protected-attribute assignments per launch, so a chunk whose
    partitions split the PA range differently (a PA wider than the partition size, e.g. Adult
    age with P=10) is verified as one group per distinct PA range; the records come back in
    ``ids`` order with the chunk's stage times apportioned over all of its partitions."""
    lo_np, hi_np = grid.decode(ids)
    groups = pa_groups(q, lo_np, hi_np)
    if len(groups) <= 1:
        core, seg = _verify_group(GroupState(be, mlp, q, ids, lo_np, hi_np, grid, timer), cfg, time_budget)
    else:
        t0 = time.time()
        core, seg = None, np.zeros(5)
        for sel in groups:
            left = None if time_budget is None else time_budget - (time.time() - t0)
            gcore, gseg = _verify_group(GroupState(be, mlp, q, ids[sel], lo_np[sel], hi_np[sel], grid, timer), cfg, left)
            if core is None:
                core = {k: np.zeros((len(ids),) + v.shape[1:], dtype=v.dtype) for k, v in gcore.items()}
            for k, v in gcore.items():
                core[k][sel] = v
            seg += np.asarray(gseg, dtype=np.float64)
        seg = (len(ids),) + tuple(seg[1:].tolist())
    return ChunkRecords(core, orig_acc, segments=[seg], n_neurons=mlp.n_neurons, sim_size=cfg.sim_size)


class StreamPool:
    """Host threads, each driving its own HIP stream, that verify several chunks of one model
    concurrently (the native BaB level loop releases the GIL, so one chunk's host phases and
    synchronisations overlap the other chunks' kernels).  ``workers == 1`` runs inline."""

    def __init__(self, device: torch.device, workers: int):
        self.device = torch.device(device)
        self.workers = max(1, int(workers))
        self._tls = threading.local()
        self._pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 1 else None

    def _stream_ctx(self):
        if self.device.type != "cuda":
            return contextlib.nullcontext()
        if getattr(self._tls, "stream", None) is None:
            self._tls.stream = torch.cuda.Stream(self.device)
        return torch.cuda.stream(self._tls.stream)

    def run(self, fn: Callable, items: Sequence) -> List:
        """``[fn(item) for item in items]``, concurrently, results in item order."""
        def one(it):
            with self._stream_ctx():
                out = fn(it)
                if self.device.type == "cuda":
                    torch.cuda.current_stream(self.device).synchronize()
            return out

        if self._pool is None or len(items) <= 1:
            return [one(it) for it in items]
        return [f.result() for f in [self._pool.submit(one, it) for it in items]]

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)


def concat_records(parts: Sequence["ChunkRecords"]) -> "ChunkRecords":
    parts = [p for p in parts if len(p)]
    if not parts:
        raise ValueError("no records")
    if len(parts) == 1:
        return parts[0]
    keys = [k for k in parts[0].core if all(k in p.core for p in parts)]
    core = {k: np.concatenate([p.core[k] for p in parts]) for k in keys}
    segs = [sg for p in parts for sg in p.segments]
    return ChunkRecords(core, parts[0].orig_acc, segments=segs, n_neurons=parts[0].n_neurons,
                        sim_size=parts[0].sim_size)


CORE_COLUMNS = ("grid_id", "verdict", "stage", "h_attempt", "h_success", "b_cnt", "s_cnt", "st_cnt", "h_cnt",
                "t_cnt", "agree", "tp", "fp", "nodes", "c_check", "v_accurate", "cex_x", "cex_xp")


def derive_columns(core: Dict[str, np.ndarray], segments, n_neurons: int, sim_size: int) -> Dict[str, np.ndarray]:
    """The 24-column CSV quantities from the per-partition core columns.

    Compressions = dead counts / N (output neuron included, utils/prune.py:194-203); Pruned-acc
    = agreeing simulation points / sim_size; the stage times of every chunk segment
    ``(n, t_sim+prune+bab, t_bab, t_heur, t_replay)`` are apportioned over its partitions by
    work (BaB node expansions).  Pure function of its inputs, so rank 0 reproduces exactly what
    the producing rank would have written."""
    N = float(max(1, n_neurons))
    h = core["h_attempt"] > 0
    out = dict(core)
    out["b_comp"] = core["b_cnt"] / N
    out["s_comp"] = core["s_cnt"] / N
    out["st_comp"] = core["st_cnt"] / N
    out["h_comp"] = np.where(h, core["h_cnt"] / N, 0.0)
    out["t_comp"] = core["t_cnt"] / N
    out["pruned_acc"] = core["agree"] / float(max(1, sim_size))
    # F1 of the pruned net's labels against the original's on the simulation points (sklearn
    # f1_score(sim_y_orig, sim_y), zero_division -> 0): fn = S - agree - fp
    if "tp" in core:
        tp_, fp_ = core["tp"].astype(np.float64), core["fp"].astype(np.float64)
        fn_ = float(sim_size) - core["agree"] - fp_
        den = 2 * tp_ + fp_ + fn_
        out["pruned_f1"] = np.where(den > 0, 2 * tp_ / np.maximum(den, 1), 0.0)
    n = len(core["verdict"])
    s_t, sv_t, hv_t, rp_t = (np.zeros(n) for _ in range(4))
    off = 0
    for cnt, t_spb, t_bab, t_heur, t_rep in segments:
        cnt = int(cnt)
        sl = slice(off, off + cnt)
        work = core["nodes"][sl]
        s_t[sl] = _amortize(t_spb, work)
        sv_t[sl] = _amortize(t_bab, work)
        if t_heur > 0:
            hv_t[sl] = _amortize(t_heur, np.where(h[sl], work, 0))
        rp_t[sl] = _amortize(t_rep, np.zeros(cnt))
        off += cnt
    if off != n:
        raise ValueError(f"segments cover {off} partitions, records hold {n}")
    out["sv_time"], out["s_time"], out["hv_time"], out["h_time"] = sv_t, s_t, hv_t, hv_t
    out["total_time"] = s_t + hv_t + rp_t
    return out


class ChunkRecords(Sequence):
    """Per-partition results of one or more chunks, stored column-wise (numpy arrays).

    ``core`` holds what a rank ships (verdicts, stages, dead counts, work, counterexamples),
    ``segments`` the per-chunk stage times; ``cols`` adds the derived CSV quantities.  Behaves
    like a list of per-partition dicts (the CSV/runner view, built lazily per row)."""

    _INT = ("grid_id", "h_attempt", "h_success", "c_check", "v_accurate", "nodes")
    _HIDE = ("cex_x", "cex_xp", "b_cnt", "s_cnt", "st_cnt", "h_cnt", "t_cnt", "agree", "tp", "fp", "pruned_f1",
             "mask_bits", "stage_nodes")

    def __init__(self, core: Dict[str, np.ndarray], orig_acc: Optional[float] = None, segments=None,
                 n_neurons: int = 1, sim_size: int = 1):
        self.core = core
        self.orig_acc = orig_acc
        self.segments = list(segments) if segments is not None else [(len(core["verdict"]), 0.0, 0.0, 0.0, 0.0)]
        self.n_neurons = n_neurons
        self.sim_size = sim_size
        self.cols = derive_columns(core, self.segments, n_neurons, sim_size)

    def __len__(self) -> int:
        return len(self.cols["verdict"])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        c = self.cols
        sat = c["verdict"][i] == "sat"
        d = {k: (int(v[i]) if k in self._INT else (str(v[i]) if v.dtype.kind in "OU" else float(v[i])))
             for k, v in c.items() if k not in self._HIDE}
        d["orig_acc"] = self.orig_acc
        d["c1"] = c["cex_x"][i].astype(np.float32) if sat else None
        d["c2"] = c["cex_xp"][i].astype(np.float32) if sat else None
        return d

    def counts(self) -> Dict[str, int]:
        v = self.cols["verdict"]
        return {"sat": int((v == "sat").sum()), "unsat": int((v == "unsat").sum()),
                "unknown": int((v == "unknown").sum())}


def sample_host(lo: np.ndarray, hi: np.ndarray, pid: int, n_samples: int, seed: int) -> np.ndarray:
    X = sample_points(torch.from_numpy(lo[None]).float(), torch.from_numpy(hi[None]).float(),
                      torch.tensor([pid]), n_samples, seed)
    return X[0].numpy().astype(np.int64)


def verify_model(mlp: MLP, q: ResolvedQuery, grid: Grid, order: np.ndarray, cfg: VerifyConfig,
                 device="cpu", orig_acc: Optional[float] = None,
                 on_chunk: Optional[Callable[[List[PartitionRecord]], None]] = None,
                 max_partitions: Optional[int] = None) -> ModelRun:
    """Verify partitions of ``grid`` in ``order`` (ids) until done or the hard timeout."""
    be = Backend(mlp, device=device)
    run = ModelRun(model=mlp.name)
    t0 = time.time()
    total = len(order) if max_partitions is None else min(len(order), max_partitions)
    pos = 0
    while pos < total:
        elapsed = time.time() - t0
        if elapsed > cfg.hard_timeout:
            run.stopped_by_hard_timeout = True
            break
        ids = order[pos:min(total, pos + cfg.chunk)]
        recs = verify_chunk(be, mlp, q, grid, ids, cfg, orig_acc=orig_acc,
                            time_budget=cfg.hard_timeout - elapsed)
        out = []
        for r in recs:
            out.append(PartitionRecord(partition_id=pos + len(out) + 1, **r))
        run.records.extend(out)
        pos += len(ids)
        if on_chunk is not None:
            on_chunk(out)
    run.attempted = len(run.records)
    run.wall = time.time() - t0
    return run
