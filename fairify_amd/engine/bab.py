"""Batched branch-and-bound decision procedure for the fairness query (K8 + K9).

The reference decides a partition with one Z3 ``check()`` under a soft timeout
(src/AC/Verify-AC.py:127-163).  Z3 is not part of this framework; instead every partition of a
chunk is decided *together* by a device-resident branch-and-bound over the integer lattice:

* a node is an integer sub-box of the partition (plus, for relaxed attributes, a box for x');
* its rows (one per protected-attribute assignment v) are bounded with the symbolic bound
  propagation kernel, and :func:`pair_certify` proves "no violating pair inside" (node closed)
  or returns the most violating pair, a split dimension and a candidate vertex pair;
* candidates are evaluated with the fp32 forward + rounding bound and confirmed exactly on the
  host (``engine.exact``), so SAT answers are true counterexamples;
* leaves are single lattice points, evaluated exactly — the procedure is complete on the finite
  domain, budgets (nodes per partition, wall clock) turn the remainder into UNKNOWN.

All node bookkeeping is tensor code on the device; the only host round trip per iteration is the (tiny)
SAT-candidate list.  The torch loop here (state ``_TorchSearch``, one function per step) is what the CPU tier
tests; a HIP device runs csrc/bab_runtime.cpp.  Verdict codes, result record, PA grouping: engine/search.py.
"""
from __future__ import annotations

import os
import threading
import time
from collections import namedtuple
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..models.mlp import MLP
from ..ops.backend import Backend
from ..spec import ResolvedQuery
from ..utils.timer import NULL, StageTimer
from . import exact
from .search import (RUNNING, SAT, UNKNOWN, UNSAT, VERDICT_NAMES, BaBResult, Verdicts, clamp_tau,  # noqa: F401
                     confirm_pairs, halve, pa_groups, pa_table, pool_overflow, solve_pa_groups)
from .search import pa_table as _pa_table  # noqa: F401  (test modules of the parent commit import it from here)

# process-wide native-runtime counters (diagnostics: tools/diag_shard_diff.py, bench --profile)
STATS: Dict[str, int] = {"levels": 0, "launches": 0, "cand_overflow_levels": 0}
_STATS_LOCK = threading.Lock()


@dataclass
class BaBConfig:
    node_budget: int = 4096          # max node expansions per partition (soft-timeout analogue)
    batch_nodes: int = 32768         # nodes bounded per iteration
    max_pool: int = 1 << 24          # live-node capacity per runtime (grown lazily; UNKNOWN beyond)
    time_budget: float = 1e9         # wall-clock seconds for the whole call
    mode: str = "symbolic"
    cand_cap: int = 1 << 17          # candidate pairs confirmed per BFS level (native runtime)
    crown: bool = os.environ.get("FAIRIFY_CROWN", "1") != "0"   # backward output bounds per node
    # hidden-layer bounds tightened by back-substitution before the output pass (csrc/refine.hip):
    # "auto" = networks with >= 3 hidden layers of which one is >= 10 wide (AC-7's residue closes
    # in ~800 nodes instead of > 32 768; on 1-2 hidden layers it equals the forward bounds), "on", "off"
    refine: str = os.environ.get("FAIRIFY_REFINE", "auto")
    # native runtime input-split scores: "auto" = first-layer smear (CertArgs.smear) for networks
    # whose first hidden layer is >= 32 wide (AC-2/3/4/5/7; the narrow deep nets keep the
    # certificate scores), "on", "off"
    smear: str = os.environ.get("FAIRIFY_SMEAR", "auto")
    # native runtime: the level end (fa_settle) runs in the level's last split launch (its last
    # workgroup) instead of its own launch.  Off: the device-scope release fence every workgroup
    # needs before counting itself done writes back the XCD's L2 (the level's children pool), and
    # cost more than the launch it saves (N=1 944 -> 1 011 ms/step, 1/8 shard 141 -> 169 ms,
    # profiles/r4/ab_fuse_settle.md)
    fuse_settle: bool = os.environ.get("FAIRIFY_FUSE_SETTLE", "0") == "1"
    # native runtime branching rule: a partition with w nodes in a BFS level splits each along
    # clamp(log2(split_target / w), 1, 6) dims (per partition: verdicts do not depend on which
    # partitions share a chunk)
    split_target: int = int(os.environ.get("FAIRIFY_SPLIT_TARGET", "256"))
    # native runtime inline escalation: a partition that reaches node_budget with a frontier of at
    # most escalate_max_w nodes continues up to escalate_budget (0 = off)
    escalate_budget: int = 0
    escalate_max_w: int = 0
    # intermediate (budget, max frontier) steps of the inline escalation, between node_budget and
    # escalate_budget: a partition continues past step k's budget only with a frontier of at most
    # its limit (fa_settle_kernel)
    escalate_steps: Tuple[Tuple[int, int], ...] = ()


def refine_level(mode: str, widths) -> int:
    """How the BaB bounds its nodes (BaBConfig.refine): 0 forward symbolic + backward output pass,
    1 with back-substituted hidden-layer bounds between them (csrc/refine.hip), 2 back-substitution
    alone (one launch, no forward pass).  ``auto``: level 1 for networks with at least 3 hidden
    layers, one of them at least 10 wide -- with 1-2 hidden layers the refined bounds equal the
    forward ones, and on the narrow deep nets (AC-9/10/12, 3-5 wide) the extra pass costs more than
    it closes (tools/diag_open_nodes.py on the bench residue)."""
    if mode in ("on", "refine"):
        return 1
    if mode == "full":
        return 2
    if mode != "auto":
        return 0
    hidden = list(widths)[:-1]
    return 1 if (len(hidden) >= 3 and max(hidden) >= 10) else 0


def smear_on(mode: str, widths) -> bool:
    """First-layer smear split scores in the native runtime (BaBConfig.smear)."""
    if mode == "on":
        return True
    if mode != "auto":
        return False
    return len(widths) >= 2 and int(widths[0]) >= 32


def refine_on(mode: str, widths) -> bool:
    """Hidden-layer bounds tightened by back-substitution (any level > 0 of :func:`refine_level`)."""
    return refine_level(mode, widths) > 0


# nodes of the torch loop: x boxes, x' boxes (full rows; the x tensors themselves for a PA-only query), partitions
_Nodes = namedtuple("_Nodes", "lo hi plo phi part")


class _TorchSearch:
    """State of the torch loop over one PA group: the PA table, the device status / node counts the loop
    works on, the FIFO pool (a root per RUNNING partition)."""

    def __init__(self, sol: "BaBSolver", lo_np, hi_np, v: Verdicts, values_np, pairs_np):
        dev = sol.dev
        self.values = torch.from_numpy(values_np).to(dev)
        self.pairs = torch.from_numpy(pairs_np).to(dev)
        run_idx = np.nonzero(v.status == RUNNING)[0]
        xlo = torch.from_numpy(lo_np[run_idx]).to(dev, torch.float32)
        xhi = torch.from_numpy(hi_np[run_idx]).to(dev, torch.float32)
        xplo, xphi = xlo, xhi
        if sol.relaxed:
            xplo, xphi = xlo.clone(), xhi.clone()
            xplo[:, sol.ra] -= sol.tau
            xphi[:, sol.ra] += sol.tau
        self.pool = _Nodes(xlo, xhi, xplo, xphi, torch.from_numpy(run_idx).to(dev))
        self.status_t = torch.from_numpy(v.status).to(dev)
        self.nodes_t = torch.zeros(len(v.status), dtype=torch.long, device=dev)


class BaBSolver:
    def __init__(self, backend: Backend, query: ResolvedQuery, cfg: BaBConfig, dead: Optional[torch.Tensor] = None,
                 timer: StageTimer = NULL):
        self.tm = timer
        self.be = backend
        self.q = query
        self.cfg = cfg
        self.dev = backend.device
        self.dead = dead            # optional [P, N_hidden] bool (heuristically pruned nets)
        self.pa = torch.tensor(list(query.pa_idx), dtype=torch.long, device=self.dev)
        self.ra = torch.tensor(list(query.ra_idx), dtype=torch.long, device=self.dev)
        shared = np.ones(query.n, dtype=bool)
        shared[list(query.ra_idx)] = False
        self.shared = torch.from_numpy(shared).to(self.dev)     # PA dims are fixed per row -> "shared" ok
        self.relaxed = query.relaxed
        self.tau = float(query.tau)

    # --------------------------------------------------------------------------------------
    def _rows(self, lo: torch.Tensor, hi: torch.Tensor, values: torch.Tensor):
        """Expand node boxes [N, n] into node-major rows [N*V, n] with PA dims set to v."""
        N, n = lo.shape
        V = values.shape[0]
        rlo = lo[:, None, :].expand(N, V, n).clone()
        rhi = hi[:, None, :].expand(N, V, n).clone()
        vv = values.to(lo.dtype)[None, :, :].expand(N, V, values.shape[1])
        rlo[:, :, self.pa] = vv
        rhi[:, :, self.pa] = vv
        return rlo.reshape(N * V, n), rhi.reshape(N * V, n)

    def _eval_pairs(self, x: torch.Tensor, xp: torch.Tensor, part: torch.Tensor):
        """Rigorous evaluation of point pairs (value + running error bound that keeps exact
        zeros exact): returns (certain_violation, possible_but_uncertain) masks."""
        d = self.dead[part] if self.dead is not None else None
        xlb, xub = self.be.point_bounds(x, d)
        plb, pub = self.be.point_bounds(xp, d)
        sure = ((xub < 0) & (plb > 0)) | ((xlb > 0) & (pub < 0))
        poss = ((xlb < 0) & (pub > 0)) | ((xub > 0) & (plb < 0))
        return sure, poss & ~sure

    # --------------------------------------------------------------------------------------
    def solve(self, lo_np: np.ndarray, hi_np: np.ndarray, mlp_exact: MLP, init_status: Optional[np.ndarray] = None,
              exact_models: Optional[List[MLP]] = None) -> BaBResult:
        """Decide every partition box ``[lo_np[p], hi_np[p]]``.  ``mlp_exact`` is the network used for exact
        confirmation (per-partition nets in ``exact_models`` when heuristic masks are active)."""
        t0 = time.time()
        groups = pa_groups(self.q, lo_np, hi_np)
        if len(groups) > 1:
            return self._solve_groups(groups, lo_np, hi_np, mlp_exact, init_status, exact_models, t0)
        values_np, pairs_np = pa_table(self.q, lo_np, hi_np)
        v = Verdicts(*lo_np.shape, init_status)
        if pairs_np.shape[0] == 0:
            return v.close_running(UNSAT).result(t0)    # a single PA value: no x' can differ
        if self.be.hip and os.environ.get("FAIRIFY_TORCH_BAB") != "1":
            return self._solve_native(lo_np, hi_np, v.status, values_np, pairs_np, mlp_exact, exact_models, t0)
        s, it = _TorchSearch(self, lo_np, hi_np, v, values_np, pairs_np), 0
        while s.pool.part.shape[0] > 0:
            if time.time() - t0 > self.cfg.time_budget:
                break
            it += 1
            b = self._take_batch(s)
            if b is None:
                continue
            dec = self._bound(s, b)
            cx, cxp, leaf, sel, found = self._candidates(s, b, dec)
            found += self._leaves(s, b, torch.nonzero(leaf & sel).flatten(), cx, cxp)
            if found:
                rows = torch.cat(found)
                with self.tm("bab.confirm"):   # in the order found; new SATs go into the device status too
                    newly = confirm_pairs(v, self.q, lo_np, hi_np, mlp_exact, b.part[rows].cpu().numpy(), cx[rows],
                                          cxp[rows], exact_models, lex_order=False)
                    if newly:
                        s.status_t[torch.tensor(newly, device=s.status_t.device)] = SAT
            self._update_pool(s, b, dec, leaf)
        # partitions still running: no nodes left => UNSAT ; nodes left (time budget) => UNKNOWN.  The
        # device status holds the budget / pool UNKNOWNs; the SATs confirmed on the host override it
        v.status[:] = np.where(v.status == SAT, SAT, s.status_t.cpu().numpy())
        v.nodes = s.nodes_t.cpu().numpy()
        return v.sweep(s.pool.part.cpu().numpy()).result(t0, it)

    def _each(self, fn, *sets) -> _Nodes:
        """``fn`` over the columns of node sets; a PA-only query keeps x' an alias of x."""
        lo, hi, plo, phi, part = zip(*sets)
        lo, hi = fn(*lo), fn(*hi)
        return _Nodes(lo, hi, fn(*plo) if self.relaxed else lo, fn(*phi) if self.relaxed else hi, fn(*part))

    def _take_batch(self, s: _TorchSearch) -> Optional[_Nodes]:
        """The pool's first ``batch_nodes`` nodes without those of decided partitions (None: none left)."""
        B = min(self.cfg.batch_nodes, s.pool.part.shape[0])
        b = self._each(lambda t: t[:B], s.pool)
        s.pool = self._each(lambda t: t[B:], s.pool)
        alive = s.status_t[b.part] == RUNNING
        if not bool(alive.all()):
            b = self._each(lambda t: t[alive], b)
        if b.part.shape[0] == 0:
            return None
        s.nodes_t.index_add_(0, b.part, torch.ones_like(b.part))
        return b

    def _bound(self, s: _TorchSearch, b: _Nodes):
        """Symbolic bounds of the batch's rows (one per PA assignment) and the pair certificate."""
        cfg = self.cfg
        dead_rows = None if self.dead is None else self.dead[b.part].repeat_interleave(s.values.shape[0], dim=0)
        with self.tm("bab.bounds"):
            rlo, rhi = self._rows(b.lo, b.hi, s.values)
            rf = refine_on(cfg.refine, self.be.widths)
            res_x = self.be.bounds(rlo, rhi, mode=cfg.mode, dead=dead_rows, crown=cfg.crown, refine=rf)
            if self.relaxed:
                plo, phi = self._rows(b.plo, b.phi, s.values)
                res_xp = self.be.bounds(plo, phi, mode=cfg.mode, dead=dead_rows, crown=cfg.crown, refine=rf)
            else:
                res_xp = res_x
        with self.tm("bab.certify"):
            return self.be.pair_certify(res_x, res_xp, b.lo, b.hi, b.plo, b.phi, s.pairs, s.values, self.pa,
                                        self.shared, self.relaxed)

    def _candidates(self, s: _TorchSearch, b: _Nodes, dec):
        """Candidate vertex pairs (falsification inside BaB): the pairs, the leaf mask, the open nodes of
        running partitions, and (a list) the rows whose pair the rigorous evaluation cannot rule out."""
        values, pv = s.values, s.pairs[dec.cand_v]
        cx, cxp = dec.cand_x.clone(), dec.cand_xp.clone()
        cx[:, self.pa] = values[pv[:, 0]].to(cx.dtype)
        cxp[:, self.pa] = values[pv[:, 1]].to(cx.dtype)
        if self.relaxed:
            r = self.ra
            cxp[:, r] = clamp_tau(cxp[:, r], cx[:, r], self.tau)
            cxp[:, r] = torch.minimum(torch.maximum(cxp[:, r], b.plo[:, r]), b.phi[:, r])
        # leaves: single lattice points (x and x')
        wmask = torch.ones(b.lo.shape[1], dtype=torch.bool, device=b.lo.device)
        wmask[self.pa] = False
        width = (b.hi - b.lo)[:, wmask].amax(dim=1)
        if self.relaxed:
            width = torch.maximum(width, (b.phi - b.plo)[:, self.ra].amax(dim=1) if self.ra.numel() else width)
        leaf = dec.open_ & (width == 0)
        sel = dec.open_ & (s.status_t[b.part] == RUNNING)
        cand_rows = torch.nonzero(sel & ~leaf).flatten()
        found = []
        if cand_rows.numel():
            with self.tm("bab.eval_cand"):
                sure, amb = self._eval_pairs(cx[cand_rows], cxp[cand_rows], b.part[cand_rows])
            hit = cand_rows[sure | amb]
            if hit.numel():
                found.append(hit)
        return cx, cxp, leaf, sel, found

    def _leaves(self, s: _TorchSearch, b: _Nodes, leaf_rows: torch.Tensor, cx, cxp) -> list:
        """All PA pairs at the leaf points: the leaves with a possible violation (its pair put into cx / cxp)."""
        if not leaf_rows.numel():
            return []
        values, pairs, n = s.values, s.pairs, b.lo.shape[1]
        L_, Pp = leaf_rows.numel(), pairs.shape[0]
        px = b.lo[leaf_rows][:, None, :].expand(L_, Pp, n).clone()
        ppx = b.plo[leaf_rows][:, None, :].expand(L_, Pp, n).clone()
        px[:, :, self.pa] = values[pairs[:, 0]].to(px.dtype)[None].expand(L_, Pp, -1)
        ppx[:, :, self.pa] = values[pairs[:, 1]].to(px.dtype)[None].expand(L_, Pp, -1)
        lp = b.part[leaf_rows][:, None].expand(L_, Pp)
        sure, amb = self._eval_pairs(px.reshape(-1, n), ppx.reshape(-1, n), lp.reshape(-1))
        flag = (sure | amb).view(L_, Pp)
        anyf = flag.any(dim=1)
        if not bool(anyf.any()):
            return []
        first = flag.float().argmax(dim=1)
        sel_l = torch.nonzero(anyf).flatten()
        cx[leaf_rows[sel_l]] = px[sel_l, first[sel_l]]
        cxp[leaf_rows[sel_l]] = ppx[sel_l, first[sel_l]]
        return [leaf_rows[sel_l]]

    def _update_pool(self, s: _TorchSearch, b: _Nodes, dec, leaf: torch.Tensor) -> None:
        """Open non-leaf nodes of running partitions split while the partition is within its node budget
        (the device-side count), else it ends UNKNOWN; next pool = rest + children, cut to ``max_pool``."""
        cfg = self.cfg
        grow = dec.open_ & ~leaf & (s.status_t[b.part] == RUNNING)
        budget_ok = s.nodes_t[b.part] < cfg.node_budget
        over = grow & ~budget_ok
        if bool(over.any()):
            s.status_t[b.part[over]] = UNKNOWN
        sidx = torch.nonzero(grow & budget_ok).flatten()
        with self.tm("bab.split"):
            kids = self._split(*(t[sidx] for t in b), dec.split_dim[sidx])
        s.pool = self._each(lambda rest, new: torch.cat([rest, new]), s.pool, kids)
        if s.pool.part.shape[0] > cfg.max_pool:     # keep the oldest nodes; partitions losing nodes become UNKNOWN
            pool_overflow(s.pool.part, cfg.max_pool, s.status_t)
            s.pool = self._each(lambda t: t[:cfg.max_pool], s.pool)

    def _solve_groups(self, groups, lo_np, hi_np, mlp_exact, init_status, exact_models, t0) -> BaBResult:
        """Partitions with different PA ranges: a sub-solver per PA group, with the group's rows of the
        forced-dead masks and its masked exact models; ``open_left`` zeros where a group reports none."""
        def one(g, status_g, left):
            sub = BaBSolver(self.be, self.q, replace(self.cfg, time_budget=left),
                            dead=None if self.dead is None else self.dead[torch.from_numpy(g).to(self.dead.device)],
                            timer=self.tm)
            em = None if exact_models is None else [exact_models[int(k)] for k in g]
            return sub.solve(lo_np[g], hi_np[g], mlp_exact, init_status=status_g, exact_models=em)

        return solve_pa_groups(groups, lo_np, hi_np, init_status, self.cfg.time_budget, t0, one, open_left=True)

    # --------------------------------------------------------------------------------------
    def _runtime(self, values_np: np.ndarray, pairs_np: np.ndarray, n_run: int):
        """Native (C++/HIP) BaB runtime checked out of the backend's pool (engine/rtpool.py)."""
        from ..ops import ext
        from ..ops.hip import _net
        from .rtpool import checkout

        rf = refine_level(self.cfg.refine, self.be.widths)
        sm = smear_on(self.cfg.smear, self.be.widths)
        key = (tuple(self.q.pa_idx), tuple(self.q.ra_idx), self.q.tau, values_np.tobytes(), pairs_np.tobytes(),
               bool(self.cfg.crown), int(self.cfg.split_target), rf, sm)
        shared = np.ones(self.q.n, dtype=np.uint8)
        shared[list(self.q.ra_idx)] = 0

        def make(cap):
            return ext().BabRuntime(_net(self.be), self.be.flat.data_ptr(), list(self.q.pa_idx),
                                    values_np.astype(np.float32).reshape(-1).tolist(),
                                    values_np.astype(np.int64).reshape(-1).tolist(),
                                    pairs_np.astype(np.int64).reshape(-1).tolist(),
                                    list(self.q.ra_idx) if self.relaxed else [], float(self.q.tau),
                                    shared.tolist(), int(cap), int(self.cfg.batch_nodes), int(self.cfg.cand_cap),
                                    float(self.be.unit), bool(self.cfg.crown), int(self.cfg.split_target), rf, sm,
                                    self.be.flat)

        return checkout(self.be, "_bab_rt", key, max(self.cfg.max_pool, n_run), make)

    def _solve_native(self, lo_np, hi_np, status, values_np, pairs_np, mlp_exact, exact_models, t0) -> BaBResult:
        n_run = int((status == RUNNING).sum())
        check = exact.make_confirm(mlp_exact, lo_np, hi_np, self.q, exact_models)

        def confirm(parts: np.ndarray, buf: np.ndarray) -> np.ndarray:
            with self.tm("bab.confirm"):
                return check(parts, buf)

        dead_ptr = 0
        if self.dead is not None:
            self._dead_u8 = self.dead.to(torch.uint8).contiguous()
            dead_ptr = self._dead_u8.data_ptr()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        with self.tm("bab.native"), self._runtime(values_np, pairs_np, n_run) as rt:
            rt.set_fuse_settle(bool(self.cfg.fuse_settle))
            st, cx, cxp, nodes, stats = rt.solve(lo_np.astype(np.float32), hi_np.astype(np.float32), status,
                                                  int(self.cfg.node_budget), float(self.cfg.time_budget), dead_ptr,
                                                  confirm, stream, exact_models is None,
                                                  int(self.cfg.escalate_budget), int(self.cfg.escalate_max_w),
                                                  [(int(b), int(o)) for b, o in self.cfg.escalate_steps])
        self.stats = dict(stats)
        with _STATS_LOCK:
            for k in STATS:
                STATS[k] += int(self.stats.get(k, 0))
        return BaBResult(np.asarray(st, dtype=np.int8), np.asarray(cx), np.asarray(cxp), np.asarray(nodes),
                         int(stats["levels"]), time.time() - t0, open_left=np.asarray(stats["open_left"]))

    def _split(self, lo, hi, plo, phi, part, dim):
        n = lo.shape[1]
        if lo.shape[0] == 0:
            return lo[:0], lo[:0], lo[:0], lo[:0], part[:0]
        # children along x dim or x' dim
        on_x = dim < n
        d = torch.where(on_x, dim, dim - n)
        xs, ps = torch.nonzero(on_x).flatten(), torch.nonzero(~on_x).flatten()
        lo1, hi1, lo2, hi2 = halve(lo, hi, xs, d[xs])
        plo1, phi1, plo2, phi2 = halve(plo, phi, ps, d[ps])
        clo, chi, cpart = torch.cat([lo1, lo2]), torch.cat([hi1, hi2]), torch.cat([part, part])
        cplo, cphi = torch.cat([plo1, plo2]), torch.cat([phi1, phi2])
        if not self.relaxed:
            return clo, chi, clo, chi, cpart
        # shared dims of x' follow x; tighten the |x_r - x'_r| <= tau coupling
        cplo = torch.where(self.shared[None, :], clo, cplo)
        cphi = torch.where(self.shared[None, :], chi, cphi)
        r, t = self.ra, self.tau
        cplo[:, r] = torch.maximum(cplo[:, r], clo[:, r] - t)
        cphi[:, r] = torch.minimum(cphi[:, r], chi[:, r] + t)
        clo[:, r] = torch.maximum(clo[:, r], cplo[:, r] - t)
        chi[:, r] = torch.minimum(chi[:, r], cphi[:, r] + t)
        ok = torch.all(clo <= chi, dim=1) & torch.all(cplo <= cphi, dim=1)
        return clo[ok], chi[ok], cplo[ok], cphi[ok], cpart[ok]
