#!/usr/bin/env python
"""Micro-benchmark of one beta-CROWN BaB level: per-node kernel (arm A, fa_beta_kernel) against the
two-phase batched level (arm B: fa_beta_opt16_kernel, then fa_beta_kernel at iters = 0).

A fixed synthetic node set per network: seeded integer boxes, one binary PA dim, each copy's
partition bounds over its box, alternating orientations, and 15 % of the neurons fixed to the phase they take at a seeded
point of the box (so the regions are non-empty and the optimiser runs its full course).
Arms alternate on one device; times are device times between events, parameters re-initialised
outside the timed region.

Infeasibility arm (--feas-iters, default 64; 0: off): the pass alone (hip.beta_feas) on the rows the
per-node level leaves open with a fixed phase, at that level's best parameters and the roots' step
sizes -- the per-node pass against the two-phase one (proposals by the feas mode of
fa_beta_opt16_kernel, decision by fa_beta_kernel at iters = 0); closed counts of both reported.

    python tools/bench_beta_level.py [--nets AC-7,BM-8,AC-4] [--R 32768] [--iters 128] [--lookahead 8]
                                     [--runs 3] [--feas-iters 64] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fairify_amd.models.zoo import get_model  # noqa: E402
from fairify_amd.ops import hip  # noqa: E402
from fairify_amd.ops.backend import Backend  # noqa: E402


def node_set(be, m, R, seed, fix=0.15):
    dev = be.device
    g = torch.Generator().manual_seed(seed)
    n0, NH = int(np.asarray(m.weights[0]).shape[0]), be.n_hidden
    pa = [1]
    lo = torch.randint(0, 6, (R, n0), generator=g).float()
    hi = lo + torch.randint(0, 3, (R, n0), generator=g).float()
    lo[:, pa] = 0
    hi[:, pa] = 1
    x = lo + torch.floor(torch.rand(R, n0, generator=g) * (hi - lo + 1)).clamp(max=hi - lo)
    va, vb = torch.zeros(R, 1), torch.ones(R, 1)
    bnd, ph = [], []
    for v in (va, vb):
        rl, rh, xv = lo.clone(), hi.clone(), x.clone()
        rl[:, pa] = v
        rh[:, pa] = v
        xv[:, pa] = v
        res = be.bounds(rl.to(dev), rh.to(dev), keep_layers=True)
        lb = torch.cat(res.layer_lb, 1)[:, :NH].float()
        ub = torch.cat(res.layer_ub, 1)[:, :NH].float()
        # pre-activations at the point: the phases fixed are satisfiable together
        h, zs = xv.double(), []
        for W, b in list(zip(m.weights, m.biases))[:-1]:
            z = h @ torch.tensor(np.asarray(W), dtype=torch.float64) + torch.tensor(np.asarray(b), dtype=torch.float64)
            zs.append(z)
            h = z.clamp(min=0)
        z = torch.cat(zs, 1)
        pick = torch.rand(R, NH, generator=g) < fix
        p = torch.where(pick, torch.where(z >= 0, 1, -1), 0).to(torch.int8)
        bnd.append((lb, ub))
        ph.append(p.to(dev))
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    # orientations alternate: whatever the logit's sign over a box, one of each pair of nodes is open
    osg = d(torch.tensor([1, -1], dtype=torch.int8).repeat((R + 1) // 2)[:R])
    return dict(lo=d(lo), hi=d(hi), pa=pa, va=d(va), vb=d(vb), bnd=bnd, ph=ph, R=R, NH=NH, seed=seed, osg=osg)


def fresh(ns, dev):
    g = torch.Generator().manual_seed(ns["seed"] + 1)
    R, NH = ns["R"], ns["NH"]
    al = [torch.rand(R, NH, generator=g).to(dev) for _ in range(2)]
    be_ = [torch.zeros(R, NH, device=dev) for _ in range(2)]
    t = torch.full((R,), 0.5, device=dev)
    return al, be_, t


def timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="AC-7,BM-8,AC-4")
    ap.add_argument("--R", type=int, default=32768)
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--lookahead", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--feas-iters", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    lr = dict(lr_a=0.03, lr_b=0.15, lr_t=0.03)      # the children's steps (BetaConfig: lr x child_lr)
    rows = []
    for name in a.nets.split(","):
        m = get_model(name, weights="zoo", seed=0)
        be = Backend(m, dev)
        ns = node_set(be, m, a.R, 7)
        common = (ns["lo"], ns["hi"], ns["pa"], ns["va"], ns["vb"], ns["bnd"][0][0], ns["bnd"][0][1], ns["bnd"][1][0],
                  ns["bnd"][1][1], ns["ph"][0], ns["ph"][1])

        def level(batched):
            al, be_, t = fresh(ns, dev)
            return timed(lambda: hip.beta_level(be, *common, al[0], al[1], be_[0], be_[1], t, a.iters, decay=0.98,
                                                lookahead=a.lookahead, pgap=1, osg=ns["osg"], batched=batched,
                                                **lr), dev)

        def phase1():
            al, be_, t = fresh(ns, dev)
            return timed(lambda: hip.beta_opt16(be, *common, al[0], al[1], be_[0], be_[1], t, a.iters, lr["lr_a"],
                                                lr["lr_b"], lr["lr_t"], decay=0.98, pgap=1, osg=ns["osg"]), dev)

        level(False), level(True)            # warm-up (module load, allocator)
        tA, tB, t1 = [], [], []
        for _ in range(a.runs):              # alternating arms
            msA, la = level(False)
            msB, lb = level(True)
            ms1, _ = phase1()
            tA.append(msA), tB.append(msB), t1.append(ms1)
        ca, cb = int((la.bound >= 0).sum()), int((lb.bound >= 0).sum())
        row = dict(net=name, R=a.R, iters=a.iters, lookahead=a.lookahead, per_node_ms=tA, batched_ms=tB,
                   batched_phase1_ms=t1, per_node_closed=ca, batched_closed=cb,
                   mean_bound_per_node=float(la.bound[torch.isfinite(la.bound)].mean()),
                   mean_bound_batched=float(lb.bound[torch.isfinite(lb.bound)].mean()))
        if a.feas_iters > 0:
            al, be_, t = fresh(ns, dev)
            lev = hip.beta_level(be, *common, al[0], al[1], be_[0], be_[1], t, a.iters, decay=0.98,
                                 lookahead=a.lookahead, pgap=1, osg=ns["osg"], **lr)
            fixed = (ns["ph"][0] != 0).any(1) | (ns["ph"][1] != 0).any(1)
            idx = torch.nonzero((lev.bound < 0) & fixed).flatten()
            sub = [x[idx].contiguous() for x in common[:2] + common[3:]]
            rest = (al[0][idx].contiguous(), al[1][idx].contiguous(), t[idx].contiguous(), lev.bound[idx].contiguous())

            def feas(batched):
                return timed(lambda: hip.beta_feas(be, sub[0], sub[1], ns["pa"], *sub[2:], *rest, a.feas_iters,
                                                   (0.1, 0.5, 0.1), batched, decay=0.98, osg=ns["osg"][idx]), dev)

            tFa, tFb, fa, fb = [], [], None, None
            if idx.numel():
                feas(False), feas(True)
                for _ in range(a.runs):
                    msA, fa = feas(False)
                    msB, fb = feas(True)
                    tFa.append(msA), tFb.append(msB)
            row.update(feas_iters=a.feas_iters, feas_rows=int(idx.numel()), feas_per_node_ms=tFa, feas_batched_ms=tFb,
                       feas_per_node_closed=int(fa[0].sum()) if fa else 0,
                       feas_batched_closed=int(fb[0].sum()) if fb else 0)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
