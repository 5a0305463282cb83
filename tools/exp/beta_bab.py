#!/usr/bin/env python
"""CPU prototype (fp64 torch, batched, analytic gradients) of the beta-CROWN ReLU-phase BaB that
round 5 puts on the GPU: per node the coupled bound  min_x t N(x, va) - (1 - t) N(x, vb)  over the
node box with the node's phase constraints, slopes alpha, split multipliers beta and t optimised by
projected Adam; children WARM-START from their parent's (alpha, beta, t).  Intermediate bounds are
the partition root's rigorous per-layer bounds (the verified LP's, smt/milp.py:layer_bounds_rows),
clamped by the phases.  Compare node counts with the LP (profiles/r4/lp_tree_sizes_ac7_trained.jsonl).

    python tools/exp/beta_bab.py --model AC-7 --pids 12596,4387,6769 --iters 20
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def backward(ws, bs, LB, UB, ph, al, be, scale):
    """Backward pass of ONE copy for rows R: objective scale[R] * logit.  LB/UB: per hidden layer
    [R, w] phase-clamped pre-activation bounds; ph/al/be: per hidden layer [R, w].  Returns the
    input coefficients [R, n0], the constant [R] and per layer (lam_h, mu, kind) for the gradient
    (kind: 0 dead, 1 active, 2 unstable lower (alpha), 3 unstable upper (chord))."""
    L = len(ws)
    lam = scale[:, None] * ws[L - 1][:, 0][None]
    c = scale * bs[L - 1][0]
    rec = [None] * (L - 1)
    for l in range(L - 2, -1, -1):
        lb, ub, p = LB[l], UB[l], ph[l]
        dead = (ub <= 0) | (p < 0)
        act = ((lb >= 0) | (p > 0)) & ~dead
        un = ~(dead | act)
        low = un & (lam >= 0)
        upp = un & (lam < 0)
        den = torch.where(un, ub - lb, torch.ones_like(ub))
        s = torch.where(un, ub / den, torch.zeros_like(ub))
        slope = torch.where(act, torch.ones_like(ub), torch.where(low, al[l], torch.where(upp, s, torch.zeros_like(ub))))
        mu = lam * slope
        c = c + torch.where(upp, -mu * lb, torch.zeros_like(ub)).sum(1)
        mu = mu - be[l] * p.to(mu.dtype)
        c = c + (mu * bs[l][None]).sum(1)
        kind = torch.where(dead, 0, torch.where(act, 1, torch.where(low, 2, 3)))
        rec[l] = (lam, mu, kind, s)
        lam = mu @ ws[l].T
    return lam, c, rec


def forward_lin(ws, bs, x, LB, rec, al):
    """Pre-activations of the linearised network (the relaxation each neuron used) at x [R, n0]."""
    h = x
    zs = []
    for l in range(len(ws) - 1):
        z = h @ ws[l] + bs[l][None]
        zs.append(z)
        lam, mu, kind, s = rec[l]
        h = torch.where(kind == 1, z, torch.where(kind == 2, al[l] * z, torch.where(kind == 3, s * (z - LB[l]),
                                                                                     torch.zeros_like(z))))
    return zs, (h @ ws[-1] + bs[-1][None])[:, 0]


def pair_bound(net, lo, hi, pa, va, vb, bA, bB, st):
    """Bound + gradients for rows R.  st: dict phA, phB, alA, alB, beA, beB (lists per layer), t."""
    ws, bs = net
    t = st["t"]
    cA, kA, rA = backward(ws, bs, bA[0], bA[1], st["phA"], st["alA"], st["beA"], t)
    cB, kB, rB = backward(ws, bs, bB[0], bB[1], st["phB"], st["alB"], st["beB"], -(1 - t))
    kA = kA + (cA[:, pa] * va[None]).sum(1)
    kB = kB + (cB[:, pa] * vb[None]).sum(1)
    coef = cA + cB
    coef[:, pa] = 0
    xs = torch.where(coef >= 0, lo, hi)
    B = (coef * xs).sum(1) + kA + kB
    xa, xb = xs.clone(), xs.clone()
    xa[:, pa] = va[None]
    xb[:, pa] = vb[None]
    zA, oA = forward_lin(ws, bs, xa, bA[0], rA, st["alA"])
    zB, oB = forward_lin(ws, bs, xb, bB[0], rB, st["alB"])
    g = {"t": oA + oB}
    for nm, z, rec, ph in (("A", zA, rA, st["phA"]), ("B", zB, rB, st["phB"])):
        g["al" + nm] = [torch.where(r[2] == 2, r[0] * zz, torch.zeros_like(zz)) for zz, r in zip(z, rec)]
        g["be" + nm] = [-p.to(zz.dtype) * zz for zz, p in zip(z, ph)]
    return B, g, (zA, rA), (zB, rB)


def branch_scores(bnd, lin, ph):
    """|lam_h| x relaxation gap at x* for unstable unfixed neurons (the bound the split recovers)."""
    LB, UB = bnd
    z, rec = lin
    out = []
    for l in range(len(z)):
        lam, mu, kind, s = rec[l]
        zz = z[l]
        gap = torch.where(kind == 2, torch.relu(zz) - mu / torch.where(lam == 0, torch.ones_like(lam), lam) * zz,
                          torch.where(kind == 3, s * (zz - LB[l]) - torch.relu(zz), torch.zeros_like(zz)))
        out.append(torch.where((kind >= 2) & (ph[l] == 0), lam.abs() * gap.abs(), torch.zeros_like(zz)))
    return torch.cat(out, 1)


def _intercepts(bnd, lin, ph):
    LB, UB = bnd
    z, rec = lin
    out = []
    for l in range(len(z)):
        lam, mu, kind, s = rec[l]
        out.append(torch.where((kind >= 2) & (ph[l] == 0), (lam * s * LB[l]).abs() + 1e-30, torch.zeros_like(lam)))
    return torch.cat(out, 1)


def clamp_bounds(LB, UB, ph):
    lbs = [torch.where(p > 0, lb.clamp(min=0), lb) for lb, p in zip(LB, ph)]
    ubs = [torch.where(p < 0, ub.clamp(max=0), ub) for ub, p in zip(UB, ph)]
    infeas = torch.zeros(ph[0].shape[0], dtype=torch.bool)
    for lb, ub in zip(lbs, ubs):
        infeas |= (lb > ub).any(1)
    return lbs, ubs, infeas


def split_layers(v, widths):
    out, o = [], 0
    for w in widths:
        out.append(v[:, o:o + w])
        o += w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="src/AC-sex")
    ap.add_argument("--model", default="AC-7")
    ap.add_argument("--weights", default="zoo")
    ap.add_argument("--pids", default="12596,4387,6769,6543,4330")
    ap.add_argument("--budget", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--root-iters", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--lrb", type=float, default=0.05)
    ap.add_argument("--check-grad", action="store_true")
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    from fairify_amd import presets
    from fairify_amd.engine.search import pa_table
    from fairify_amd.models.zoo import get_model
    from fairify_amd.ops.backend import Backend
    from fairify_amd.smt import milp

    torch.set_num_threads(8)
    pre = presets.get(a.preset)
    grid, q = pre.grid(), pre.resolved()
    m = get_model(a.model, weights=a.weights, seed=0)
    be_ = Backend(m, "cpu")
    ws = [torch.tensor(np.asarray(w), dtype=torch.float64) for w in m.weights]
    bs = [torch.tensor(np.asarray(b), dtype=torch.float64).reshape(-1) for b in m.biases]
    widths = [w.shape[1] for w in ws[:-1]]
    pa = list(q.pa_idx)
    ids = np.array([int(x) for x in a.pids.split(",")])
    lo_all, hi_all = grid.decode(ids)
    vals, pairs = pa_table(q, lo_all, hi_all)
    lbs, ubs = milp.layer_bounds_rows(be_, lo_all, hi_all, q, vals, widen_ra=False)
    for k, pid in enumerate(ids):
        t0 = time.time()
        verdict, per = "unsat", []
        for vi, vj in pairs:
            va = torch.tensor(vals[int(vi)], dtype=torch.float64)
            vb = torch.tensor(vals[int(vj)], dtype=torch.float64)
            rootA = [torch.tensor(lb[k, int(vi)], dtype=torch.float64) for lb in lbs], \
                [torch.tensor(ub[k, int(vi)], dtype=torch.float64) for ub in ubs]
            rootB = [torch.tensor(lb[k, int(vj)], dtype=torch.float64) for lb in lbs], \
                [torch.tensor(ub[k, int(vj)], dtype=torch.float64) for ub in ubs]
            lo = torch.tensor(lo_all[k], dtype=torch.float64)[None]
            hi = torch.tensor(hi_all[k], dtype=torch.float64)[None]
            z = lambda: [torch.zeros(1, w, dtype=torch.float64) for w in widths]  # noqa: E731
            st = {"phA": [torch.zeros(1, w, dtype=torch.int8) for w in widths],
                  "phB": [torch.zeros(1, w, dtype=torch.int8) for w in widths],
                  "alA": [torch.full((1, w), 0.5, dtype=torch.float64) for w in widths],
                  "alB": [torch.full((1, w), 0.5, dtype=torch.float64) for w in widths],
                  "beA": z(), "beB": z(), "t": torch.full((1,), 0.5, dtype=torch.float64)}
            nodes, depth, status = 0, 0, "unsat"
            n_in = [0]
            while lo.shape[0]:
                R = lo.shape[0]
                nodes += R
                if nodes > a.budget:
                    status = "unknown"
                    break
                bA = clamp_bounds([x.expand(R, -1) for x in rootA[0]],
                                  [x.expand(R, -1) for x in rootA[1]], st["phA"])
                bB = clamp_bounds([x.expand(R, -1) for x in rootB[0]], [x.expand(R, -1) for x in rootB[1]], st["phB"])
                feas = ~(bA[2] | bB[2])
                keys = ["alA", "alB", "beA", "beB"]
                mom = {kk: [torch.zeros_like(x) for x in st[kk]] for kk in keys}
                vel = {kk: [torch.zeros_like(x) for x in st[kk]] for kk in keys}
                mt = torch.zeros_like(st["t"])
                vt = torch.zeros_like(st["t"])
                best = torch.full((R,), -np.inf, dtype=torch.float64)
                iters = a.root_iters if depth == 0 else a.iters
                lin = None
                for it in range(iters + 1):
                    B, g, linA, linB = pair_bound((ws, bs), lo, hi, pa, va, vb, bA[:2], bB[:2], st)
                    if a.check_grad and it == 3 and depth == 0:
                        _check_grad((ws, bs), lo, hi, pa, va, vb, bA, bB, st, g)
                    imp = B > best
                    best = torch.maximum(best, B)
                    if lin is None:
                        lin = (linA, linB, B.clone())
                    else:   # keep the linearisation of the best iterate for branching
                        lin = (linA, linB, B) if bool(imp.all()) else lin
                    if it == iters or bool(((best >= 0) | ~feas).all()):
                        break
                    b1, b2, eps = 0.9, 0.999, 1e-8
                    for kk in keys:
                        lr = a.lr if kk.startswith("al") else a.lrb
                        for i in range(len(widths)):
                            gg = g[kk][i]
                            mom[kk][i] = b1 * mom[kk][i] + (1 - b1) * gg
                            vel[kk][i] = b2 * vel[kk][i] + (1 - b2) * gg * gg
                            mh = mom[kk][i] / (1 - b1 ** (it + 1))
                            vh = vel[kk][i] / (1 - b2 ** (it + 1))
                            x = st[kk][i] + lr * mh / (vh.sqrt() + eps)
                            st[kk][i] = x.clamp(0, 1) if kk.startswith("al") else x.clamp(min=0)
                    mt = b1 * mt + (1 - b1) * g["t"]
                    vt = b2 * vt + (1 - b2) * g["t"] ** 2
                    st["t"] = (st["t"] + a.lr * (mt / (1 - b1 ** (it + 1))) /
                               ((vt / (1 - b2 ** (it + 1))).sqrt() + 1e-8)).clamp(0, 1)
                closed = (best >= 0) | ~feas
                if os.environ.get("BDBG"): print("lvl", R, float(best.min()), float(best.max()), int(closed.sum()))
                if a.verify:
                    _verify(ws, bs, lo, hi, pa, va, vb, st, B, bA, bB)
                depth += 1
                keep = torch.nonzero(~closed)[:, 0]
                if keep.numel() == 0:
                    break
                linA, linB, _ = lin
                sc = torch.cat([branch_scores(bA[:2], linA, st["phA"]), branch_scores(bB[:2], linB, st["phB"])], 1)
                sc = sc[keep]
                mx, j = sc.max(1)
                # fallback: an unstable unfixed neuron by chord intercept; none left -> input split
                fb_sc = torch.cat([_intercepts(bA[:2], linA, st["phA"]), _intercepts(bB[:2], linB, st["phB"])], 1)[keep]
                mx2, j2 = fb_sc.max(1)
                j = torch.where(mx > 0, j, j2)
                neuron = (mx > 0)
                NH = sum(widths)
                new = {kk: [] for kk in ("lo", "hi", "phA", "phB", "alA", "alB", "beA", "beB", "t")}
                fa = torch.cat(st["phA"], 1)
                fb = torch.cat(st["phB"], 1)
                cat = {kk: torch.cat(st[kk], 1) for kk in ("alA", "alB", "beA", "beB")}
                for r_i in range(keep.numel()):
                    r = int(keep[r_i])
                    kids = []
                    if bool(neuron[r_i]):
                        jj = int(j[r_i])
                        for sg in (-1, 1):
                            a2, b2 = fa[r].clone(), fb[r].clone()
                            if jj < NH:
                                a2[jj] = sg
                            else:
                                b2[jj - NH] = sg
                            kids.append((lo[r], hi[r], a2, b2))
                    else:
                        w = hi[r] - lo[r]
                        w[pa] = -1
                        d = int(torch.argmax(w))
                        if w[d] <= 0:
                            status = "leaf"       # single lattice point: exact check
                            continue
                        mid = torch.floor((lo[r, d] + hi[r, d]) / 2)
                        for a_, b_ in ((lo[r, d], mid), (mid + 1, hi[r, d])):
                            l2, h2 = lo[r].clone(), hi[r].clone()
                            l2[d], h2[d] = a_, b_
                            kids.append((l2, h2, fa[r], fb[r]))
                        n_in[0] += 1
                    for l2, h2, a2, b2 in kids:
                        new["lo"].append(l2); new["hi"].append(h2); new["phA"].append(a2); new["phB"].append(b2)
                        for kk in ("alA", "alB", "beA", "beB"):
                            new[kk].append(cat[kk][r])
                        new["t"].append(st["t"][r])
                if status == "leaf" or not new["lo"]:
                    break
                lo, hi = torch.stack(new["lo"]), torch.stack(new["hi"])
                for kk in ("phA", "phB", "alA", "alB", "beA", "beB"):
                    st[kk] = split_layers(torch.stack(new[kk]), widths)
                st["t"] = torch.stack(new["t"])
            per.append((status, nodes, depth, n_in[0]))
            if status != "unsat":
                verdict = status
                break
        print(json.dumps({"pid": int(pid), "verdict": verdict, "pairs": per, "s": round(time.time() - t0, 2)}),
              flush=True)


def _verify(ws, bs, lo, hi, pa, va, vb, st, B, bA, bB, n=4000):
    """Soundness spot check: on random lattice points of each node's box that satisfy its phase
    constraints, t N(x, va) - (1 - t) N(x, vb) >= the node's bound at the current parameters."""
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for r in range(lo.shape[0]):
        x = lo[r][None] + torch.floor(torch.rand(n, lo.shape[1], generator=g, dtype=torch.float64) *
                                      (hi[r] - lo[r] + 1)[None])
        ok = torch.ones(n, dtype=torch.bool)
        outs = []
        for v, ph in ((va, st["phA"]), (vb, st["phB"])):
            h = x.clone()
            h[:, pa] = v[None]
            for l in range(len(ws) - 1):
                z = h @ ws[l] + bs[l][None]
                p = ph[l][r].to(torch.float64)
                ok &= ((p[None] * z) >= 0).all(1)
                h = torch.relu(z)
            outs.append((h @ ws[-1] + bs[-1][None])[:, 0])
        t = st["t"][r]
        f = t * outs[0] - (1 - t) * outs[1]
        if ok.any():
            gap = float((f[ok].min() - B[r]).item())
            worst = min(worst, gap)
            if gap < -1e-9 * (1 + abs(float(B[r]))):
                print("UNSOUND node", r, "bound", float(B[r]), "min f", float(f[ok].min()))
    return worst


def _check_grad(net, lo, hi, pa, va, vb, bA, bB, st, g):
    """Finite-difference check of the analytic gradient (first row, a few coordinates)."""
    h = 1e-6
    for kk in ("alA", "beB"):
        for l in range(len(st[kk])):
            for j in range(min(3, st[kk][l].shape[1])):
                old = st[kk][l][0, j].item()
                st[kk][l][0, j] = old + h
                Bp = pair_bound(net, lo, hi, pa, va, vb, bA[:2], bB[:2], st)[0][0].item()
                st[kk][l][0, j] = old - h
                Bm = pair_bound(net, lo, hi, pa, va, vb, bA[:2], bB[:2], st)[0][0].item()
                st[kk][l][0, j] = old
                fd = (Bp - Bm) / (2 * h)
                an = g[kk][l][0, j].item()
                if abs(fd - an) > 1e-5 * (1 + abs(fd)):
                    print("grad mismatch", kk, l, j, fd, an)
    print("grad check done")


if __name__ == "__main__":
    main()
