#!/usr/bin/env python
"""A fixed list of small cases through the three BaB front ends (``BaBSolver``, ``ReluBaBSolver``,
``BetaBaBSolver``), with everything a caller can see of each solve saved to one ``.npz``.

The dump of one commit against the dump of another, on the same machine and device, is the check
that a change of the solvers' host code moved no verdict, witness or node count.  Only
``XSolver(be, q, cfg).solve(...)`` is called, so the same file runs on any commit.  Per case the
``.npz`` holds ``status``, ``cex_x``, ``cex_xp``, ``nodes``, ``iters``, ``open_left`` (no key where
the result has none) and the integer entries of ``solver.stats``.  No case sets ``time_budget``: the
wall clock decides nothing.

The cases: the 5-feature toy domain with ``random_mlp(5, [6, 4])`` (PA-only, two PAs, relaxed with
tau 1 to 3, two PA groups, a single-PA-value box, ``init_status``, ``dead`` / ``exact_models``, small
``node_budget`` and ``max_pool``), ``random_mlp(13, [8, 6, 4])`` on 24 narrowed ``src/AC-sex``
partitions (beta: every branching rule and switch of the torch loop), AC-8 / AC-12 random weights on
32 narrowed partitions (relu).  On a HIP device the native runtimes decide by default;
``FAIRIFY_TORCH_BAB=1 FAIRIFY_TORCH_BETA=1`` runs the torch loops there.

    python tools/dump_solvers.py OUT.npz [--device cuda]     # record
    python tools/dump_solvers.py --compare A.npz B.npz        # every differing key, exit 1 if any
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fairify_amd import presets  # noqa: E402
from fairify_amd.engine.bab import RUNNING, SAT, UNKNOWN, UNSAT, BaBConfig, BaBSolver  # noqa: E402
from fairify_amd.engine.beta_bab import BetaBaBSolver, BetaConfig  # noqa: E402
from fairify_amd.engine.relu_bab import ReluBaBSolver, ReluConfig  # noqa: E402
from fairify_amd.models.mlp import random_mlp  # noqa: E402
from fairify_amd.models.zoo import get_model  # noqa: E402
from fairify_amd.ops.backend import Backend  # noqa: E402
from fairify_amd.partition import processing_order  # noqa: E402
from fairify_amd.spec import ADULT, Domain, Feature, Query  # noqa: E402

TOY_HI = np.array([3, 4, 2, 4, 5])
TOY = Domain("toy", tuple(Feature(f"f{i}", 0, int(w)) for i, w in enumerate(TOY_HI)))


def toy_boxes(pa_ranges=((0, 2),), f0=None):
    """Partitions of the toy domain: f4 halved, one pair of halves per range of the PA f2 (several
    ranges: several PA groups, interleaved so a group's rows are not contiguous); ``f0``: its range."""
    lo, hi = [], []
    for a, b in ((0, 2), (3, 5)):
        for pl, ph in pa_ranges:
            l, h = np.zeros(5, np.int64), TOY_HI.astype(np.int64).copy()
            l[4], h[4], l[2], h[2] = a, b, pl, ph
            if f0 is not None:
                l[0], h[0] = f0
            lo.append(l)
            hi.append(h)
    return np.array(lo), np.array(hi)


def ac_boxes(count, preset="src/AC-sex"):
    grid = presets.get(preset).grid()
    lo, hi = grid.decode(processing_order(grid, 0)[:count])
    return lo, np.minimum(hi, lo + 1)


def toy_q(pa=("f2",), ra=(), tau=0):
    return Query(pa=pa, ra=ra, tau=tau).resolve(TOY)


def dead_and_models(m, P, seed):
    """Seeded per-partition forced-dead masks [P, N_hidden] and the masked exact networks."""
    g = np.random.default_rng(seed)
    hidden = [w.shape[1] for w in m.weights[:-1]]
    dead = g.random((P, sum(hidden))) < 0.2
    cuts = np.cumsum(hidden)[:-1]
    return dead, [m.masked(np.split(dead[p], cuts)) for p in range(P)]


def cases():
    """(name, solver class, mlp, query, config, lo, hi, keyword arguments of solve, dead mask)."""
    out = []
    mixed = ((0, 2), (0, 1), (1, 2))
    big = 10 ** 6
    # ---- input-split BaB on the toy domain
    for seed in (300, 301, 304, 307):
        m = random_mlp(5, [6, 4], seed=seed, bias_scale=1.0 if seed % 3 else 0.0)
        for tag, q in (("pa", toy_q()), ("two_pa", toy_q(("f2", "f0"))), ("rx1", toy_q(ra=("f3",), tau=1)),
                       ("rx2", toy_q(ra=("f1", "f4"), tau=2))):
            lo, hi = toy_boxes()
            out.append((f"bab.{tag}.{seed}", BaBSolver, m, q, BaBConfig(node_budget=big), lo, hi, {}, None))
        lo, hi = toy_boxes(mixed)
        out.append((f"bab.groups.{seed}", BaBSolver, m, toy_q(), BaBConfig(node_budget=big), lo, hi, {}, None))
        out.append((f"bab.groups_rx.{seed}", BaBSolver, m, toy_q(ra=("f3",), tau=3), BaBConfig(node_budget=big),
                    lo, hi, {}, None))
        init = np.array([RUNNING, SAT, UNSAT, UNKNOWN, RUNNING, RUNNING], np.int8)
        out.append((f"bab.init.{seed}", BaBSolver, m, toy_q(), BaBConfig(node_budget=big), lo, hi,
                    {"init_status": init}, None))
        dead, models = dead_and_models(m, len(lo), seed)
        out.append((f"bab.dead.{seed}", BaBSolver, m, toy_q(), BaBConfig(node_budget=big), lo, hi,
                    {"exact_models": models}, dead))
        out.append((f"bab.dead_rx.{seed}", BaBSolver, m, toy_q(ra=("f3",), tau=1), BaBConfig(node_budget=big),
                    lo, hi, {"exact_models": models}, dead))
        lo, hi = toy_boxes(((1, 1),))
        out.append((f"bab.single_pa.{seed}", BaBSolver, m, toy_q(), BaBConfig(), lo, hi, {}, None))
    for seed in (400, 401, 403):
        m = random_mlp(5, [8, 8], seed=seed, bias_scale=0.5)
        lo, hi = toy_boxes(mixed)
        for tag, q in (("pa", toy_q()), ("rx", toy_q(ra=("f1", "f4"), tau=2))):
            out.append((f"bab.budget_{tag}.{seed}", BaBSolver, m, q, BaBConfig(node_budget=2), lo, hi, {}, None))
            out.append((f"bab.max_pool_{tag}.{seed}", BaBSolver, m, q, BaBConfig(node_budget=big, max_pool=3),
                        lo, hi, {}, None))
    # ---- ReLU-phase BaB: the toy domain, then AC-8 / AC-12 and a relaxed query on src/AC-sex boxes
    for seed in (300, 304, 401):
        m = random_mlp(5, [6, 4], seed=seed, bias_scale=1.0 if seed % 3 else 0.0)
        lo, hi = toy_boxes(mixed)
        init = np.array([RUNNING, SAT, UNSAT, UNKNOWN, RUNNING, RUNNING], np.int8)
        for tag, q, cfg, kw in (
                ("groups", toy_q(), ReluConfig(node_budget=4096), {}),
                ("two_pa", toy_q(("f2", "f0")), ReluConfig(node_budget=4096), {}),
                ("init", toy_q(), ReluConfig(node_budget=4096), {"init_status": init}),
                ("rx1", toy_q(ra=("f3",), tau=1), ReluConfig(node_budget=4096), {}),
                ("rx2_nomerge", toy_q(ra=("f1", "f4"), tau=2), ReluConfig(node_budget=4096, merge_orient=False), {}),
                ("rx3_init", toy_q(ra=("f3",), tau=3), ReluConfig(node_budget=4096), {"init_status": init}),
                ("budget", toy_q(), ReluConfig(node_budget=3), {}),
                ("budget_rx", toy_q(ra=("f3",), tau=1), ReluConfig(node_budget=3), {}),
                ("max_pool", toy_q(), ReluConfig(node_budget=4096, max_pool=4), {}),
                ("max_pool_rx", toy_q(ra=("f3",), tau=1), ReluConfig(node_budget=4096, max_pool=4,
                                                                   merge_orient=False), {})):
            out.append((f"relu.{tag}.{seed}", ReluBaBSolver, m, q, cfg, lo, hi, kw, None))
        lo, hi = toy_boxes(((2, 2),))
        out.append((f"relu.single_pa.{seed}", ReluBaBSolver, m, toy_q(), ReluConfig(), lo, hi, {}, None))
    q_sex = presets.get("src/AC-sex").resolved()
    lo, hi = ac_boxes(32)
    for name in ("AC-8", "AC-12"):
        m = get_model(name, weights="random", seed=1)
        out.append((f"relu.{name}", ReluBaBSolver, m, q_sex, ReluConfig(node_budget=4096), lo, hi, {}, None))
        out.append((f"relu.{name}.budget", ReluBaBSolver, m, q_sex, ReluConfig(node_budget=4), lo, hi, {}, None))
        out.append((f"relu.{name}.max_pool", ReluBaBSolver, m, q_sex, ReluConfig(node_budget=4096, max_pool=8),
                    lo, hi, {}, None))
    q_age = Query(pa=("sex",), ra=("age",), tau=2).resolve(ADULT)
    lo, hi = ac_boxes(12)
    for merge in (True, False):
        out.append((f"relu.age2.merge{int(merge)}", ReluBaBSolver, random_mlp(13, [6, 6], seed=21, bias_scale=0.0),
                    q_age, ReluConfig(node_budget=8192, merge_orient=merge), lo, hi, {}, None))
    # ---- beta-CROWN BaB: random_mlp(13, [8, 6, 4]) on narrowed src/AC-sex boxes, then the toy domain
    lo, hi = ac_boxes(24)
    base = dict(node_budget=256, iters=20, root_iters=40)
    m3 = random_mlp(13, [8, 6, 4], seed=3, bias_scale=0.5)
    for tag, kw in (("kernel", dict(branch="kernel")), ("pgap", dict(branch="pgap")), ("lpgap", dict(branch="lpgap")),
                    ("input2", dict(branch="kernel", input_every=2)), ("noprune", dict(sign_prune=False)),
                    ("notighten", dict(tighten=False)), ("trees", dict(trees=((0, 1),))),
                    ("budget", dict(node_budget=3)), ("max_pool", dict(max_pool=6))):
        out.append((f"beta.{tag}", BetaBaBSolver, m3, q_sex, BetaConfig(**{**base, **kw}), lo, hi, {}, None))
    m5 = random_mlp(13, [24, 12, 6], seed=5, bias_scale=0.5)
    lo12, hi12 = presets.get("src/AC-sex").grid().decode(processing_order(presets.get("src/AC-sex").grid(), 0)[:8])
    out.append(("beta.probe", BetaBaBSolver, m5, q_sex, BetaConfig(node_budget=48, iters=10, root_iters=20,
                                                                    probe_levels=1), lo12, hi12, {}, None))
    lo, hi = ac_boxes(12)
    m21 = random_mlp(13, [8, 6, 4], seed=21, bias_scale=0.5)
    for merge in (True, False):
        out.append((f"beta.age2.merge{int(merge)}", BetaBaBSolver, m21, q_age,
                    BetaConfig(node_budget=512, iters=20, root_iters=40, merge_orient=merge), lo, hi, {}, None))
    m = random_mlp(5, [6, 4], seed=304, bias_scale=1.0)
    lo, hi = toy_boxes(mixed)
    init = np.array([RUNNING, SAT, UNSAT, UNKNOWN, RUNNING, RUNNING], np.int8)
    for tag, q, kw in (("groups", toy_q(), {}), ("init", toy_q(), {"init_status": init}),
                       ("rx1", toy_q(ra=("f3",), tau=1), {}),
                       ("rx3_init", toy_q(ra=("f3",), tau=3), {"init_status": init})):
        out.append((f"beta.toy_{tag}", BetaBaBSolver, m, q, BetaConfig(**base), lo, hi, kw, None))
    out.append(("beta.toy_rx2_nomerge", BetaBaBSolver, m, toy_q(ra=("f1", "f4"), tau=2),
                BetaConfig(merge_orient=False, **base), lo, hi, {}, None))
    out.append(("beta.toy_rx1_max_pool", BetaBaBSolver, m, toy_q(ra=("f3",), tau=1), BetaConfig(max_pool=6, **base),
                lo, hi, {}, None))
    out.append(("beta.toy_rx2_nomerge_max_pool", BetaBaBSolver, m, toy_q(ra=("f1", "f4"), tau=2),
                BetaConfig(merge_orient=False, max_pool=6, **base), lo, hi, {}, None))
    for tag, kw in (("kernel", dict(branch="kernel")), ("lpgap", dict(branch="lpgap")),
                    ("input2", dict(input_every=2)), ("notighten", dict(tighten=False)),
                    ("probe", dict(probe_levels=1)), ("budget", dict(node_budget=3))):
        out.append((f"beta.toy_rx1_{tag}", BetaBaBSolver, m, toy_q(ra=("f3",), tau=1), BetaConfig(**{**base, **kw}),
                    lo, hi, {}, None))
    lo, hi = toy_boxes(((0, 1),), f0=(1, 2))
    out.append(("beta.toy_two_pa", BetaBaBSolver, random_mlp(5, [6, 4], seed=301, bias_scale=1.0),
                toy_q(("f0", "f2")), BetaConfig(**base), lo, hi, {}, None))   # (native runtime: increasing PA dims)
    lo, hi = toy_boxes(((0, 0),))
    out.append(("beta.toy_single_pa", BetaBaBSolver, m, toy_q(), BetaConfig(**base), lo, hi, {}, None))
    return out


def dump(dev, only=None):
    """name/key -> numpy array of every case, in case order."""
    arrays, backends = {}, {}
    for name, cls, m, q, cfg, lo, hi, kw, dead in cases():
        if only and not any(name.startswith(p) for p in only):
            continue
        be = backends.setdefault(id(m), Backend(m, device=dev))
        t0 = time.time()
        if cls is BaBSolver:
            solver = cls(be, q, cfg, dead=None if dead is None else torch.from_numpy(dead).to(be.device))
        else:
            solver = cls(be, q, cfg)
        res = solver.solve(lo, hi, m, **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        for k in ("status", "cex_x", "cex_xp", "nodes"):
            arrays[f"{name}/{k}"] = np.asarray(getattr(res, k))
        arrays[f"{name}/iters"] = np.asarray(int(res.iters))
        if res.open_left is not None:
            arrays[f"{name}/open_left"] = np.asarray(res.open_left)
        for k, v in sorted(getattr(solver, "stats", {}).items()):
            if isinstance(v, (bool, int, np.integer)):
                arrays[f"{name}/stats.{k}"] = np.asarray(int(v))
        st = arrays[f"{name}/status"]
        print(f"{name:28s} sat {int((st == SAT).sum()):2d} unsat {int((st == UNSAT).sum()):2d} "
              f"unknown {int((st == UNKNOWN).sum()):2d} nodes {int(res.nodes.sum()):6d} {time.time() - t0:6.2f} s",
              flush=True)
    return arrays


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in a.files:
        if k in b.files and not (a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])):
            bad.append(k)
    for k in bad:
        print("differs:", k)
    print(f"{a_path} against {b_path}: {len(set(a.files) | set(b.files)) - len(bad)} keys equal, {len(bad)} differ")
    return bad


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--only", nargs="*", default=None, help="case name prefixes")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(*a.compare) else 0)
    dev = torch.device("cuda:0" if a.device == "cuda" else a.device)
    arrays = dump(dev, a.only)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"{len(arrays)} arrays -> {a.out}")


if __name__ == "__main__":
    main()
