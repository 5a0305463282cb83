#!/usr/bin/env python
"""Every wrapper of ``fairify_amd.ops.hip`` that fills an ``args.h`` struct, called once on the
smallest shapes that reach it, with every array it returns or updates in place saved to one ``.npz``.

The dump of one build against the dump of another is the check that a change of the Python/C++
boundary moved no pointer and no scalar: every array must be equal bit for bit
(``tests/test_boundary_gpu.py`` compares against ``tests/golden/boundary_parent.npz``).  Inputs are
drawn on the CPU from fixed seeds: the net ``random_mlp(13, [8, 6, 4])``, R = 5 rows, P = 3
partitions, 128 samples.  While the wrappers run, ``torch.empty`` buffers are filled (NaN / the
largest integer, torch's deterministic mode), so rows a kernel leaves unwritten compare equal too;
``unwritten(arrays)`` names the float arrays that hold such rows.

    python tools/dump_boundary.py OUT.npz             # record
    python tools/dump_boundary.py OUT.npz --against tests/golden/boundary_parent.npz
"""
import contextlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fairify_amd.models.mlp import random_mlp  # noqa: E402
from fairify_amd.ops import hip  # noqa: E402
from fairify_amd.ops.backend import Backend  # noqa: E402
from fairify_amd.partition import Grid  # noqa: E402
from fairify_amd.spec import ADULT, Query  # noqa: E402

R, P, S = 5, 3, 128
LR = dict(lr_a=0.1, lr_b=0.5, lr_t=0.1)


@contextlib.contextmanager
def filled_empty():
    """``torch.empty`` returns filled memory inside the block (the state before is restored)."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
        torch.utils.deterministic.fill_uninitialized_memory = fill


def _boxes(seed, rows=R, n0=13):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(0, 6, (rows, n0), generator=g).float()
    hi = lo + torch.randint(0, 3, (rows, n0), generator=g).float()
    return lo, hi


def _points(lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return lo + torch.floor(torch.rand(lo.shape, generator=g) * (hi - lo + 1)).clamp(max=hi - lo)


def _phase_at(m, x, seed, fix=0.3):
    """int8 [R, NH]: a seeded ``fix`` share of the neurons fixed to the phase they take at ``x``."""
    h, zs = x.double().numpy(), []
    for W, b in list(zip(m.weights, m.biases))[:-1]:
        z = h @ np.asarray(W, np.float64) + np.asarray(b, np.float64).reshape(-1)
        zs.append(z)
        h = np.maximum(z, 0)
    z = torch.from_numpy(np.concatenate(zs, 1))
    pick = torch.rand(z.shape, generator=torch.Generator().manual_seed(seed)) < fix
    return torch.where(pick, torch.where(z >= 0, 1, -1), 0).to(torch.int8)


def _res(out, name, res):
    for k in ("out_lb", "out_ub", "Lc", "L0", "Le", "Uc", "U0", "Ue", "lay_lb_full", "lay_ub_full", "dead_u8",
              "infeasible"):
        v = getattr(res, k, None)
        if v is not None:
            out[f"{name}.{k}"] = v


def bound_family(out, m, be, dev):
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    lo, hi = _boxes(7)
    L, H = d(lo), d(hi)
    ph = _phase_at(m, _points(lo, hi, 8), 9)
    g = torch.Generator().manual_seed(10)
    dead = d((torch.rand(R, be.n_hidden, generator=g) < 0.2).to(torch.uint8))
    _res(out, "bounds.sym", hip.bounds(be, L, H))
    _res(out, "bounds.sym_dead", hip.bounds(be, L, H, dead=dead))
    _res(out, "bounds.sym_phase", hip.bounds(be, L, H, keep_layers=True, phase=d(ph)))
    _res(out, "bounds.interval", hip.bounds(be, L, H, mode="interval"))
    _res(out, "bounds.keep_layers", hip.bounds(be, L, H, keep_layers=True))
    flo, fhi = lo.clone(), hi.clone()
    flo[:, 4] = fhi[:, 4] = 2
    flo[:, 11] = fhi[:, 11] = 1
    _res(out, "bounds.fold", hip.bounds(be, d(flo), d(fhi), fold=(4, 11)))
    _res(out, "crown", hip.crown(be, L, H, hip.bounds(be, L, H, keep_layers=True)))
    _res(out, "crown.dead", hip.crown(be, L, H, hip.bounds(be, L, H, dead=dead, keep_layers=True), dead=dead))
    _res(out, "refine", hip.refine(be, L, H, hip.bounds(be, L, H, keep_layers=True)))
    _res(out, "refine.phase", hip.refine(be, L, H, hip.bounds(be, L, H, keep_layers=True, phase=d(ph)),
                                         phase=d(ph)))
    bb = hip.backward_bounds(be, L, H)
    assert bb is not None
    _res(out, "backward_bounds", bb)
    _res(out, "backward_bounds.nolayers", hip.backward_bounds(be, L, H, dead=dead, keep_layers=False))
    res = hip.bounds(be, L, H, keep_layers=True, phase=d(ph))
    pc, _ = hip.crown_phase(be, L, H, res, d(ph))
    _res(out, "crown_phase.res", res)
    out["crown_phase.low"], out["crown_phase.split"], out["crown_phase.score"] = pc.low, pc.split, pc.score
    x = d(_points(lo, hi, 11))
    out["point_bounds.lb"], out["point_bounds.ub"] = hip.point_bounds(be, x)
    out["point_bounds.dead.lb"], out["point_bounds.dead.ub"] = hip.point_bounds(be, x, dead=dead)
    # pair certificate of R nodes, relaxed (input 0 is the RA dim, PA dim 8 with values 0 / 1)
    values = torch.tensor([[0], [1]])
    pairs = torch.tensor([[0, 1], [1, 0]])
    lo[:, 8], hi[:, 8] = 0, 1
    plo, phi = lo.clone(), hi.clone()
    plo[:, 0] -= 2
    phi[:, 0] += 2
    shared = torch.ones(13, dtype=torch.bool)
    shared[0] = False

    def rows(a, b):
        ra, rb = a[:, None, :].repeat(1, 2, 1), b[:, None, :].repeat(1, 2, 1)
        ra[:, :, 8] = rb[:, :, 8] = values[:, 0].float()
        return d(ra.reshape(-1, 13)), d(rb.reshape(-1, 13))

    rx, rxp = hip.bounds(be, *rows(lo, hi)), hip.bounds(be, *rows(plo, phi))
    for relaxed in (False, True):
        dec = hip.pair_certify(be, rx, rxp, d(lo), d(hi), d(plo), d(phi), d(pairs), d(values), torch.tensor([8]),
                               d(shared), relaxed)
        for k in ("open_", "score", "split_dim", "cand_x", "cand_xp", "cand_v", "cand_orient"):
            out[f"pair_certify.{int(relaxed)}.{k}"] = getattr(dec, k)


def sampling_family(out, m, be, dev):
    grid = Grid.reference(ADULT, 10)
    ids = np.arange(0, 16000, 401)[:P]
    lo_np, hi_np = grid.decode(ids)
    lo, hi = torch.from_numpy(lo_np).float().to(dev), torch.from_numpy(hi_np).float().to(dev)
    pids = torch.from_numpy(ids).to(dev)
    for kind, q in (("pa", Query(("race",)).resolve(ADULT)), ("relaxed", Query(("sex",), ("age",), 2).resolve(ADULT))):
        v_np = q.pa_values(lo_np[0], hi_np[0])
        values, pairs = torch.from_numpy(v_np).to(dev), torch.from_numpy(q.pa_pairs(v_np)).to(dev)
        for split, blocks in ((1, 0), (2, 2048)):
            was = hip._SIM_BLOCKS, hip._SIM_BLOCKS_ENV
            hip._SIM_BLOCKS, hip._SIM_BLOCKS_ENV = blocks, None      # workgroups per partition list, not the env's
            try:
                assert hip._sim_split(P, S) == split
                sim = hip.simulate(be, q, lo, hi, pids, S, 9, values, pairs, 0, 0, return_z0=True)
            finally:
                hip._SIM_BLOCKS, hip._SIM_BLOCKS_ENV = was
            for k in ("counts", "found", "wit_x", "wit_xp", "z0"):
                out[f"simulate.{kind}.split{split}.{k}"] = getattr(sim, k)
        for split in (1, 2):
            f, a, idx = hip.rate_counts(be, q, lo, hi, pids, S, 5, values, pairs, split=split)
            out[f"rate.{kind}.{split}.flips"], out[f"rate.{kind}.{split}.amb"], out[f"rate.{kind}.{split}.idx"] = f, a, idx
        free = [k for k in range(13) if k not in set(q.pa_idx)]
        fo = hip.falsify(be, q, lo, hi, pids, values, pairs, 3, S, 64, 4, 6, 4, 6, free, dseed=17)
        assert fo is not None
        for k, v in zip(("found", "wit_x", "wit_xp", "how"), fo):
            out[f"falsify.{kind}.{k}"] = v
        if kind == "pa":
            K = 4
            lo3, hi3 = lo.cpu()[:, None, :].repeat(1, K, 1), hi.cpu()[:, None, :].repeat(1, K, 1)
            x0 = _points(lo3, hi3, 12).to(dev)
            f0 = torch.full((P, K), -1e30, device=dev)
            q0 = torch.zeros(P, K, dtype=torch.int32, device=dev)
            ao = hip.ascent(be, q, lo, hi, x0, f0, q0, 6, values, pairs, free)
            assert ao is not None
            for k, v in zip(("found", "wit_x", "wit_xp"), ao):
                out[f"ascent.{k}"] = v


def beta_family(out, m, be, dev):
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    NH, pa = be.n_hidden, [1]
    lo, hi = _boxes(21)
    lo[:, pa], hi[:, pa] = 0, 1
    x = _points(lo, hi, 22)
    va, vb = torch.zeros(R, 1), torch.ones(R, 1)
    ram = torch.zeros(13, dtype=torch.bool)
    ram[2] = True
    plo, phi = lo.clone(), hi.clone()
    plo[:, 2] -= 1
    phi[:, 2] += 1

    def copy_bounds(a, b, v):
        rl, rh = a.clone(), b.clone()
        rl[:, pa] = rh[:, pa] = v
        res = hip.bounds(be, d(rl), d(rh), keep_layers=True)
        return res.lay_lb_full[:, :NH].contiguous(), res.lay_ub_full[:, :NH].contiguous()

    ph = []
    for k, v in enumerate((va, vb)):
        xv = x.clone()
        xv[:, pa] = v
        ph.append(d(_phase_at(m, xv, 23 + k, fix=0.2)))
    A, Bc, Brx = copy_bounds(lo, hi, va), copy_bounds(lo, hi, vb), copy_bounds(plo, phi, vb)
    osg = d(torch.tensor([1, -1], dtype=torch.int8).repeat(R)[:R])

    # phases taken at two different points of the box: each neuron's phase is reachable, all together
    # mostly not -- the regions the infeasibility pass exists for
    ph_any = []
    for k, v in enumerate((va, vb)):
        xv = _points(lo, hi, 40 + k)
        xv[:, pa] = v
        other = d(_phase_at(m, xv, 42 + k, fix=0.4))
        ph_any.append(torch.where(ph[k] != 0, ph[k], other))

    def common(relaxed, ph=ph):
        b = Brx if relaxed else Bc
        return (d(lo), d(hi), pa, d(va), d(vb), A[0], A[1], b[0], b[1], ph[0], ph[1])

    def fresh(seed=31):
        g = torch.Generator().manual_seed(seed)
        al = [d(torch.rand(R, NH, generator=g)) for _ in range(2)]
        return al + [torch.zeros(R, NH, device=dev) for _ in range(2)] + [torch.full((R,), 0.5, device=dev)]

    def tie(seed=32):
        g = torch.Generator().manual_seed(seed)
        return (ram, d(plo), d(phi), 1.0, d(torch.rand(R, 13, generator=g) * ram.float()),
                d(torch.rand(R, 13, generator=g) * ram.float()))

    def level(name, relaxed=False, **kw):
        par, rx = fresh(), (tie() if relaxed else None)
        lev = hip.beta_level(be, *common(relaxed), *par, 8, decay=0.98, lookahead=4, pgap=1, osg=osg, rx=rx,
                             feas_iters=4, **kw, **LR)
        for k in ("bound", "split", "xstar", "binit", "xpstar"):
            out[f"beta_level.{name}.{k}"] = getattr(lev, k)
        for k, v in zip(("alA", "alB", "beA", "beB", "t"), par):
            out[f"beta_level.{name}.{k}"] = v
        if rx is not None:
            out[f"beta_level.{name}.gP"], out[f"beta_level.{name}.gM"] = rx[4], rx[5]
        return lev, par

    lev, par = level("per_node")
    level("batched", batched=True)
    level("batched_feas", batched=True, batched_feas=True)
    level("relaxed_tie", relaxed=True)
    level("relaxed_tie_batched_feas", relaxed=True, batched=True, batched_feas=True)
    for name, relaxed in (("pa", False), ("relaxed_tie", True)):
        o = hip.beta_opt16(be, *common(relaxed), *fresh(), 8, LR["lr_a"], LR["lr_b"], LR["lr_t"], decay=0.98, pgap=1,
                           rx=tie() if relaxed else None, osg=osg)
        for k, v in zip(("par", "t", "gP", "gM", "pgsum", "pgn"), o):
            if v is not None:
                out[f"beta_opt16.{name}.{k}"] = v
    # the infeasibility pass alone, at the per-node level's best parameters with every row open, on
    # satisfiable (nothing closes) and on random phases
    bound = torch.full((R,), -1.0, dtype=torch.float64, device=dev)
    for name, relaxed, php in (("pa", False, ph), ("relaxed_tie", True, ph), ("pa_any", False, ph_any),
                               ("relaxed_tie_any", True, ph_any)):
        rest = (par[0], par[1], par[4], bound, 6, (0.1, 0.5, 0.1))
        kw = dict(decay=0.98, osg=osg)
        rx = lambda: tie() if relaxed else None  # noqa: E731
        c0, v0 = hip.beta_feas(be, *common(relaxed, php), *rest, False, rx=rx(), **kw)
        c1, v1, prop = hip.beta_feas(be, *common(relaxed, php), *rest, True, rx=rx(), return_proposal=True, **kw)
        c3, v3 = hip.beta_feas(be, *common(relaxed, php), *rest, True, rx=rx(), proposal=prop, **kw)
        for mode, c, v in ((0, c0, v0), (1, c1, v1), (3, c3, v3)):
            out[f"beta_feas.{name}.mode{mode}.closed"], out[f"beta_feas.{name}.mode{mode}.value"] = c, v
        out[f"beta_feas.{name}.fpar"] = prop[0]
        if prop[1] is not None:
            out[f"beta_feas.{name}.fgt"] = prop[1]


def dump(dev=None):
    """name -> numpy array of every output, in call order."""
    dev = torch.device("cuda:0") if dev is None else dev
    m = random_mlp(13, [8, 6, 4], seed=3, bias_scale=0.5)
    be = Backend(m, dev)
    assert be.hip, "the HIP extension must be active"
    out = {}
    with filled_empty():
        for family in (bound_family, sampling_family, beta_family):
            family(out, m, be, dev)
        torch.cuda.synchronize(dev)
        return {k: v.detach().cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def unwritten(arrays):
    """Names of the float arrays with elements no kernel wrote (still the fill value, NaN)."""
    return [k for k, v in arrays.items() if v.dtype.kind == "f" and np.isnan(v).any()]


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--against", default=None, help="an earlier dump: exit 1 unless every array is bitwise equal")
    a = ap.parse_args()
    arrays = dump()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"{len(arrays)} arrays, {sum(v.nbytes for v in arrays.values())} bytes -> {a.out}")
    print("arrays with unwritten elements:", ", ".join(unwritten(arrays)) or "none")
    if a.against:
        old = np.load(a.against)
        bad = sorted(set(old.files) ^ set(arrays)) + [k for k in arrays if k in old.files and not same_bits(arrays[k], old[k])]
        print(f"against {a.against}: {len(arrays) - len(bad)} equal, differing: {bad or 'none'}")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
