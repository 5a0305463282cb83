"""Command line interface (replaces ``src/fairify.sh`` + the per-family copied driver scripts).

    python -m fairify_amd.cli presets
    python -m fairify_amd.cli verify --preset src/GC-age --models GC-1,GC-3 --out results/gc
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m fairify_amd.cli verify --preset stress/AC ...
    python -m fairify_amd.cli zoo [--import-dir /path/to/models]
    python -m fairify_amd.cli analyze --preset experiment/AC-3 --model AC-3 --fairer AC-3 ...
    python -m fairify_amd.cli measure --preset src/GC-age --model GC-1 --results results/gc --out results/gc-rate
    python -m fairify_amd.cli measure --preset src/GC-age --model GC-1 --certify [--node-budget N] [--leaf-points K]
    python -m fairify_amd.cli audit --preset src/AC-sex --model AC-3 [--data rows.csv] [--results results/ac] --out ...
    python -m fairify_amd.cli audit --preset src/GC-age --model GC-1 --neighbours --radius-of credit_amount=3 --out ...
    python -m fairify_amd.cli causal --preset src/AC-sex --model AC-3 --max-values 10 --out results/ac3-causal
    python -m fairify_amd.cli repair --model AC-3 --counterexamples results/ac3/counterexamples.csv ...
    python -m fairify_amd.cli export-cex --preset src/AC-sex --model AC-3 --results results/ac

The reference's only flag is ``sys.argv[1]`` = soft timeout (src/AC/Verify-AC.py:147-148);
every other constant is a preset field here and can be overridden on the command line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import replace


def _device(arg):
    import torch

    if arg:
        return arg
    return "cuda" if torch.cuda.is_available() else "cpu"


def cmd_presets(args):
    from . import presets

    for name, p in sorted(presets.PRESETS.items()):
        g = p.grid()
        print(f"{name:20s} suite={p.suite:9s} PA={','.join(p.query.pa):22s} RA={','.join(p.query.ra) or '-':9s} "
              f"tau={p.query.tau:<2d} P={p.partition_size:<4d} partitions={len(g):<9d} soft={p.soft_timeout:g}s "
              f"hard={p.hard_timeout:g}s models={len(p.models)}  [{p.source}]")


def cmd_verify(args):
    import os

    from .parallel import balance as BL

    # several ranks per node (torchrun): each takes the CPUs local to its GPU (sysfs NUMA locality,
    # parallel/balance.py) for its host threads / HIP streams / LP workers, before the GPU is touched
    BL.pin_rank(int(os.environ.get("LOCAL_RANK", "0")),
                int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
    from . import presets
    from .engine.pipeline import VerifyConfig
    from .engine.runner import run_preset
    from .parallel import dist as D

    pre = presets.get(args.preset)
    if args.partition_size:
        pre = replace(pre, partition_size=args.partition_size)
    info = D.init(_device(args.device))
    cfg = VerifyConfig(sim_size=args.sim_size or pre.sim_size, seed=args.seed, chunk=args.chunk,
                       soft_timeout=args.soft_timeout if args.soft_timeout is not None else pre.soft_timeout,
                       hard_timeout=args.hard_timeout if args.hard_timeout is not None else pre.hard_timeout,
                       node_budget=args.node_budget, heuristic=not args.no_heuristic,
                       heuristic_p=args.heuristic_p if args.heuristic_p is not None else pre.heuristic_p,
                       heuristic_node_budget=args.node_budget, smt_backend=args.smt,
                       escalate_budget=args.escalate_budget, escalate_max_open=args.escalate_max_open,
                       escalate_probation=tuple(tuple(int(v) for v in st.split(":"))
                                                for st in args.escalate_probation.split(",") if st),
                       keep_masks=args.keep_masks, lp_budget=args.lp_budget, trust_milp=args.trust_milp)
    if args.residual_samples is not None:
        cfg.residual_samples = args.residual_samples
    models = args.models.split(",") if args.models else None
    run_preset(pre, models=models, weights=args.weights, out_dir=args.out, cfg=cfg, info=info,
               max_partitions=args.max_partitions, resume=args.resume, seed=args.seed,
               accuracy=not args.no_accuracy, escalate=args.escalate,
               concurrency=args.concurrency or (4 if info.device.type == "cuda" else 1),
               anytime_budget=(args.anytime_budget or cfg.hard_timeout) if args.anytime else None,
               metrics_csv=True if args.metrics_csv else None, balance=args.balance)
    D.destroy(info)


def cmd_zoo(args):
    from .models.zoo import ZOO, get_model, has_weights

    if args.import_dir:
        import subprocess

        tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "import_zoo.py")
        subprocess.run([sys.executable, tool, args.import_dir], check=True)
    for name, (suite, n_in, hidden) in sorted(ZOO.items()):
        print(f"{name:10s} suite={suite:9s} {n_in}->{'-'.join(map(str, hidden))}->1 "
              f"weights={'shipped' if has_weights(name) else 'random-only'}")


def cmd_analyze(args):
    from .analysis.report import analyze_model

    out = analyze_model(args.preset, args.model, fairer=args.fairer, results=args.results, weights=args.weights,
                        seed=args.seed, out_dir=args.out, device=_device(args.device),
                        causal_samples=args.causal_max)
    print(json.dumps(out, indent=2, default=float))


def cmd_measure(args):
    from .analysis.rate import measure_preset

    out = measure_preset(args.preset, args.model, results=args.results, n_samples=args.samples, seed=args.seed,
                         max_partitions=args.max_partitions, check_unsat=args.check_unsat, weights=args.weights,
                         device=_device(args.device), out_dir=args.out, certify=args.certify,
                         node_budget=args.node_budget, leaf_points=args.leaf_points)
    print(json.dumps(out, indent=2, default=float))


def cmd_gap(args):
    from .analysis.gap import gap_preset

    out = gap_preset(args.preset, args.model, results=args.results, tol=args.tol, node_budget=args.node_budget,
                     leaf_points=args.leaf_points, max_partitions=args.max_partitions, seed=args.seed,
                     weights=args.weights, device=_device(args.device), out_dir=args.out)
    print(json.dumps(out, indent=2, default=float))


def cmd_audit(args):
    from .analysis.audit import audit_preset

    out = audit_preset(args.preset, args.model, data=args.data, split=args.split, results=args.results,
                       weights=args.weights, seed=args.seed, device=_device(args.device), max_rows=args.max_rows,
                       out_dir=args.out, pairs_out=args.pairs_out, neighbours=args.neighbours, radius=args.radius,
                       radius_of=_radius_of(args.radius_of))
    print(json.dumps(out, indent=2, default=float))


def cmd_causal(args):
    from .analysis.causal_sets import causal_preset

    out = causal_preset(args.preset, args.model, max_size=args.max_size, samples=args.samples, seed=args.seed,
                        threshold=args.threshold, conf=args.conf, margin=args.margin, min_samples=args.min_samples,
                        values=args.values, max_values=args.max_values, max_assignments=args.max_assignments,
                        base=args.base, data=args.data, split=args.split, weights=args.weights,
                        device=_device(args.device), out_dir=args.out, pairs_out=args.pairs_out)
    print(json.dumps(out, indent=2, default=float))


def _radius_of(items):
    """``name=R`` arguments -> {name: R}."""
    out = {}
    for it in items or []:
        name, sep, r = it.partition("=")
        if not sep or not name or not r:
            raise SystemExit(f"--radius-of {it!r}: expected name=R with R an integer or 'full'")
        out[name] = r
    return out


def cmd_repair(args):
    if args.method == "finetune":
        # GC/BM recipe: fine-tune on a synthetic CSV with early stopping (src/GC/new_model.py:8-58,
        # src/BM/new_model.py:8-40)
        from .models.zoo import get_model
        from .repair.finetune import finetune_csv

        if not args.data or not args.suite:
            raise SystemExit("--method finetune needs --data CSV and --suite german|bank")
        m = get_model(args.model, weights=args.weights, seed=args.seed)
        r = finetune_csv(m, args.data, args.suite, lr=args.lr, epochs=args.max_epochs, seed=args.seed,
                         device=_device(args.device), name=os.path.splitext(os.path.basename(args.out))[0])
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        r.model.save_npz(args.out if args.out.endswith(".npz") else args.out + ".npz")
        print(json.dumps({"model": args.model, "out": args.out, "epochs_run": r.epochs_run, "best_epoch": r.best_epoch,
                          "val_acc": r.val_acc, "val_loss": r.val_loss, "train_rows": r.train_rows,
                          "val_rows": r.val_rows}, indent=2))
        return
    from .repair.retrain import repair_model

    out = repair_model(args.model, counterexamples=args.counterexamples, method=args.method, out=args.out,
                       top_k=args.top_k, epochs=args.epochs, weights=args.weights, seed=args.seed,
                       device=_device(args.device))
    print(json.dumps(out, indent=2, default=float))


def cmd_export(args):
    from .report.counterexamples import export_counterexamples

    path = export_counterexamples(args.preset, args.model, args.results, out=args.out, weights=args.weights)
    print(path)


def cmd_export_smt(args):
    """Write the SMT-LIB2 query of partitions (sound-pruned on the box) for external solvers."""
    import numpy as np
    import torch

    from . import presets
    from .engine import prune as P_
    from .models.zoo import get_model
    from .ops.backend import Backend
    from .partition import processing_order
    from .smt import encode_partition, pruned_network

    pre = presets.get(args.preset)
    grid = pre.grid()
    q = pre.resolved()
    m = get_model(args.model, weights=args.weights, seed=args.seed)
    order = processing_order(grid, seed=args.seed)
    ids = order[:args.count] if args.ids is None else np.array([int(x) for x in args.ids.split(",")])
    lo, hi = grid.decode(ids)
    be = Backend(m, device=_device(args.device))
    r = be.bounds(torch.from_numpy(lo).float().to(be.device), torch.from_numpy(hi).float().to(be.device),
                  mode="ibp", keep_layers=True)
    nh = int(sum(m.hidden))
    dead = torch.cat(r.layer_ub, dim=1)[:, :nh] <= 0
    dead = P_.ensure_one_alive(torch.cat([dead, torch.zeros_like(dead[:, :1])], dim=1), m.widths)[:, :nh]
    dead = dead.cpu().numpy()
    os.makedirs(args.out, exist_ok=True)
    for k, gid in enumerate(ids):
        net = pruned_network(m, dead[k])
        text = encode_partition(net, q, lo[k], hi[k], timeout_s=args.timeout, fork_params=args.fork_params).text
        path = os.path.join(args.out, f"{args.model}-p{int(gid)}.smt2")
        with open(path, "w") as f:
            f.write(text)
        print(path, f"(pruned {m.n_neurons - net.n_neurons} of {m.n_neurons} neurons)")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="fairify_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("presets").set_defaults(fn=cmd_presets)

    v = sub.add_parser("verify", help="verify a preset's models (torchrun for multi-GPU)")
    v.add_argument("--preset", required=True)
    v.add_argument("--models", default=None)
    v.add_argument("--weights", default="zoo", help="zoo | random | path/to/model.h5")
    v.add_argument("--out", default="results")
    v.add_argument("--partition-size", type=int, default=None)
    v.add_argument("--soft-timeout", type=float, default=None)
    v.add_argument("--hard-timeout", type=float, default=None)
    v.add_argument("--heuristic-p", type=float, default=None)
    v.add_argument("--no-heuristic", action="store_true")
    v.add_argument("--node-budget", type=int, default=4096)
    v.add_argument("--sim-size", type=int, default=None)
    v.add_argument("--chunk", type=int, default=4096)
    v.add_argument("--seed", type=int, default=0)
    v.add_argument("--max-partitions", type=int, default=None)
    v.add_argument("--resume", action="store_true")
    v.add_argument("--escalate", type=int, default=1,
                   help="retry each round's UNKNOWN partitions on all ranks with N x the node budget")
    v.add_argument("--escalate-budget", type=int, default=0,
                   help="second sound BaB pass with this node budget on each chunk's UNKNOWN residue")
    v.add_argument("--escalate-probation", default="",
                   help="inline escalation steps 'budget:max_open,...' between the node budget and "
                        "--escalate-budget (native BaB; bench default 2048:768,4096:768,8192:768,16384:1024 with --escalate-budget 32768)")
    v.add_argument("--escalate-max-open", type=int, default=0,
                   help="escalate only residue partitions that left <= this many open BaB nodes (0 = all)")
    v.add_argument("--balance", default="queue", choices=["queue", "strided"],
                   help="several ranks: claim units of each round from a shared atomic counter (queue, dynamic "
                        "load balance) or verify fixed strided shares (strided)")
    v.add_argument("--concurrency", type=int, default=0,
                   help="chunks verified at once per rank, one HIP stream each (default 4 on GPU, 1 on CPU)")
    v.add_argument("--smt", default="auto", help="host SMT back-end for the residue: auto | z3py | z3bin | none")
    v.add_argument("--lp-budget", type=int, default=4096,
                   help="without Z3 (--smt auto/milp): verified-LP branch-and-bound nodes per partition on the "
                        "residue, sound UNSAT (smt/lpbab.py); 0 = the HiGHS MILP, whose UNSAT is not a proof")
    v.add_argument("--trust-milp", action="store_true",
                   help="count HiGHS MILP UNSAT (floating-point dual bound) as verdicts (stage 'milp', excluded "
                        "from the sound figures); implies the MILP stage")
    v.add_argument("--anytime", action="store_true",
                   help="spend the per-model wall budget (--anytime-budget, default the preset's hard timeout) on "
                        "growing sound BaB budgets and falsifier rounds over the UNKNOWN residue")
    v.add_argument("--anytime-budget", type=float, default=None, help="seconds per model for --anytime")
    v.add_argument("--keep-masks", action="store_true",
                   help="gather every partition's final dead-neuron mask (packed bitset) to rank 0 and write "
                        "OUT/masks/<model>.npz with the unique masks (dedup) for pruned-subnet export")
    v.add_argument("--residual-samples", type=int, default=None)
    v.add_argument("--metrics-csv", action="store_true",
                   help="also write the per-partition metrics CSV of the experiment drivers "
                        "(on by default for experiment/* presets)")
    v.add_argument("--no-accuracy", action="store_true")
    v.add_argument("--device", default=None)
    v.set_defaults(fn=cmd_verify)

    z = sub.add_parser("zoo", help="list the model zoo / import Keras .h5 models")
    z.add_argument("--import-dir", default=None)
    z.set_defaults(fn=cmd_zoo)

    a = sub.add_parser("analyze", help="group metrics, causal discrimination, hybrid routing")
    a.add_argument("--preset", required=True)
    a.add_argument("--model", required=True)
    a.add_argument("--fairer", default=None)
    a.add_argument("--results", default=None, help="results dir of a verify run (partition verdicts)")
    a.add_argument("--weights", default="zoo")
    a.add_argument("--seed", type=int, default=0)
    a.add_argument("--out", default=None)
    a.add_argument("--causal-max", type=int, default=1000)
    a.add_argument("--device", default=None)
    a.set_defaults(fn=cmd_analyze)

    ms = sub.add_parser("measure", help="per-partition discrimination rates + stratified domain-wide estimate")
    ms.add_argument("--preset", required=True)
    ms.add_argument("--model", required=True)
    ms.add_argument("--results", default=None,
                    help="results dir of a verify run: UNSAT partitions count as rate 0 and are not sampled")
    ms.add_argument("--samples", type=int, default=1000, help="profiles per partition")
    ms.add_argument("--seed", type=int, default=0)
    ms.add_argument("--max-partitions", type=int, default=None)
    ms.add_argument("--check-unsat", action="store_true",
                    help="sample the UNSAT partitions too; an exact flip inside one is a prover bug (SoundnessError)")
    ms.add_argument("--weights", default="zoo")
    ms.add_argument("--device", default=None)
    ms.add_argument("--certify", action="store_true",
                    help="count the sampled partitions with the counting branch-and-bound: bounds.csv and "
                         "certified_lower / certified_upper in rate.json")
    ms.add_argument("--node-budget", type=int, default=65536, help="--certify: nodes box-tested per partition")
    ms.add_argument("--leaf-points", type=int, default=1024,
                    help="--certify: open nodes of at most this many points are enumerated (<= 65536)")
    ms.add_argument("--out", default=None, help="directory for rate.csv / rate.json (and bounds.csv)")
    ms.set_defaults(fn=cmd_measure)

    gp = sub.add_parser("gap", help="certified largest score gap between counterparts, per partition",
                        description="Brackets, per partition, the largest |logit(x) - logit(x')| over the pairs the "
                                    "query relates (gap_lo <= G <= gap_hi, units of the logit) with an exactly "
                                    "evaluated witness pair.  FAIRIFY_GAP_FUSED=1 enumerates leaves with the fused GPU "
                                    "kernel (networks with at most 32 inputs, layers up to 160 wide and 64 KB of LDS); "
                                    "otherwise the composed path runs.  Writes gap.csv / gap.json.")
    gp.add_argument("--preset", required=True)
    gp.add_argument("--model", required=True)
    gp.add_argument("--results", default=None,
                    help="results dir of a verify run: maxima per verdict class; a witness that flips inside an "
                         "UNSAT partition is a prover bug (SoundnessError)")
    gp.add_argument("--tol", type=float, default=0.01, help="a node within this of the incumbent is pruned")
    gp.add_argument("--node-budget", type=int, default=65536, help="nodes bounded per partition")
    gp.add_argument("--leaf-points", type=int, default=1024,
                    help="open nodes of at most this many points are enumerated (<= 65536)")
    gp.add_argument("--max-partitions", type=int, default=None)
    gp.add_argument("--seed", type=int, default=0)
    gp.add_argument("--weights", default="zoo")
    gp.add_argument("--device", default=None)
    gp.add_argument("--out", required=True, help="directory for gap.csv / gap.json")
    gp.set_defaults(fn=cmd_gap)

    au = sub.add_parser("audit", help="exact per-row discrimination flags of a table of individuals")
    au.add_argument("--preset", required=True)
    au.add_argument("--model", required=True)
    au.add_argument("--data", default=None,
                    help="CSV of encoded integer rows whose header holds the domain's feature names "
                         "(default: the suite's dataset)")
    au.add_argument("--split", default="all", choices=["all", "train", "test"], help="without --data: which rows")
    au.add_argument("--results", default=None,
                    help="results dir of a verify run: rows per verdict class; a flagged row inside an UNSAT "
                         "partition is a prover bug (SoundnessError)")
    au.add_argument("--max-rows", type=int, default=None)
    au.add_argument("--pairs-out", default=None,
                    help="FILE.npz: one exactly confirmed pair (x, xp) per flagged row, for repair --counterexamples")
    au.add_argument("--seed", type=int, default=0)
    au.add_argument("--weights", default="zoo")
    au.add_argument("--device", default=None)
    au.add_argument("--neighbours", action="store_true",
                    help="also decide every row's single-attribute neighbours (one non-protected attribute set to "
                         "another value of its domain): neighbours.csv / neighbours.json with the rows that are "
                         "flagged, exposed (a flagged neighbour) or robust (a proof that there is none)")
    au.add_argument("--radius", default="full",
                    help="--neighbours: largest change of an attribute, an integer or 'full' (the whole range)")
    au.add_argument("--radius-of", action="append", default=[], metavar="NAME=R",
                    help="--neighbours: radius of one feature (repeatable); wide features need one")
    au.add_argument("--out", default=None, help="directory for audit.csv / audit.json")
    au.set_defaults(fn=cmd_audit)

    ca = sub.add_parser("causal", help="search attribute sets (1..4 attributes) for causal discrimination: which "
                                       "attributes do the decisions depend on at all",
                        description="Themis's discrimination search with exact flip bits.  One base table is shared "
                                    "by all sets (the reference draws one per set).  A set has at most 4 attributes "
                                    "and at most --max-assignments assignments; the fused GPU kernel covers networks "
                                    "with at most 32 inputs, layers up to 160 wide and 64 KB of staged weights and "
                                    "is the default there (FAIRIFY_CAUSAL_FUSED=0: the composed path); other shapes "
                                    "take the composed path.  Writes causal.csv / causal.json.")
    ca.add_argument("--preset", required=True)
    ca.add_argument("--model", required=True)
    ca.add_argument("--max-size", type=int, default=2, choices=[1, 2, 3, 4], help="largest attribute set")
    ca.add_argument("--samples", type=int, default=1000,
                    help="base rows; one table is shared by all sets (common random numbers)")
    ca.add_argument("--seed", type=int, default=42, help="seed of the drawn base table")
    ca.add_argument("--threshold", type=float, default=0.15, help="a set is discriminatory above this rate")
    ca.add_argument("--conf", type=float, default=0.99)
    ca.add_argument("--margin", type=float, default=0.01)
    ca.add_argument("--min-samples", type=int, default=100)
    ca.add_argument("--values", default="data", choices=["data", "domain"],
                    help="value lists: the values observed in the dataset (default), or the whole range lo..hi")
    ca.add_argument("--max-values", type=int, default=None, metavar="K",
                    help="thin a longer list to K values evenly spaced by rank, first and last kept")
    ca.add_argument("--max-assignments", type=int, default=4096,
                    help="a set with more assignments (the product of its list sizes) is not tested")
    ca.add_argument("--base", default="sampled", choices=["sampled", "data"],
                    help="base rows: drawn from the value lists, or the first --samples real rows (0: all)")
    ca.add_argument("--data", default=None,
                    help="CSV of encoded integer rows whose header holds the domain's feature names "
                         "(default: the suite's dataset)")
    ca.add_argument("--split", default="all", choices=["all", "train", "test"], help="without --data: which rows")
    ca.add_argument("--pairs-out", default=None,
                    help="FILE.npz: the exactly confirmed pair (x, xp) of every discriminatory set, for "
                         "repair --counterexamples")
    ca.add_argument("--weights", default="zoo")
    ca.add_argument("--device", default=None)
    ca.add_argument("--out", default=None, help="directory for causal.csv / causal.json")
    ca.set_defaults(fn=cmd_causal)

    r = sub.add_parser("repair", help="bias localisation + masked fine-tune / counterexample retraining")
    r.add_argument("--model", required=True)
    r.add_argument("--counterexamples", default=None)
    r.add_argument("--method", default="masked", choices=["masked", "retrain", "finetune"])
    r.add_argument("--data", default=None, help="finetune: synthetic CSV (reference experimentData layout)")
    r.add_argument("--suite", default=None, choices=["german", "bank"], help="finetune: column spec")
    r.add_argument("--lr", type=float, default=5e-4)
    r.add_argument("--max-epochs", type=int, default=100, help="finetune: epochs before early stopping")
    r.add_argument("--out", required=True)
    r.add_argument("--top-k", type=int, default=10)
    r.add_argument("--epochs", type=int, default=5)
    r.add_argument("--weights", default="zoo")
    r.add_argument("--seed", type=int, default=0)
    r.add_argument("--device", default=None)
    r.set_defaults(fn=cmd_repair)

    e = sub.add_parser("export-cex", help="decode counterexamples of a verify run to category labels")
    e.add_argument("--preset", required=True)
    e.add_argument("--model", required=True)
    e.add_argument("--results", required=True)
    e.add_argument("--out", default=None)
    e.add_argument("--weights", default="zoo")
    e.set_defaults(fn=cmd_export)

    x = sub.add_parser("export-smt", help="write SMT-LIB2 partition queries (GPU-pruned) for external solvers")
    x.add_argument("--preset", required=True)
    x.add_argument("--model", required=True)
    x.add_argument("--out", required=True)
    x.add_argument("--count", type=int, default=4, help="first N partitions of the seeded order")
    x.add_argument("--ids", default=None, help="comma list of grid ids (overrides --count)")
    x.add_argument("--timeout", type=float, default=100.0)
    x.add_argument("--fork-params", action="store_true")
    x.add_argument("--weights", default="zoo")
    x.add_argument("--seed", type=int, default=0)
    x.add_argument("--device", default=None)
    x.set_defaults(fn=cmd_export_smt)

    args = ap.parse_args(argv)
    args.fn(args)


if __name__ == "__main__":
    main()
