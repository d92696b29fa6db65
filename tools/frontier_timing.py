#!/usr/bin/env python
"""The device-resident BaB frontier (gnn_branching_amd/frontier.py) timed against the one-domain-per-iteration loop (GPU box).

cifar_base_kw, eps 0.09, seeded N(0,1) image (RandomState(4)), property 3 vs 5, n_iter 20, lr 0.1, eps_bab 1e-4, no decision bound.  Per
K in --ks: branch_and_bound_frontier for --rounds rounds; wall time between the root's log line and the last round's (each round ends
with the host's read of the state record, so the stamps are synchronised): ms per round, domains bounded per second, ms per domain, and
the same over the FULL rounds alone (those that expanded K domains: the frontier starts at one domain and at best doubles per round).
The baseline is lp_producer.branch_and_bound_threshold(child_lp="dual_device", branching_threshold=0: GNN decisions only, two domains
bounded per branch) for as many branches as the largest K bounded domains (at most --baseline-branches), its children's ascent set to
the same 20 iterations (the loop's own default is 100), stamps between its first and last branch line.

    python tools/frontier_timing.py [--out profiles/frontier_timing.json] [--ks 1,4,16,64] [--rounds 60,40,40,30] [--capacity 8192]

--split-depth none,2,4,8 measures DESIGN.md section 7.20 instead (default --out profiles/frontier_depth_timing.json): the same problem with
a fixed --decision-bound, so that a run ends on a verdict, per K in --ks (default 16,64) and per D of the list (none: no split_depth) one
untimed warm-up run of the whole search, then --repeats timed ones: rounds to the stop reason, wall clock, domains bounded, ms per round.
--parent-record FILE adds the record the same command wrote, with --split-depth none, from a checkout of the parent commit.

    python tools/frontier_timing.py --split-depth none,2,4,8 [--ks 16,64] [--decision-bound -0.15] [--max-rounds 200] [--repeats 2] [--parent-record FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import _lib, lp_producer, nets                # noqa: E402
from gnn_branching_amd.frontier import DomainPool, branch_and_bound_frontier      # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice       # noqa: E402

NET, EPS, N_ITER, LR, EPS_BAB = "cifar_base_kw", 0.09, 20, 0.1, 1e-4
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")


def commit_id():
    try:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() or None
    except OSError:
        return None


def frontier(lp, choice, K, rounds, capacity):
    stamps, picked = [], []

    def log(line):
        stamps.append(time.perf_counter())
        if " picked " in line:
            picked.append(int(line.split(" picked ")[1].split()[0]))
    branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, capacity=capacity, log=lambda s: None)      # warm-up: allocations, first launches
    glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=capacity, log=log)
    wall = stamps[-1] - stamps[0]
    n = bounded - 1
    full = [(stamps[i + 1] - stamps[i], k) for i, k in enumerate(picked) if k == K]      # rounds that expanded K domains
    return {"K": K, "rounds": done, "picked_per_round": picked, "full_rounds": len(full),
            "ms_per_full_round": round(1e3 * sum(t for t, _ in full) / len(full), 3) if full else None,
            "ms_per_domain_in_full_rounds": round(1e3 * sum(t for t, _ in full) / (2 * K * len(full)), 4) if full else None, "domains_bounded": n, "stop": reason, "global_lb": glb, "global_ub": gub, "seconds": round(wall, 4),
            "ms_per_round": round(1e3 * wall / max(done, 1), 3), "ms_per_domain": round(1e3 * wall / max(n, 1), 4),
            "domains_per_second": round(n / wall, 1) if wall > 0 else None}


def depth_runs(lp, choice, K, D, max_rounds, capacity, decision_bound, repeats):
    """One warm-up run of the whole search (untimed: every shape the timed runs launch), then ``repeats`` timed ones.  The span is
    ``frontier``'s: from the root's log line to the last round's."""
    lp.split_depth = D                                            # (the option travels on the root's description; a root of before it never reads it)

    def once():
        stamps, picked = [], []

        def log(line):
            stamps.append(time.perf_counter())
            if " picked " in line:
                picked.append(int(line.split(" picked ")[1].split()[0]))
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=max_rounds, capacity=capacity,
                                        decision_bound=decision_bound, log=log)
        return res, stamps[-1] - stamps[0], picked
    once()
    runs = [once() for _ in range(repeats)]
    (glb, gub, done, bounded, reason), _, picked = runs[0]
    secs = [r[1] for r in runs]
    return {"K": K, "split_depth": D, "rounds": done, "stop": reason, "global_lb": glb, "global_ub": gub,
            "verdict": "holds" if glb >= decision_bound else ("counter-example" if gub < decision_bound else "undecided"),
            "repeats_agree": all(r[0] == runs[0][0] for r in runs), "domains_bounded": bounded - 1, "picked_per_round": picked, "seconds": [round(t, 4) for t in secs],
            "seconds_best": round(min(secs), 4), "spread": round((max(secs) - min(secs)) / min(secs), 4) if min(secs) > 0 else None,
            "ms_per_round": round(1e3 * min(secs) / max(done, 1), 3)}


def depth_main(args, lp, choice, eng):
    depths = [None if d.strip().lower() == "none" else int(d) for d in args.split_depth.split(",")]
    out = args.out or os.path.join(ROOT, "profiles", "frontier_depth_timing.json")
    rec = {"what": f"branch_and_bound_frontier with and without split_depth (DESIGN.md section 7.20) on {NET}, eps {EPS}, property 3 vs 5, n_iter {N_ITER}, "
                   f"lr {LR}, BaB eps {EPS_BAB}, decision_bound {args.decision_bound}, at most {args.max_rounds} rounds; per run one untimed warm-up of the "
                   f"whole search, then {args.repeats} timed repeats; wall clock on the host from the root's record to the last round's, every round "
                   "synchronised by its state read; seconds_best is the least, spread (max - min) / min",
           "device": torch.cuda.get_device_name(), "commit": commit_id(), "library_build_id": _lib.library_build_id(), "pool_capacity": args.capacity,
           "decision_bound": args.decision_bound, "runs": [], "parent_commit": None}
    if args.parent_record:
        with open(args.parent_record) as f:
            parent = json.load(f)
        rec["parent_commit"] = {k: parent[k] for k in ("commit", "library_build_id", "runs")}
    for K in [int(k) for k in (args.ks or "16,64").split(",")]:
        for D in depths:
            rec["runs"].append(depth_runs(lp, choice, K, D, args.max_rounds, args.capacity, args.decision_bound, args.repeats))
            print(rec["runs"][-1], flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                json.dump(rec, f, indent=1)
    print("written", out)


def baseline(lp, choice, branches):
    from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
    solve_many = lp.solve_many
    lp.solve_many = lambda items, lp="highs", n_iter=100, lr=0.1: solve_many(items, lp=lp, n_iter=N_ITER, lr=LR)     # the frontier's 20 iterations
    stamps = []

    def kw(sub, icp, order, sparsest):
        return choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, order, sparsest)
    try:
        glb, gub, solves, done, _, _ = lp_producer.branch_and_bound_threshold(
            lp, lp_producer.gnn_scorer(choice, lp), kw, lp.layers, eps=EPS_BAB, max_branches=branches, branching_threshold=0.0,
            log=lambda s: stamps.append(time.perf_counter()), child_lp="dual_device")
    finally:
        del lp.solve_many
    if len(stamps) < 2:
        return {"branches": done, "note": "fewer than two branches: nothing to time"}
    wall, n = stamps[-1] - stamps[0], 2 * (len(stamps) - 1)
    return {"branches": done, "domains_bounded_in_the_timed_span": n, "global_lb": glb, "global_ub": gub, "seconds": round(wall, 4),
            "ms_per_domain": round(1e3 * wall / n, 4), "domains_per_second": round(n / wall, 1),
            "note": "root by HiGHS (outside the span); children by solve_many(lp='dual_device', n_iter=20); GNN decisions only"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/frontier_timing.json (profiles/frontier_depth_timing.json with --split-depth)")
    ap.add_argument("--ks", default=None, help="default 1,4,16,64 (16,64 with --split-depth)")
    ap.add_argument("--split-depth", default=None, metavar="LIST", help="e.g. none,2,4,8: measure split_depth (DESIGN.md section 7.20) instead")
    ap.add_argument("--decision-bound", type=float, default=-0.15, help="with --split-depth: the bound every run decides against")
    ap.add_argument("--max-rounds", type=int, default=200, help="with --split-depth: rounds at most")
    ap.add_argument("--repeats", type=int, default=2, help="with --split-depth: timed runs per setting")
    ap.add_argument("--parent-record", default=None, metavar="FILE", help="with --split-depth: the same command's record from the parent commit")
    ap.add_argument("--rounds", default="60,40,40,30")
    ap.add_argument("--baseline-branches", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=8192, help="slots of the pool")
    args = ap.parse_args()
    if args.split_depth is None:
        args.out, args.ks = args.out or os.path.join(ROOT, "profiles", "frontier_timing.json"), args.ks or "1,4,16,64"
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    lp = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng)
    eng.bind(list(layers[:-1]), (3, 32, 32))
    if args.split_depth is not None:
        return depth_main(args, lp, choice, eng)
    rec = {"what": "branch_and_bound_frontier (open domains in device memory, K expanded per round) vs branch_and_bound_threshold(child_lp='dual_device') "
                   f"on {NET}, eps {EPS}, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}; wall clock on the host, every round synchronised by its state read",
           "device": torch.cuda.get_device_name(), "commit": commit_id(), "library_build_id": _lib.library_build_id(),
           "pool_capacity": args.capacity, "bytes_per_open_domain": DomainPool.bytes_per_domain(eng.sizes, eng.R), "frontier": [], "baseline": None}
    for K, rounds in zip([int(k) for k in args.ks.split(",")], [int(r) for r in args.rounds.split(",")]):
        rec["frontier"].append(frontier(lp, choice, K, rounds, args.capacity))
        print(rec["frontier"][-1], flush=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    most = max(r["domains_bounded"] for r in rec["frontier"])
    rec["baseline"] = baseline(lp, choice, min(args.baseline_branches, max(2, most // 2)))
    print(rec["baseline"], flush=True)
    k1 = rec["frontier"][0]
    for r in rec["frontier"]:
        r["ms_per_domain_relative_to_first_K"] = round(r["ms_per_domain"] / k1["ms_per_domain"], 3) if k1["ms_per_domain"] else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
