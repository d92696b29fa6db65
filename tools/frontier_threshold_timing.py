#!/usr/bin/env python
"""The BaBSR fall-back below a branching threshold inside the device-resident frontier, timed (GPU box).

cifar_base_kw, eps 0.09, seeded N(0,1) image (RandomState(4)), property 3 vs 5, n_iter 20, lr 0.1, eps_bab 1e-4, no decision bound: the
set-up of tools/frontier_timing.py (section 7.3).  Per K in --ks, at a fixed max_rounds: branch_and_bound_frontier with
branching_threshold=None ("off") and =--threshold ("on"), one warm-up run each, then --repeats timed runs each with the sides
alternating; wall time between the root's log line and the last round's (every round ends with the host's read of the state record).
Recorded per side: median and min / max of ms per round and ms per domain over the repeats, rounds, domains bounded, stop reason, final
bounds; for "on" also the share of expanded parents whose KW pair was bounded and whose KW pair won.  The committed
profiles/frontier_timing.json (the parent's figures for the option-less loop) is copied beside "off" for the same K.  Then, in runs of
their own: the ms of the new entry points' kernels per launch from gnnb_profile_enable, and
lp_producer.branch_and_bound_threshold(child_lp="dual_device", branching_threshold=--threshold), the loop the mode moves onto the device.

    python tools/frontier_threshold_timing.py [--out profiles/frontier_threshold_timing.json] [--ks 1,16,64] [--rounds 60,40,30] [--threshold 0.2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import _lib, lp_producer, nets                # noqa: E402
from gnn_branching_amd.frontier import branch_and_bound_frontier     # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice       # noqa: E402

NET, EPS, N_ITER, LR, EPS_BAB = "cifar_base_kw", 0.09, 20, 0.1, 1e-4
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
NEW_KERNELS = ("k_frontier_candidates", "k_frontier_fallback", "k_frontier_choose", "k_frontier_choose_copy")


def one_run(lp, choice, K, rounds, capacity, threshold):
    stamps, stats = [], {}
    glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                                                capacity=capacity, log=lambda s: stamps.append(time.perf_counter()),
                                                                branching_threshold=threshold, stats=stats)
    wall = stamps[-1] - stamps[0]
    return {"seconds": wall, "rounds": done, "domains_bounded": bounded - 1, "stop": reason, "global_lb": glb, "global_ub": gub, "stats": stats}


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def summary(runs):
    last = runs[-1]
    out = {"ms_per_round": spread([1e3 * r["seconds"] / max(r["rounds"], 1) for r in runs]),
           "ms_per_domain": spread([1e3 * r["seconds"] / max(r["domains_bounded"], 1) for r in runs]),
           "rounds": last["rounds"], "domains_bounded": last["domains_bounded"], "stop": last["stop"], "global_lb": last["global_lb"],
           "global_ub": last["global_ub"], "gap": last["global_ub"] - last["global_lb"],
           "same_result_in_every_repeat": all((r["global_lb"], r["global_ub"], r["domains_bounded"]) == (last["global_lb"], last["global_ub"], last["domains_bounded"])
                                              for r in runs)}
    st = last["stats"]
    if st.get("branches"):
        out.update(parents_expanded=st["branches"], kw_pairs_bounded=st["kw_bounded"], kw_pairs_used=st["kw_used"],
                   share_fell_back=round(st["kw_bounded"] / st["branches"], 4), share_kw_won=round(st["kw_used"] / st["branches"], 4))
    return out


def profiled(lp, choice, eng, K, rounds, capacity, threshold):
    """ms per launch of the new kernels (HIP events around every launch: a run of its own, never a timed one)."""
    eng.profile_enable(1)
    try:
        eng.profile_read(reset=True)
        r = one_run(lp, choice, K, rounds, capacity, threshold)
        prof = eng.profile_read(reset=True)
    finally:
        eng.profile_enable(0)
    out = {k: {"launches": int(prof[k][1]), "ms_per_launch": round(prof[k][0] / prof[k][1], 5) if prof[k][1] else None} for k in NEW_KERNELS}
    out["ms_of_the_new_kernels_per_round"] = round(sum(prof[k][0] for k in NEW_KERNELS) / max(r["rounds"], 1), 5)
    return out


def host_loop(lp, choice, branches, threshold):
    from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
    solve_many = lp.solve_many
    lp.solve_many = lambda items, lp="highs", n_iter=100, lr=0.1: solve_many(items, lp=lp, n_iter=N_ITER, lr=LR)     # the frontier's 20 iterations
    stamps = []

    def kw(sub, icp, order, sparsest):
        return choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, order, sparsest)
    try:
        glb, gub, solves, done, n_kw, n_used = lp_producer.branch_and_bound_threshold(
            lp, lp_producer.gnn_scorer(choice, lp), kw, lp.layers, eps=EPS_BAB, max_branches=branches, branching_threshold=threshold,
            log=lambda s: stamps.append(time.perf_counter()), child_lp="dual_device")
    finally:
        del lp.solve_many
    if len(stamps) < 2:
        return {"branches": done, "note": "fewer than two branches: nothing to time"}
    wall = stamps[-1] - stamps[0]
    n = solves * (len(stamps) - 1) / max(len(stamps), 1)           # the first branch's solves lie before the first stamp
    return {"branches": done, "kw_pairs_bounded": n_kw, "kw_pairs_used": n_used, "domains_bounded": solves, "global_lb": glb, "global_ub": gub,
            "seconds": round(wall, 4), "ms_per_domain": round(1e3 * wall / n, 4), "ms_per_branch": round(1e3 * wall / (len(stamps) - 1), 4),
            "note": "root by HiGHS (outside the span); children by solve_many(lp='dual_device', n_iter=20); stamps at the branch lines"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_threshold_timing.json"))
    ap.add_argument("--ks", default="1,16,64")
    ap.add_argument("--rounds", default="60,40,30")
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-branches", type=int, default=60)
    ap.add_argument("--capacity", type=int, default=8192, help="slots of the pool")
    args = ap.parse_args()
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    lp = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng)
    eng.bind(list(layers[:-1]), (3, 32, 32))
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "frontier_timing.json")) as f:
            prev = json.load(f)
        parent = {r["K"]: {k: r[k] for k in ("rounds", "ms_per_round", "ms_per_domain", "domains_bounded", "global_lb", "global_ub")} for r in prev["frontier"]}
        parent["library_build_id"] = prev.get("library_build_id")
    except (OSError, KeyError, ValueError):
        pass
    rec = {"what": f"branch_and_bound_frontier with branching_threshold=None (off) and {args.threshold} (on) on {NET}, eps {EPS}, property 3 vs 5, n_iter {N_ITER}, "
                   f"lr {LR}, BaB eps {EPS_BAB}; wall clock on the host, every round synchronised by its state read; one warm-up run per side, then "
                   f"{args.repeats} repeats per side, the sides alternating; median and min / max over the repeats",
           "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "pool_capacity": args.capacity,
           "branching_threshold": args.threshold, "frontier": [], "host_loop": None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for K, rounds in zip([int(k) for k in args.ks.split(",")], [int(r) for r in args.rounds.split(",")]):
        sides = {"off": None, "on": args.threshold}
        for thr in sides.values():                                # warm-up: allocations, first launches
            branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, capacity=args.capacity, log=lambda s: None,
                                      branching_threshold=thr)
        runs = {"off": [], "on": []}
        for _ in range(args.repeats):
            for side, thr in sides.items():                       # alternating
                runs[side].append(one_run(lp, choice, K, rounds, args.capacity, thr))
        entry = {"K": K, "max_rounds": rounds, "off": summary(runs["off"]), "on": summary(runs["on"]),
                 "parent_commit_frontier_timing": parent.get(K), "parent_commit_library_build_id": parent.get("library_build_id"),
                 "profile_of_the_new_kernels": profiled(lp, choice, eng, K, rounds, args.capacity, args.threshold)}
        entry["on_over_off_ms_per_round"] = round(entry["on"]["ms_per_round"]["median"] / entry["off"]["ms_per_round"]["median"], 3)
        rec["frontier"].append(entry)
        print(json.dumps(entry), flush=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    rec["host_loop"] = host_loop(lp, choice, args.host_branches, args.threshold)
    print(json.dumps(rec["host_loop"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
