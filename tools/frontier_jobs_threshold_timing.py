#!/usr/bin/env python
"""The BaBSR fall-back for every job of a many-job frontier (gnn_branching_amd/frontier.py verify_properties_threshold) timed in one
process (GPU box) against what a user could do before it and against the option off.

tools/frontier_jobs_timing.py's set-up: cifar_base_kw; job j: the box of eps 0.09 around the seeded N(0,1) stand-in image
RandomState(100 + j), true class 3, the wrong class cycling over the other nine; n_iter 20, lr 0.1, eps_bab 1e-4, no decision bound, every
job --rounds rounds at most, --capacity slots per job on every side, all J jobs in flight (segments = J); branching_threshold --threshold.
Configurations: J = 1 / 4 / 16 / 64 at K = 16.  Three sides alternate --repeats times after one warm-up each:

  (a) the same jobs one after the other through branch_and_bound_frontier(branching_threshold=T) -- per-job results asserted equal to (b);
  (b) verify_properties_threshold;
  (c) verify_properties, the option off.

Per side the median and the spread (max - min over the repeats) of the wall seconds of the whole call(s) and of the ROUND SPAN (from the
log line after the root(s) to the last round's line; every round ends with the host's read of the record(s), so the stamps are
synchronised) -> ms per round.  From (b)'s stats: the domains bounded, the share of the parents expanded that fell back and had a KW
decision bounded, the share that kept the KW pair, M (selected parents, all jobs together) per round.  The ratios: wall (a) / (b), ms per
round (b) / (c).  A difference counts only beyond three times the larger spread.  With --kernels, in a run of their own with
gnnb_profile_enable: the kernel classes' device time per round of (b) and of (c) at every configuration.

    python tools/frontier_jobs_threshold_timing.py [--out profiles/frontier_jobs_threshold_timing.json] [--rounds 8] [--capacity 129]
                                                   [--repeats 3] [--threshold 0.2] [--kernels]
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
from gnn_branching_amd.frontier import FrontierJob, branch_and_bound_frontier, verify_properties, verify_properties_threshold      # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice       # noqa: E402
from tools.frontier_jobs_timing import CKPT, EPS, EPS_BAB, GT, LR, N_ITER, NET, make_lps      # noqa: E402

CONFIGS = [(1, 16), (4, 16), (16, 16), (64, 16)]                        # (J, K)


def sequential(lps, choice, K, rounds, capacity, threshold):
    t0, span, results, all_stats = time.perf_counter(), 0.0, [], []
    for lp in lps:
        stamps, stats = [], {}
        results.append(branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=capacity,
                                                 log=lambda s: stamps.append(time.perf_counter()), branching_threshold=threshold, stats=stats))
        span += stamps[-1] - stamps[0]
        all_stats.append(stats)
    return {"wall": time.perf_counter() - t0, "span": span, "rounds": sum(r[2] for r in results)}, results, all_stats


def together(lps, choice, K, rounds, capacity, threshold):
    """verify_properties_threshold, or verify_properties with threshold None."""
    stamps, stats = [], []

    def log(line):
        if " root " in line or " picked " in line:
            stamps.append(time.perf_counter())
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps]
    kw = dict(K=K, segments=len(jobs), capacity=capacity, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=log)
    t0 = time.perf_counter()
    if threshold is None:
        results = verify_properties(choice, lps[0].layers[:-1], jobs, **kw)
    else:
        results = verify_properties_threshold(choice, lps[0].layers[:-1], jobs, threshold, stats=stats, **kw)
    return {"wall": time.perf_counter() - t0, "span": stamps[-1] - stamps[0], "rounds": max(r[2] for r in results)}, results, stats


def med_spread(vals):
    return {"median": round(statistics.median(vals), 4), "spread": round(max(vals) - min(vals), 4), "values": [round(v, 4) for v in vals]}


def summary(runs):
    return {"wall_seconds": med_spread([r["wall"] for r in runs]), "round_span_seconds": med_spread([r["span"] for r in runs]), "rounds": runs[0]["rounds"],
            "ms_per_round": med_spread([1e3 * r["span"] / max(r["rounds"], 1) for r in runs])}


def verdict(a, b, low, high):
    """a against b (med_spread dicts): which is lower beyond three times the larger spread."""
    noise = 3 * max(a["spread"], b["spread"])
    return low if b["median"] - a["median"] > noise else (high if a["median"] - b["median"] > noise else "no difference beyond 3x the spread")


def kernels_per_round(eng, lps, choice, K, rounds, capacity, threshold):
    """Device ms per kernel class and per round over the rounds of a many-job run (from its first k_frontier_pick_jobs on)."""
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True)
        eng.profile_trace(cap=1 << 17)
        info, _, _ = together(lps, choice, K, rounds, capacity, threshold)
        eng.profile_read(reset=True)
        trace = eng.profile_trace(cap=1 << 17)
    finally:
        eng.profile_enable(False)
    first = min(i for i, (name, _) in enumerate(trace) if name == "k_frontier_pick_jobs")
    per, n = {}, max(info["rounds"], 1)
    for name, ms in trace[first:]:
        per[name] = per.get(name, 0.0) + ms
    return {"J": len(lps), "K": K, "threshold": threshold, "rounds": info["rounds"], "kernel_ms_per_round": {k: round(v / n, 4) for k, v in sorted(per.items())},
            "sum_ms_per_round": round(sum(per.values()) / n, 3), "launches_per_round": round((len(trace) - first) / n, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_jobs_threshold_timing.json"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=129, help="slots per job, on every side")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--configs", default=",".join(f"{j}x{k}" for j, k in CONFIGS), help="JxK,...")
    ap.add_argument("--kernels", action="store_true", help="also the per-kernel device times, in runs of their own")
    args = ap.parse_args()
    torch.set_num_threads(16)
    T = args.threshold
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    layers = nets.load_verified_net(NET, GT, 5)
    x = torch.zeros(3, 32, 32)
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    lps = make_lps(max(j for j, _ in configs), eng)
    rec = {"what": f"(a) the jobs one after the other through branch_and_bound_frontier(branching_threshold={T}), (b) verify_properties_threshold, (c) "
                   f"verify_properties; all J jobs in flight (segments = J), {NET}, eps {EPS}, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, max_rounds "
                   f"{args.rounds}, {args.capacity} slots per job; host wall clock, every round synchronised by its read of the record(s); per side the "
                   "median and the spread (max - min) over the repeats, the sides alternating",
           "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "repeats": args.repeats, "threshold": T, "configs": [],
           "kernels": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    for J, K in configs:
        sub = lps[:J]
        sequential(sub[:1], choice, K, 2, args.capacity, T)           # warm-up: allocations, first launches at these shapes
        together(sub, choice, K, 2, args.capacity, T)
        together(sub, choice, K, 2, args.capacity, None)
        a_runs, b_runs, c_runs = [], [], []
        for _ in range(args.repeats):
            a, a_res, a_stats = sequential(sub, choice, K, args.rounds, args.capacity, T)
            b, b_res, b_stats = together(sub, choice, K, args.rounds, args.capacity, T)
            c, c_res, _ = together(sub, choice, K, args.rounds, args.capacity, None)
            assert a_res == b_res and a_stats == b_stats, "a job's result in the many-job run differs from its result alone"
            a_runs.append(a)
            b_runs.append(b)
            c_runs.append(c)
        branches, kw_bounded, kw_used = (sum(s[k] for s in b_stats) for k in ("branches", "kw_bounded", "kw_used"))
        row = {"J": J, "K": K, "stop_reasons": sorted({r[4] for r in b_res}), "stop_reasons_off": sorted({r[4] for r in c_res}),
               "domains_bounded": sum(r[3] for r in b_res), "domains_bounded_off": sum(r[3] for r in c_res), "parents_expanded": branches,
               "fell_back_and_bounded": kw_bounded, "fell_back_share": round(kw_bounded / max(branches, 1), 4), "kw_pair_kept": kw_used,
               "kw_pair_kept_share": round(kw_used / max(branches, 1), 4), "M_per_round": round(kw_bounded / max(b_runs[0]["rounds"], 1), 2),
               "one_after_the_other_threshold": summary(a_runs), "together_threshold": summary(b_runs), "together_off": summary(c_runs)}
        A, B, Cc = row["one_after_the_other_threshold"], row["together_threshold"], row["together_off"]
        row["wall_ratio_a_over_b"] = round(A["wall_seconds"]["median"] / B["wall_seconds"]["median"], 3)
        row["wall_verdict"] = verdict(B["wall_seconds"], A["wall_seconds"], "together ahead", "together behind")
        row["ms_per_round_ratio_b_over_c"] = round(B["ms_per_round"]["median"] / Cc["ms_per_round"]["median"], 3)
        row["ms_per_round_verdict"] = verdict(Cc["ms_per_round"], B["ms_per_round"], "the option costs", "the option is cheaper")
        rec["configs"].append(row)
        print(json.dumps(row), flush=True)
        write()
    if args.kernels:
        for J, K in configs:
            for thr in (T, None):
                rec["kernels"].append(kernels_per_round(eng, lps[:J], choice, K, args.rounds, args.capacity, thr))
                print(json.dumps(rec["kernels"][-1]), flush=True)
        write()
    print("written", args.out)


if __name__ == "__main__":
    main()
