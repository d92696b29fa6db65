#!/usr/bin/env python
"""Many verification jobs in one frontier (gnn_branching_amd/frontier.py verify_properties) timed against the same jobs run one after the
other through branch_and_bound_frontier, in one process (GPU box).

cifar_base_kw; job j: the box of eps 0.09 around the seeded N(0,1) stand-in image RandomState(100 + j), true class 3, the wrong class
cycling over the other nine; n_iter 20, lr 0.1, eps_bab 1e-4, no decision bound, every job --rounds rounds at most, --capacity slots per
job on both sides, all J jobs in flight (segments = J).  Configurations: J = 1 / 4 / 16 / 64 at K = 16 and J = 64 at K = 4.  The two sides
alternate --repeats times after one warm-up each; per side the median and the spread (max - min over the repeats) of

  * wall seconds of the whole call(s), allocations and roots included -> jobs per second;
  * the ROUND SPAN: from the log line after the root(s) to the last round's line (each round ends with the host's read of the
    record(s), so the stamps are synchronised) -> ms per round, domains bounded per second.  The sequential side's span is the sum of
    its jobs' spans and its rounds the sum of their rounds.

A difference counts only beyond three times the larger spread.  The per-job results of the two sides must be equal (asserted).  In a run
of their own, with gnnb_profile_enable: the kernel classes' device time in the LAST round of a many-job run at J = 16 and J = 64.

    python tools/frontier_jobs_timing.py [--out profiles/frontier_jobs_timing.json] [--rounds 8] [--capacity 129] [--repeats 3]
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
from gnn_branching_amd.frontier import FrontierJob, branch_and_bound_frontier, verify_properties      # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice       # noqa: E402

NET, EPS, N_ITER, LR, EPS_BAB, GT = "cifar_base_kw", 0.09, 20, 0.1, 1e-4, 3
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
CONFIGS = [(1, 16), (4, 16), (16, 16), (64, 16), (64, 4)]              # (J, K)


def make_lps(J, eng):
    wrong = [c for c in range(10) if c != GT]
    lps = []
    for j in range(J):
        layers = nets.load_verified_net(NET, GT, wrong[j % 9])
        x = torch.from_numpy(np.random.RandomState(100 + j).standard_normal((3, 32, 32)).astype(np.float32))
        lps.append(lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng))
    return lps


def sequential(lps, choice, K, rounds, capacity):
    t0, span, results = time.perf_counter(), 0.0, []
    for lp in lps:
        stamps = []
        results.append(branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=capacity,
                                                 log=lambda s: stamps.append(time.perf_counter())))
        span += stamps[-1] - stamps[0]
    return {"wall": time.perf_counter() - t0, "span": span, "rounds": sum(r[2] for r in results)}, results


def together(lps, choice, K, rounds, capacity):
    stamps = []

    def log(line):
        if " root " in line or " picked " in line:
            stamps.append(time.perf_counter())
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps]
    t0 = time.perf_counter()
    results = verify_properties(choice, lps[0].layers[:-1], jobs, K=K, segments=len(jobs), capacity=capacity, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                                max_rounds=rounds, log=log)
    return {"wall": time.perf_counter() - t0, "span": stamps[-1] - stamps[0], "rounds": max(r[2] for r in results)}, results


def summary(runs, J, domains):
    def med_spread(vals):
        return {"median": round(statistics.median(vals), 4), "spread": round(max(vals) - min(vals), 4), "values": [round(v, 4) for v in vals]}
    return {"wall_seconds": med_spread([r["wall"] for r in runs]), "round_span_seconds": med_spread([r["span"] for r in runs]), "rounds": runs[0]["rounds"],
            "ms_per_round": med_spread([1e3 * r["span"] / max(r["rounds"], 1) for r in runs]),
            "domains_per_second": med_spread([domains / r["span"] for r in runs]), "jobs_per_second": med_spread([J / r["wall"] for r in runs])}


def last_round_kernels(eng, lps, choice, K, rounds, capacity):
    """Device ms per kernel class over the launches of the last round of a many-job run (from its k_frontier_pick_jobs on)."""
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True)
        eng.profile_trace(cap=1 << 16)
        _, results = together(lps, choice, K, rounds, capacity)
        eng.profile_read(reset=True)
        trace = eng.profile_trace(cap=1 << 16)
    finally:
        eng.profile_enable(False)
    last = max(i for i, (name, _) in enumerate(trace) if name == "k_frontier_pick_jobs")
    per = {}
    for name, ms in trace[last:]:
        per[name] = round(per.get(name, 0.0) + ms, 4)
    return {"J": len(lps), "K": K, "kernel_ms": per, "sum_ms": round(sum(per.values()), 3), "launches": len(trace) - last}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_jobs_timing.json"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=129, help="slots per job, on both sides")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default=",".join(f"{j}x{k}" for j, k in CONFIGS), help="JxK,...")
    args = ap.parse_args()
    torch.set_num_threads(16)
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    layers = nets.load_verified_net(NET, GT, 5)
    x = torch.zeros(3, 32, 32)
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    lps = make_lps(max(j for j, _ in configs), eng)
    rec = {"what": f"verify_properties (all J jobs in flight, segments = J) vs the same jobs one after the other through branch_and_bound_frontier, {NET}, "
                   f"eps {EPS}, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, max_rounds {args.rounds}, {args.capacity} slots per job; host wall clock, every "
                   "round synchronised by its read of the record(s); per side the median and the spread (max - min) over the repeats, the sides alternating",
           "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "repeats": args.repeats, "configs": [], "last_round_kernels": []}
    for J, K in configs:
        sub = lps[:J]
        sequential(sub[:1], choice, K, 2, args.capacity)              # warm-up: allocations, first launches at these shapes
        together(sub, choice, K, 2, args.capacity)
        a_runs, b_runs = [], []
        for _ in range(args.repeats):
            a, a_res = sequential(sub, choice, K, args.rounds, args.capacity)
            b, b_res = together(sub, choice, K, args.rounds, args.capacity)
            assert a_res == b_res, "a job's result in the many-job run differs from its result alone"
            a_runs.append(a)
            b_runs.append(b)
        domains = sum(r[3] for r in a_res) - J                        # (the roots are outside the round spans)
        row = {"J": J, "K": K, "domains_bounded_in_rounds": domains, "stop_reasons": sorted({r[4] for r in a_res}),
               "one_after_the_other": summary(a_runs, J, domains), "together": summary(b_runs, J, domains)}
        for key in ("wall_seconds", "round_span_seconds"):
            a, b = row["one_after_the_other"][key], row["together"][key]
            noise = 3 * max(a["spread"], b["spread"])
            row[key + "_ratio"] = round(a["median"] / b["median"], 3)
            row[key + "_verdict"] = "together ahead" if a["median"] - b["median"] > noise else ("together behind" if b["median"] - a["median"] > noise else "no difference beyond 3x the spread")
        rec["configs"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    for J, K in [(j, k) for j, k in configs if (j, k) in ((16, 16), (64, 16))]:
        rec["last_round_kernels"].append(last_round_kernels(eng, lps[:J], choice, K, args.rounds, args.capacity))
        print(json.dumps(rec["last_round_kernels"][-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
