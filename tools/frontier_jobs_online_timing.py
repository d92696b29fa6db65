#!/usr/bin/env python
"""Online learning for every job of a many-job frontier (gnn_branching_amd/frontier.py verify_properties_online)
timed in one process (GPU box).

tools/frontier_jobs_threshold_timing.py's set-up: cifar_base_kw, that tool's property table (job j: the box of eps 0.09 around the seeded
N(0,1) stand-in image RandomState(100 + j), true class 3, the wrong class cycling over the other nine), n_iter 20, lr 0.1, eps_bab 1e-4, no
decision bound, --rounds rounds at most per job, --capacity slots per job, all J jobs in flight (segments = J), branching_threshold
--threshold (0.2).  One warm-up run per side, then --repeats repeats with the sides alternating; per side the median and (min - max).
EVERY run starts from the checkpoint's parameters and a fresh optimizer: a new graph_score_online.GraphChoice per run, made outside the
timed span.

  (a) the option changes nothing when off: ``verify_properties_threshold`` ms per round here, next to the same figure of the PARENT
      commit's library measured in the same session with the parent's own tools/frontier_jobs_threshold_timing.py; its JSON is handed over
      with --parent.  The margin is the parent's own repeat spread, (max - min) / median.
  (b) three sides at J x K = 16 x 16 and 64 x 4: ``verify_properties_threshold`` at its default kwbd_threshold; a control with
      kwbd_threshold = 2**31 - 1 and no learning; ``verify_properties_online`` at --online (5).  Per side ms per round, domains bounded,
      KW pairs bounded / won, learning rounds and rows per step, and per job global_lb and the gap after the same number of rounds.
  (c) the pool against the serial alternative: the same jobs one after the other through
      ``branch_and_bound_frontier(online_threshold=...)`` with ONE shared GraphChoice: wall clock and the learn rows the scorer saw.
  (d) the device time of the profile class k_frontier_learn under gnnb_profile_enable in an online pool run, which launches nothing
      else of that class: the class total is k_frontier_learn_jobs + k_frontier_learn_compact.

    python tools/frontier_jobs_online_timing.py [--out profiles/frontier_jobs_online_timing.json] [--rounds 8] [--capacity 129] [--repeats 3]
                                                [--threshold 0.2] [--online 5] [--configs 16x16,64x4] [--parent parent.json] [--skip-serial]
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
from gnn_branching_amd.frontier import (KWBD_NEVER, FrontierJob, branch_and_bound_frontier, verify_properties_online,      # noqa: E402
                                        verify_properties_threshold)
from gnn_branching_amd.graphnet.graph_score_online import GraphChoice      # noqa: E402
from tools.frontier_jobs_timing import CKPT, EPS, EPS_BAB, GT, LR, N_ITER, NET, make_lps      # noqa: E402

CONFIGS = [(16, 16), (64, 4)]                                           # (J, K)


def fresh_choice(lp0):
    """The checkpoint's parameters and a fresh optimizer."""
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    return choice


def pool(side, lps, K, rounds, capacity, threshold, online):
    """One pool run of ``side``: "threshold", "control" (kwbd_threshold 2**31 - 1, no learning) or "online"."""
    choice = fresh_choice(lps[0])
    stamps, stats, learned = [], [], {}

    def log(line):
        if " root " in line or " picked " in line:
            stamps.append(time.perf_counter())
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps]
    kw = dict(K=K, segments=len(jobs), capacity=capacity, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=log, stats=stats)
    t0 = time.perf_counter()
    if side == "online":
        results = verify_properties_online(choice, lps[0].layers[:-1], jobs, threshold, online, learned=learned, **kw)
    else:
        results = verify_properties_threshold(choice, lps[0].layers[:-1], jobs, threshold, **({"kwbd_threshold": KWBD_NEVER} if side == "control" else {}), **kw)
    return {"wall": time.perf_counter() - t0, "span": stamps[-1] - stamps[0], "rounds": max(r[2] for r in results), "results": results, "stats": stats,
            "learned": learned, "engine": choice._eng() if side == "online" else choice.model.engine()}


def serial(lps, K, rounds, capacity, threshold, online):
    """The jobs one after the other through the one-job online loop, ONE GraphChoice shared by all of them."""
    choice = fresh_choice(lps[0])
    t0, span, results, steps, rows = time.perf_counter(), 0.0, [], 0, 0
    for lp in lps:
        stamps, stats = [], {}
        results.append(branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=capacity,
                                                 log=lambda s: stamps.append(time.perf_counter()), branching_threshold=threshold, stats=stats,
                                                 online_threshold=online))
        span += stamps[-1] - stamps[0]
        steps, rows = steps + stats["online_steps"], rows + stats["online_rows"]
    return {"wall": time.perf_counter() - t0, "span": span, "rounds": sum(r[2] for r in results), "results": results, "online_steps": steps,
            "online_rows": rows}


def med(vals):
    return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}


def side_summary(runs):
    last = runs[-1]
    stats, learned = last["stats"], last["learned"]
    out = {"wall_seconds": med([r["wall"] for r in runs]), "ms_per_round": med([1e3 * r["span"] / max(r["rounds"], 1) for r in runs]),
           "rounds": last["rounds"], "domains_bounded": sum(r[3] for r in last["results"]), "kw_pairs_bounded": sum(s["kw_bounded"] for s in stats),
           "kw_pairs_won": sum(s["kw_used"] for s in stats), "stop_reasons": sorted({r[4] for r in last["results"]}),
           "global_lb": [round(r[0], 6) for r in last["results"]], "gap": [round(r[1] - r[0], 6) for r in last["results"]]}
    if learned:
        out.update(learning_rounds=learned["online_steps"], learn_rows=learned["online_rows"],
                   rows_per_step=round(learned["online_rows"] / max(learned["online_steps"], 1), 2), launched_rounds=learned["rounds"],
                   learn_rows_per_job=[s["online_rows"] for s in stats])
    return out


def learn_class_ms(lps, K, rounds, capacity, threshold, online):
    """(d): device ms of the class k_frontier_learn over an online pool run -- both new kernels and nothing else."""
    choice = fresh_choice(lps[0])
    eng = choice._eng()
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True)
        jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps]
        learned = {}
        verify_properties_online(choice, lps[0].layers[:-1], jobs, threshold, online, K=K, segments=len(jobs), capacity=capacity, n_iter=N_ITER, lr=LR,
                                 eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, learned=learned)
        per = eng.profile_read(reset=True)
    finally:
        eng.profile_enable(False)
    ms, launches = per["k_frontier_learn"]
    return {"J": len(lps), "K": K, "class": "k_frontier_learn", "what": "k_frontier_learn_jobs + k_frontier_learn_compact, the class total (they share it)",
            "launches": int(launches), "calls": int(launches) // 2, "device_ms_total": round(ms, 4), "device_us_per_call": round(1e3 * ms / max(launches // 2, 1), 2),
            "launched_rounds": learned["rounds"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_jobs_online_timing.json"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=129, help="slots per job, on every side")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--online", type=int, default=5)
    ap.add_argument("--configs", default=",".join(f"{j}x{k}" for j, k in CONFIGS), help="JxK,...")
    ap.add_argument("--parent", default=None, help="(a): the JSON the parent commit's tools/frontier_jobs_threshold_timing.py wrote in this session")
    ap.add_argument("--skip-serial", action="store_true", help="leave (c) out")
    args = ap.parse_args()
    torch.set_num_threads(16)
    T, N = args.threshold, args.online
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    layers = nets.load_verified_net(NET, GT, 5)
    x = torch.zeros(3, 32, 32)
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    lps = make_lps(max(j for j, _ in configs), fresh_choice(lp0).model.engine())
    rec = {"what": f"{NET}, eps {EPS}, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, max_rounds {args.rounds}, {args.capacity} slots per job, all J jobs "
                   f"in flight, branching_threshold {T}, online_threshold {N}; host wall clock, every round synchronised by its reads; one warm-up per "
                   "side, the sides alternating, median (min - max) over the repeats; every run from the checkpoint's parameters and a fresh optimizer",
           "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "repeats": args.repeats, "off": [], "sides": [], "serial": [],
           "kernels": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    parent = json.load(open(args.parent)) if args.parent else None
    for J, K in configs:
        sub = lps[:J]
        for side in ("threshold", "control", "online"):                  # warm-up: allocations, first launches at these shapes
            pool(side, sub, K, 2, args.capacity, T, N)
        runs = {"threshold": [], "control": [], "online": []}
        for _ in range(args.repeats):
            for side in runs:
                r = pool(side, sub, K, args.rounds, args.capacity, T, N)
                r.pop("engine")
                runs[side].append(r)
        row = {"J": J, "K": K, **{side: side_summary(rs) for side, rs in runs.items()}}
        rec["sides"].append(row)
        print(json.dumps(row), flush=True)
        # (a): the threshold pool here against the parent's own figure at the same J x K, if its JSON holds one
        here = row["threshold"]["ms_per_round"]
        off = {"J": J, "K": K, "ms_per_round_here": here, "parent": "not run"}
        for c in (parent or {}).get("configs", []):
            if (c["J"], c["K"]) == (J, K):
                p = c["together_threshold"]["ms_per_round"]
                off.update(parent={"library_build_id": parent["library_build_id"], "ms_per_round": p},
                           parent_repeat_spread=round(p["spread"] / p["median"], 4), here_over_parent=round(here["median"] / p["median"], 4))
        rec["off"].append(off)
        write()
        if not args.skip_serial:
            serial(sub[:1], K, 2, args.capacity, T, N)
            s_runs = [serial(sub, K, args.rounds, args.capacity, T, N) for _ in range(args.repeats)]
            online = row["online"]
            rec["serial"].append({"J": J, "K": K, "serial_wall_seconds": med([r["wall"] for r in s_runs]), "pool_wall_seconds": online["wall_seconds"],
                                  "wall_ratio_serial_over_pool": round(statistics.median(r["wall"] for r in s_runs) / online["wall_seconds"]["median"], 3),
                                  "serial_learning_steps": s_runs[-1]["online_steps"], "serial_learn_rows": s_runs[-1]["online_rows"],
                                  "pool_learning_steps": online["learning_rounds"], "pool_learn_rows": online["learn_rows"],
                                  "serial_global_lb": [round(r[0], 6) for r in s_runs[-1]["results"]]})
            print(json.dumps(rec["serial"][-1]), flush=True)
            write()
        rec["kernels"].append(learn_class_ms(sub, K, args.rounds, args.capacity, T, N))
        print(json.dumps(rec["kernels"][-1]), flush=True)
        write()
    print("written", args.out)


if __name__ == "__main__":
    main()
