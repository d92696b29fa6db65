#!/usr/bin/env python
"""What tightened intermediate bounds cost and what they buy, on the GPU box.  Recorded, nothing asserted.

1. Roots.  Per network (base, wide, deep; section 7.1's boxes: the seeded N(0,1) image of RandomState(4), property 3 vs 5, eps 0.09 /
   0.05 / 0.05): device ms per root (B = 1, HIP events, median of --reps calls after two untimed ones) for gnnb_kw_bounds and for
   gnnb_kw_tighten at n_iter 5 and 20; the counts (nodes the ascent ran for, nodes it decided); the ambiguous nodes left; the bytes of the
   tighten workspace; and the root's 20-iteration gnnb_dual_ascent bound on each set of bounds.
2. Frontier.  The cifar_base_kw problems of tools/frontier_branching_compare.py (eps 0.03 with decision bound 0 and without one, eps 0.09
   with decision bound 0; seeds 0..3) and its toy_kw problem, ``branching="gnn"``, with tighten_root 0 / 5 / 20: rounds, branches, domains
   bounded, stop reason, final bounds, and wall-clock seconds from before the root to the verdict (after one untimed short run of the same
   setting).  Every figure stands next to the tighten_root = 0 run of the same problem on the same library build.

    python tools/kw_tighten_timing.py [--out profiles/kw_tighten_timing.json] [--ks 16] [--rounds 40] [--seeds 0,1,2,3] [--reps 5] [--skip-frontier]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gnn_branching_amd import _lib, frontier, lp_producer, nets      # noqa: E402
from gnn_branching_amd.engine import ScorerEngine                    # noqa: E402
import frontier_branching_compare as compare                         # noqa: E402

EPS = {"cifar_base_kw": 0.09, "cifar_wide_kw": 0.05, "cifar_deep_kw": 0.05}      # tools/kw_bounds_timing.py's
TIGHTEN = (0, 5, 20)
N_ITER, LR, EPS_BAB = compare.N_ITER, compare.LR, compare.EPS_BAB


def timed_ms(call, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def roots(eng, reps):
    out = {}
    for name, eps in EPS.items():
        layers = nets.load_verified_net(name, 3, 5)
        x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
        lp = lp_producer.LayerGraphLP(layers, x - eps, x + eps, bounds="kw_device", engine=eng)
        dev = eng.device
        R = sum(int(np.prod(lp.shapes[i + 1])) for i in lp.pre_relu_indices)
        args = (lp.layers[:-1], [lp.layers[-1]], lp.input_lb[None].contiguous().to(dev), lp.input_ub[None].contiguous().to(dev),
                torch.full((1, R), -1, dtype=torch.int8, device=dev))
        rows = {}
        for n in TIGHTEN:
            ms, res = timed_ms(lambda: eng.kw_bounds(*args, tighten=n), reps)
            da = eng.dual_ascent(*args, res.lb, res.ub, N_ITER, LR)
            amb = sum(int(((lo < 0) & (up > 0)).sum()) for lo, up in zip(res.lb[:-1], res.ub[:-1]))
            rows[str(n)] = {"device_ms_per_root": round(ms, 4), "counts": res.counts.cpu().tolist()[0] if n else None, "ambiguous_nodes": amb,
                            "root_bound_20_iterations": float(da.bound.cpu()[0]), "infeasible": int(res.infeasible.cpu()[0])}
            print(f"{name} tighten {n}: {ms:.3f} ms/root, counts {rows[str(n)]['counts']}, ambiguous {amb}, bound {rows[str(n)]['root_bound_20_iterations']:.6f}",
                  flush=True)
        out[name] = {"eps": eps, "relu_nodes": R, "tighten_workspace_bytes_B1": int(eng.lib.gnnb_kw_tighten_workspace_bytes(eng.h, 1)),
                     "kw_workspace_bytes_B1": int(eng.lib.gnnb_kw_workspace_bytes(eng.h, 1)), "n_iter": rows}
    return out


def one_run(lp, choice, K, rounds, decision_bound):
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    glb, gub, done, bounded, reason = frontier.branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                                                          decision_bound=decision_bound, log=lambda s: None, stats=stats)
    torch.cuda.synchronize()
    return {"rounds": done, "branches": stats.get("branches"), "domains_bounded": bounded, "stop": reason, "global_lb": glb, "global_ub": gub,
            "wall_s": round(time.perf_counter() - t0, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kw_tighten_timing.json"))
    ap.add_argument("--ks", default="16")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--seeds", default="0,1,2,3")
    ap.add_argument("--hard-eps", type=float, default=0.09)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-frontier", action="store_true")
    ap.add_argument("--budget-s", type=float, default=None, help="start no further frontier problem after this many seconds (recorded as 'left_out')")
    args = ap.parse_args()
    torch.set_num_threads(16)
    rec = {"what": f"gnnb_kw_tighten against gnnb_kw_bounds: device ms per root (B = 1, median of {args.reps}), counts and the root's {N_ITER}-iteration "
                   f"dual bound; branch_and_bound_frontier (gnn, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, at most {args.rounds} rounds) with "
                   f"tighten_root {TIGHTEN}: branches and wall-clock from before the root to the verdict",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    t_start = time.perf_counter()
    rec["roots"] = roots(ScorerEngine(None), args.reps)
    write()
    if not args.skip_frontier:
        for name, lp, choice, bounds in compare.problems([int(s) for s in args.seeds.split(",")], args.hard_eps):
            for db in bounds:
                if args.budget_s is not None and time.perf_counter() - t_start > args.budget_s:
                    rec.setdefault("left_out", []).append({"problem": name, "decision_bound": db, "why": f"--budget-s {args.budget_s} was spent"})
                    write()
                    continue
                for K in (int(k) for k in args.ks.split(",")):
                    entry = {"problem": name, "decision_bound": db, "K": K}
                    for n in TIGHTEN:
                        lp.tighten_root = n
                        one_run(lp, choice, K, min(args.rounds, 3), db)      # warm-up: allocations, first launches of every shape
                        entry[f"tighten_root_{n}"] = one_run(lp, choice, K, args.rounds, db)
                    lp.tighten_root = 0
                    rec["runs"].append(entry)
                    print(json.dumps(entry), flush=True)
                    write()
    print("written", args.out)


if __name__ == "__main__":
    main()
