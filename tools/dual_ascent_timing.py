#!/usr/bin/env python
"""Dual ascent on the subproblem LPs on the device (gnnb_dual_ascent) against HiGHS and against its host twin (GPU box).

Per network (base, wide, deep; seeded N(0,1) image, RandomState(4), property 3 vs 5) on five domains -- the root and the median ambiguous
node of the first and of the last ReLU layer split both ways: HiGHS ms per LP (LayerGraphLP._solve_lp on the same Wong-Kolter bounds), the
host twin's ms per domain (LayerGraphLP.dual_ascent_host at 16 torch threads), the device's ms per call and per domain at each batch size
(the five domains repeated to B rows; HIP events around ScorerEngine.dual_ascent on device-resident inputs, after warm-up) for 20 and 100
iterations, the fraction of the gap (LP optimum - iteration 0) each closes, whether any bound exceeds its LP optimum by more than 1e-6, and
whether GraphChoice.decision picks the same node on the device-produced inputs as on HiGHS' (recorded, not a requirement: LP duals are
not unique, and the GNN was trained on Gurobi's vertices).

    python tools/dual_ascent_timing.py [--out profiles/dual_ascent_timing.json] [--batches 1,2,16,64,256] [--nets cifar_base_kw,...]
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import lp_producer, nets                      # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice       # noqa: E402

EPS = {"cifar_base_kw": 0.09, "cifar_wide_kw": 0.05, "cifar_deep_kw": 0.05}
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
ITERS = (20, 100)
LR = 0.1


def domains(lp):
    """[(name, mask, parent bounds, split layer)]: the root and four children."""
    root = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
    rb = lp.kw_bounds(root)
    out = [("root", root, None, None)]
    for r in sorted({0, len(root) - 1}):
        i = lp.pre_relu_indices[r]
        amb = torch.nonzero((rb[0][i].reshape(-1) < 0) & (rb[1][i].reshape(-1) > 0)).reshape(-1)
        node = int(amb[len(amb) // 2])
        for choice, what in ((0, "blocked"), (1, "passing")):
            m = [t.clone() for t in root]
            m[r][node] = choice
            out.append((f"layer {r} node {node} {what}", m, rb, r))
    return out


def device_ms(eng, args, n_iter, reps):
    for _ in range(2):
        eng.dual_ascent(*args, n_iter, LR)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.dual_ascent(*args, n_iter, LR)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def one_net(name, choice, batches):
    eng = choice.model.engine()
    layers = nets.load_verified_net(name, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp = lp_producer.LayerGraphLP(layers, x - EPS[name], x + EPS[name], bounds="kw_device", engine=eng)
    doms = domains(lp)
    items = [(m, p, s) for _, m, p, s in doms]
    bounds, kw, (fixed, prop, x_lo, x_hi, masks) = lp._kw_device(items)
    n = len(doms)
    rows = []
    for (dname, mask, _, _), (lbs, ubs) in zip(doms, bounds):
        t0 = time.perf_counter()
        sub = lp._solve_lp([t.clone() for t in mask], lbs, ubs)
        highs_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        twin = lp.dual_ascent_host((lbs, ubs), mask, ITERS[-1], lr=LR)
        twin_ms = 1e3 * (time.perf_counter() - t0)
        rows.append({"domain": dname, "lp_optimum": sub.lb, "highs_ms": round(highs_ms, 1), "twin_ms_100_iterations": round(twin_ms, 1),
                     "iteration_0": twin.values[0], "twin_20": max(twin.values[:ITERS[0] + 1]), "twin_100": twin.bound, "_sub": sub})
        print(f"{name} {dname}: LP {sub.lb:.6f} in {highs_ms:.0f} ms; twin {twin.values[0]:.6f} -> {twin.bound:.6f} in {twin_ms:.0f} ms", flush=True)
    # the device on the same five domains: bounds, gap closed, the scorer's decision on its inputs against HiGHS'
    fixed_dict = {"fixed_layers": list(layers[:-1]), "prop_layers": [layers[-1]]}
    score = lp_producer.gnn_scorer(choice, lp)
    for n_iter in ITERS:
        subs = lp.solve_many([(m, None if p is None else rows[0]["_sub"], s) for _, m, p, s in doms], lp="dual_device", n_iter=n_iter, lr=LR)
        for row, sub in zip(rows, subs):
            gap = row["lp_optimum"] - row["iteration_0"]
            row[f"device_{n_iter}"] = sub.lb
            row[f"gap_closed_{n_iter}"] = round((sub.lb - row["iteration_0"]) / gap, 5) if gap > 0 else None
            row[f"device_above_lp_{n_iter}"] = bool(sub.lb > row["lp_optimum"] + 1e-6)
            row[f"same_decision_as_highs_{n_iter}"] = bool(score(sub, fixed_dict) == score(row["_sub"], fixed_dict))
    for row in rows:
        del row["_sub"]
        print(name, row, flush=True)
    timing = []
    for B in batches:
        idx = torch.arange(B) % n
        args = (fixed, [prop[0]] * B, x_lo[idx].contiguous().to(eng.device), x_hi[idx].contiguous().to(eng.device), masks[idx].to(eng.device),
                [t[idx.to(t.device)].contiguous() for t in kw.lb], [t[idx.to(t.device)].contiguous() for t in kw.ub])
        rec = {"B": B}
        for n_iter in ITERS:
            ms = device_ms(eng, args, n_iter, reps=5 if B <= 16 else 3)
            rec[f"device_ms_per_call_{n_iter}"] = round(ms, 4)
            rec[f"device_ms_per_domain_{n_iter}"] = round(ms / B, 5)
        timing.append(rec)
        print(name, rec, flush=True)
    highs = float(np.mean([r["highs_ms"] for r in rows]))
    twin = float(np.mean([r["twin_ms_100_iterations"] for r in rows]))
    b64 = next((r for r in timing if r["B"] == 64), None)
    return {"eps": EPS[name], "domains": rows, "batches": timing, "highs_ms_per_lp": round(highs, 1), "twin_ms_per_domain_100_iterations": round(twin, 1),
            "host_threads": torch.get_num_threads(),
            "B64_100_iterations_highs_over_device": None if b64 is None else round(highs / b64["device_ms_per_domain_100"], 1),
            "B64_100_iterations_twin_over_device": None if b64 is None else round(twin / b64["device_ms_per_domain_100"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_ascent_timing.json"))
    ap.add_argument("--batches", default="1,2,16,64,256")
    ap.add_argument("--nets", default="cifar_base_kw,cifar_wide_kw,cifar_deep_kw")
    args = ap.parse_args()
    torch.set_num_threads(16)
    rec = {"what": "gnnb_dual_ascent (fp64, HIP, projected Adam lr 0.1) vs HiGHS (LayerGraphLP._solve_lp) and vs LayerGraphLP.dual_ascent_host "
                   "(torch fp64): the root and four children per network, property 3 vs 5, seeded image, the same Wong-Kolter bounds",
           "device": torch.cuda.get_device_name(), "host": platform.processor() or platform.machine(), "nets": {}}
    for name in args.nets.split(","):
        layers = nets.load_verified_net(name, 3, 5)
        lp = lp_producer.LayerGraphLP(layers, torch.zeros(3, 32, 32), torch.zeros(3, 32, 32))
        choice = GraphChoice([torch.zeros(int(np.prod(lp.shapes[i + 1]))) for i in lp.pre_relu_indices], CKPT)
        choice.verbose = False
        rec["nets"][name] = one_net(name, choice, [int(b) for b in args.batches.split(",")])
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
