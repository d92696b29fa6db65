#!/usr/bin/env python
"""Wong-Kolter intermediate bounds on the device (gnnb_kw_bounds) against the host's fp64 LayerGraphLP.kw_bounds (GPU box).

Per network (base, wide, deep; seeded N(0,1) image, RandomState(4), property 3 vs 5) and batch size B: device ms per call and per domain
(HIP events around ScorerEngine.kw_bounds on device-resident inputs, after warm-up), the host kw_bounds ms per domain at 16 torch threads,
and the max |device - host| over the root domain's whole bounds list.  Then one branch_and_bound_threshold run (base_easy row 0, as the
wall-clock record of DESIGN section 7 sets it up) with bounds="kw" and with "kw_device": LP ms, bounds ms, and whether the branching
decisions are equal.

    python tools/kw_bounds_timing.py [--out profiles/kw_bounds_timing.json] [--batches 1,2,4,16,64,256] [--no-bab]
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
from gnn_branching_amd.engine import ScorerEngine                    # noqa: E402

EPS = {"cifar_base_kw": 0.09, "cifar_wide_kw": 0.05, "cifar_deep_kw": 0.05}
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")


def root_mask(lp):
    return [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]


def device_ms(eng, lp, B, reps):
    """ms per gnnb_kw_bounds call for B root domains, inputs already on the device."""
    dev = eng.device
    x_lo = lp.input_lb[None].expand((B,) + lp.shapes[0]).contiguous().to(dev)
    x_hi = lp.input_ub[None].expand((B,) + lp.shapes[0]).contiguous().to(dev)
    masks = torch.full((B, sum(int(np.prod(lp.shapes[i + 1])) for i in lp.pre_relu_indices)), -1, dtype=torch.int8, device=dev)
    fixed, prop = lp.layers[:-1], [lp.layers[-1]] * B
    for _ in range(2):
        eng.kw_bounds(fixed, prop, x_lo, x_hi, masks)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.kw_bounds(fixed, prop, x_lo, x_hi, masks)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def nets_table(eng, batches):
    out = {}
    for name in ("cifar_base_kw", "cifar_wide_kw", "cifar_deep_kw"):
        layers = nets.load_verified_net(name, 3, 5)
        x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
        lp = lp_producer.LayerGraphLP(layers, x - EPS[name], x + EPS[name], bounds="kw_device", engine=eng)
        mask = root_mask(lp)
        host = []
        for _ in range(3 if name != "cifar_deep_kw" else 2):
            t0 = time.perf_counter()
            want = lp.kw_bounds(mask)
            host.append(1e3 * (time.perf_counter() - t0))
        host_ms = float(min(host))
        got = lp.bounds(mask)
        err = max(float((g - w).abs().max()) for side in (0, 1) for g, w in zip(got[side], want[side]))
        rel = max(float((g - w).abs().max()) / max(1.0, float(w.abs().max())) for side in (0, 1) for g, w in zip(got[side], want[side]))
        rows = []
        for B in batches:
            ms = device_ms(eng, lp, B, reps=5 if B <= 16 else 3)
            rows.append({"B": B, "device_ms_per_call": round(ms, 4), "device_ms_per_domain": round(ms / B, 5),
                         "host_over_device_per_domain": round(host_ms / (ms / B), 1)})
            print(f"{name} B={B}: {ms:.3f} ms/call, {ms / B:.4f} ms/domain (host {host_ms:.1f} ms/domain)", flush=True)
        b64 = next((r for r in rows if r["B"] == 64), None)
        out[name] = {"eps": EPS[name], "host_kw_bounds_ms_per_domain": round(host_ms, 2), "host_threads": torch.get_num_threads(),
                     "max_abs_device_minus_host": err, "max_rel_device_minus_host": rel, "batches": rows,
                     "target_B64_device_le_host_over_200": None if b64 is None else bool(b64["device_ms_per_domain"] <= host_ms / 200)}
    return out


def bab_run():
    """branch_and_bound_threshold on base_easy row 0 (DESIGN section 7's set-up) with each bounds mode."""
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
    g = np.load(os.path.join(ROOT, "tests", "golden", "base_easy_props.npz"))
    row = 0
    table_eps, prop = float(g["Eps"][row]), int(g["prop"][row])
    x = torch.from_numpy(np.random.RandomState(100 + row).standard_normal((3, 32, 32)).astype(np.float32))
    with torch.no_grad():
        z = x[None]
        for l in nets.build_net("cifar_base_kw"):
            z = l(z)
    gt = int(z.argmax())
    cls = prop if prop != gt else (prop + 1) % 10
    layers = nets.load_verified_net("cifar_base_kw", gt, cls)
    eps = None
    for f in (1.0, 0.75, 0.55, 0.4, 0.3, 0.2):
        lp0 = lp_producer.LayerGraphLP(layers, x - f * table_eps, x + f * table_eps)
        root = lp0.solve(root_mask(lp0))
        if root is not None and root.lb < 0 < root.ub:
            eps = round(f * table_eps, 6)
            break
    out = {"row": row, "prop": prop, "eps": eps, "target_class": cls, "max_branches": 5}
    decisions = {}
    for mode in ("kw", "kw_device"):
        lp = lp_producer.LayerGraphLP(layers, x - eps, x + eps, bounds=mode)
        clock = {"bounds_ms": 0.0, "lp_ms": 0.0, "bounds_calls": 0, "lps": 0}

        def timed(fn, key, count):
            def f(*a, **k):
                t0 = time.perf_counter()
                r = fn(*a, **k)
                if mode == "kw_device" and key == "bounds_ms":
                    torch.cuda.synchronize()
                clock[key] += 1e3 * (time.perf_counter() - t0)
                clock[count] += 1
                return r
            return f
        if mode == "kw":
            lp.bounds = timed(lp.bounds, "bounds_ms", "bounds_calls")
        else:
            lp.kw_device_bounds = timed(lp.kw_device_bounds, "bounds_ms", "bounds_calls")
        lp._solve_lp = timed(lp._solve_lp, "lp_ms", "lps")
        choice = GraphChoice(root_mask(lp), CKPT)
        choice.verbose = False
        seq = []

        def gnn(sub, fixed):
            d = lp_producer.gnn_scorer(choice, lp)(sub, fixed)
            seq.append(("gnn", [int(v) for v in d]))
            return d

        def kw(sub, icp, order, sparsest):
            d, icp = choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, order, sparsest)
            seq.append(("kw", [int(v) for v in d]))
            return d, icp
        t0 = time.perf_counter()
        res = lp_producer.branch_and_bound_threshold(lp, gnn, kw, layers, max_branches=5, decision_bound=0.0, log=lambda s: None)
        clock["total_ms"] = 1e3 * (time.perf_counter() - t0)
        out[mode] = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in clock.items()}
        out[mode]["result"] = [float(res[0]), float(res[1])] + list(res[2:])
        decisions[mode] = seq
        print(mode, out[mode], flush=True)
    out["decisions"] = decisions["kw"]
    out["decisions_equal"] = decisions["kw"] == decisions["kw_device"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kw_bounds_timing.json"))
    ap.add_argument("--batches", default="1,2,4,16,64,256")
    ap.add_argument("--no-bab", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(16)
    eng = ScorerEngine(None)
    rec = {"what": "gnnb_kw_bounds (fp64, HIP) vs LayerGraphLP.kw_bounds (torch fp64, host): root domains, property 3 vs 5, seeded image",
           "device": torch.cuda.get_device_name(), "host": platform.processor() or platform.machine(),
           "nets": nets_table(eng, [int(b) for b in args.batches.split(",")])}
    if not args.no_bab:
        rec["bab_threshold_base_easy_row0"] = bab_run()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
