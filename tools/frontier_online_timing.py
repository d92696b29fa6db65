#!/usr/bin/env python
"""Learning online inside the device-resident frontier, timed (GPU box).

cifar_base_kw, eps 0.09, seeded N(0,1) image (RandomState(4)), property 3 vs 5, n_iter 20, lr 0.1, eps_bab 1e-4, no decision bound: the
set-up of tools/frontier_threshold_timing.py (section 7.5).  Per K in --ks, at a fixed max_rounds: branch_and_bound_frontier with
branching_threshold=--threshold and online_threshold=None ("off": the parent commit's threshold run) and =--online ("on"), one warm-up run
each, then --repeats timed runs each with the sides alternating; wall time between the root's log line and the last round's (every round
ends with the host's read of the state record, an online round with its learning step behind it).  A run that learns changes the GNN's
parameters and its optimizer, so every run starts from the checkpoint's parameters and a fresh optimizer.

(a) "off" against the committed profiles/frontier_threshold_timing.json (the parent commit's figures for the same K, rounds and threshold):
    the spread of that file's own repeats, (max - min) / median, is the yardstick it is held to; bounds and counts must be identical.
(b) "on": ms per round, learning rounds, rows per step, the wall ms of gnnb_online_step_rows per n that occurred and the ms per launch of
    k_frontier_learn / k_trows_gather from gnnb_profile_enable (both in a run of their own), and the gap after the same number of rounds.
    The online mode also drops the table of inefficient KW points, so a third side, "control" (online_threshold=None,
    kwbd_threshold=2**31-1: every KW decision bounded, nothing learnt), says which part of a difference is the learning's.

    python tools/frontier_online_timing.py [--out profiles/frontier_online_timing.json] [--ks 1,16,64] [--rounds 60,40,30] [--threshold 0.2] [--online 5]
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
from gnn_branching_amd import _lib, lp_producer, nets                        # noqa: E402
from gnn_branching_amd.frontier import branch_and_bound_frontier             # noqa: E402
from gnn_branching_amd.graphnet.graph_score_online import GraphChoice        # noqa: E402

NET, EPS, N_ITER, LR, EPS_BAB = "cifar_base_kw", 0.09, 20, 0.1, 1e-4
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
NEW_KERNELS = ("k_frontier_learn", "k_trows_gather")


def reset(choice, w0):
    """The checkpoint's parameters on the device and in the module, and a fresh optimizer."""
    eng = choice._eng()
    eng.set_weights(w0)
    eng.online_create(choice.lr, choice.wd)
    choice.model.load_blob(w0)


KWBD_NEVER = 2 ** 31 - 1


def one_run(lp, choice, w0, K, rounds, capacity, threshold, online, kwbd=None):
    reset(choice, w0)
    more = {} if kwbd is None else {"kwbd_threshold": kwbd}
    stamps, stats = [], {}
    glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                                                capacity=capacity, log=lambda s: stamps.append(time.perf_counter()),
                                                                branching_threshold=threshold, stats=stats, online_threshold=online, **more)
    wall = stamps[-1] - stamps[0]
    return {"seconds": wall, "rounds": done, "domains_bounded": bounded - 1, "stop": reason, "global_lb": glb, "global_ub": gub, "stats": stats}


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def summary(runs):
    last = runs[-1]
    out = {"ms_per_round": spread([1e3 * r["seconds"] / max(r["rounds"], 1) for r in runs]),
           "rounds": last["rounds"], "domains_bounded": last["domains_bounded"], "stop": last["stop"], "global_lb": last["global_lb"],
           "global_ub": last["global_ub"], "gap": last["global_ub"] - last["global_lb"],
           "same_result_in_every_repeat": all((r["global_lb"], r["global_ub"], r["domains_bounded"]) == (last["global_lb"], last["global_ub"], last["domains_bounded"])
                                              for r in runs)}
    st = last["stats"]
    out.update(parents_expanded=st["branches"], kw_pairs_bounded=st["kw_bounded"], kw_pairs_used=st["kw_used"])
    if "online_steps" in st:
        out.update(learning_rounds=st["online_steps"], learn_rows=st["online_rows"],
                   rows_per_step=round(st["online_rows"] / st["online_steps"], 3) if st["online_steps"] else None)
    return out


def profiled(lp, choice, w0, eng, K, rounds, capacity, threshold, online):
    """A run of its own: the wall ms of every gnnb_online_step_rows call by its n (the stream is idle when it starts: the read of n_learn
    has just synchronised it; it returns synchronised), and the ms per launch of the new kernels (HIP events around every launch)."""
    steps, inner = {}, eng.online_step_rows

    def timed(batch, Kb, rows, *a, **kw):
        t0 = time.perf_counter()
        inner(batch, Kb, rows, *a, **kw)
        steps.setdefault(int(rows.numel()), []).append(1e3 * (time.perf_counter() - t0))
    eng.online_step_rows = timed
    try:
        one_run(lp, choice, w0, K, rounds, capacity, threshold, online)
    finally:
        del eng.online_step_rows
    out = {"ms_of_gnnb_online_step_rows_by_n": {str(n): {"calls": len(v), **spread(v)} for n, v in sorted(steps.items())}}
    eng.profile_enable(1)
    try:
        eng.profile_read(reset=True)
        one_run(lp, choice, w0, K, rounds, capacity, threshold, online)
        prof = eng.profile_read(reset=True)
    finally:
        eng.profile_enable(0)
    out.update({k: {"launches": int(prof[k][1]), "ms_per_launch": round(prof[k][0] / prof[k][1], 5) if prof[k][1] else None} for k in NEW_KERNELS})
    return out


def parent_figures(threshold):
    """Per K the parent commit's threshold run ("on" of profiles/frontier_threshold_timing.json) and the spread of its own repeats."""
    try:
        with open(os.path.join(ROOT, "profiles", "frontier_threshold_timing.json")) as f:
            prev = json.load(f)
        if prev.get("branching_threshold") != threshold:
            return {}
        out = {}
        for r in prev["frontier"]:
            on = r["on"]
            out[r["K"]] = {"max_rounds": r["max_rounds"], "ms_per_round": on["ms_per_round"], "rounds": on["rounds"], "domains_bounded": on["domains_bounded"],
                           "global_lb": on["global_lb"], "global_ub": on["global_ub"], "kw_pairs_bounded": on.get("kw_pairs_bounded"),
                           "kw_pairs_used": on.get("kw_pairs_used"),
                           "spread_of_its_repeats": round((on["ms_per_round"]["max"] - on["ms_per_round"]["min"]) / on["ms_per_round"]["median"], 4)}
        out["library_build_id"] = prev.get("library_build_id")
        return out
    except (OSError, KeyError, ValueError):
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_online_timing.json"))
    ap.add_argument("--ks", default="1,16,64")
    ap.add_argument("--rounds", default="60,40,30")
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--online", type=int, default=5, help="online_threshold of the 'on' side (the reference's default)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=8192, help="slots of the pool")
    args = ap.parse_args()
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice._eng()
    w0 = eng.get_weights().copy()
    lp = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng)
    eng.bind(list(layers[:-1]), (3, 32, 32))
    parent = parent_figures(args.threshold)
    rec = {"what": f"branch_and_bound_frontier(branching_threshold={args.threshold}) with online_threshold=None (off) and {args.online} (on) on {NET}, eps {EPS}, "
                   f"property 3 vs 5, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, GraphChoice lr {choice.lr} wd {choice.wd}; wall clock on the host, every "
                   f"round synchronised by its state read; one warm-up run per side, then {args.repeats} repeats per side, the sides alternating; median and "
                   f"min / max over the repeats; every run from the checkpoint's parameters and a fresh optimizer",
           "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "pool_capacity": args.capacity,
           "branching_threshold": args.threshold, "online_threshold": args.online, "frontier": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for K, rounds in zip([int(k) for k in args.ks.split(",")], [int(r) for r in args.rounds.split(",")]):
        sides = {"off": (None, None), "on": (args.online, None), "control": (None, KWBD_NEVER)}
        for online, kwbd in sides.values():                       # warm-up: allocations, first launches, the trainer's arena
            one_run(lp, choice, w0, K, min(rounds, 4), args.capacity, args.threshold, online, kwbd)
        runs = {side: [] for side in sides}
        for _ in range(args.repeats):
            for side, (online, kwbd) in sides.items():            # alternating
                runs[side].append(one_run(lp, choice, w0, K, rounds, args.capacity, args.threshold, online, kwbd))
        entry = {"K": K, "max_rounds": rounds, "off": summary(runs["off"]), "on": summary(runs["on"]),
                 "control_every_kw_decision_bounded_nothing_learnt": summary(runs["control"]),
                 "parent_commit_threshold_timing": parent.get(K), "parent_commit_library_build_id": parent.get("library_build_id"),
                 "on_in_runs_of_their_own": profiled(lp, choice, w0, eng, K, rounds, args.capacity, args.threshold, args.online)}
        p = parent.get(K)
        if p and p["max_rounds"] == rounds:
            off = entry["off"]
            entry["off_against_parent"] = {
                "ms_per_round_ratio": round(off["ms_per_round"]["median"] / p["ms_per_round"]["median"], 4),
                "parent_spread_of_its_repeats": p["spread_of_its_repeats"],
                "inside_the_parent_spread": abs(off["ms_per_round"]["median"] / p["ms_per_round"]["median"] - 1) <= p["spread_of_its_repeats"],
                "bounds_and_counts_identical": (off["global_lb"], off["global_ub"], off["domains_bounded"], off["rounds"], off["kw_pairs_bounded"], off["kw_pairs_used"]) ==
                                               (p["global_lb"], p["global_ub"], p["domains_bounded"], p["rounds"], p["kw_pairs_bounded"], p["kw_pairs_used"])}
        entry["on_over_off_ms_per_round"] = round(entry["on"]["ms_per_round"]["median"] / entry["off"]["ms_per_round"]["median"], 3)
        entry["gap_off_control_on"] = [entry["off"]["gap"], entry["control_every_kw_decision_bounded_nothing_learnt"]["gap"], entry["on"]["gap"]]
        rec["frontier"].append(entry)
        print(json.dumps(entry), flush=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    reset(choice, w0)
    print("written", args.out)


if __name__ == "__main__":
    main()
