#!/usr/bin/env python
"""The imitation step, timed (GPU box).

(a) The step.  cifar_base_kw, a seeded synthetic batch of 16 subproblems on the device (synth.make_batch, seed 31), the shipped checkpoint,
    lr = wd = 1e-4.  Per n in --rows (the first n rows) and table width M in --widths ("all": every undecided node of a row; improvements
    uniform in [0, 1], seeded): ms per ``gnnb_imitation_step_rows`` call beside ``gnnb_online_step_rows`` on the same rows (KW node: the
    middle undecided node of each row, improvement 0.1).  Both calls synchronise, so a call is timed on the host from an idle stream.  Same
    session, one warm-up call per side, then --repeats repeats with the sides alternating, each the mean of --calls calls; the online
    side's own max - min over its repeats is the spread the difference is held against.  Only the loss kernel, the dense fscore reduction,
    the fp64 chunk reduce and the gathered table row differ between the two: ``gnnb_imitation_loss`` alone on (n, R) arrays is timed with
    HIP events, and k_trows_gather's ms per launch on both sides comes from gnnb_profile_read (a run of its own).

(b) Inside a run.  tools/frontier_timing.py's problem (eps 0.09, seeded N(0,1) image, property 3 vs 5, n_iter 20, lr 0.1, BaB eps 1e-4):
    per K in --ks and branching in ("gnn", "strong") with strong_candidates = 16, ``branch_and_bound_frontier`` with ``imitate`` off and
    ``imitate=1`` over the same number of rounds, wall ms per round (every round ends with the read of the state record, a learning round
    with its step behind it), global_lb and the gap after those rounds, and -- from a traced run of its own -- the mean regret per round.
    In "gnn" mode the off side computes no table at all, so its difference is the table's cost plus the step's.  Every run starts from
    the checkpoint's parameters and a fresh optimizer.

    python tools/imitation_timing.py [--out profiles/imitation_timing.json] [--rows 1,4,16] [--widths 16,all] [--ks 1,16] [--rounds 6]
"""
import argparse
import datetime
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import _lib, lp_producer, nets, synth                  # noqa: E402
from gnn_branching_amd.engine import make_batch                               # noqa: E402
from gnn_branching_amd.frontier import branch_and_bound_frontier              # noqa: E402
from gnn_branching_amd.graphnet.graph_score_online import GraphChoice         # noqa: E402
from tools.frontier_online_timing import CKPT, EPS, EPS_BAB, LR, N_ITER, NET, reset, spread      # noqa: E402

BATCH, CANDIDATES = 16, 16


def seeded_table(masks, M, seed):
    g = np.random.RandomState(seed)
    tab = np.full(masks.shape, float("nan"))
    for b in range(masks.shape[0]):
        idx = np.flatnonzero(masks[b])
        if M is not None:
            idx = np.sort(g.choice(idx, size=min(M, idx.size), replace=False))
        tab[b, idx] = g.uniform(0.0, 1.0, idx.size)
    return tab


def step_timing(choice, w0, rows_list, widths, repeats, calls):
    eng, dev = choice._eng(), choice._eng().device
    batch = synth.make_batch(NET, BATCH, seed=31)
    m = eng._marshal(*batch.forward_args())
    cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
    masks = batch.masks.numpy()
    kw = torch.tensor([int(np.flatnonzero(r)[np.count_nonzero(r) // 2]) for r in masks], dtype=torch.int32).to(dev)
    imp = torch.full((BATCH,), 0.1, dtype=torch.float32, device=dev)
    out = []
    for n in rows_list:
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        for width in widths:
            M = None if width == "all" else int(width)
            table = torch.from_numpy(seeded_table(masks, M, 7)).to(dev)
            report = torch.zeros(n, 4, dtype=torch.int32, device=dev)
            sides = {"online": lambda: eng.online_step_rows(cb, BATCH, rows, kw[:n], imp[:n]),
                     "imitation": lambda: eng.imitation_step_rows(cb, BATCH, rows, table, 1.0, report=report)}
            ms = {k: [] for k in sides}
            reset(choice, w0)
            for f in sides.values():
                f()
            for _ in range(repeats):
                for k, f in sides.items():                        # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        f()
                    ms[k].append(1e3 * (time.perf_counter() - t0) / calls)
            # the loss kernel alone, and the gather on both sides
            sc, mk = torch.zeros(n, eng.R, device=dev), m.mask.view(BATCH, eng.R)[:n].contiguous()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eng.imitation_loss(sc, mk, table[:n].contiguous(), 1.0)
            a.record()
            for _ in range(20):
                eng.imitation_loss(sc, mk, table[:n].contiguous(), 1.0)
            b.record()
            torch.cuda.synchronize()
            gather = {}
            eng.profile_enable(1)
            try:
                for k, f in sides.items():
                    eng.profile_read(reset=True)
                    for _ in range(5):
                        f()
                    ms_total, launches = eng.profile_read(reset=True)["k_trows_gather"]
                    gather[k] = round(ms_total / launches, 5)
            finally:
                eng.profile_enable(0)
            on, im = spread(ms["online"]), spread(ms["imitation"])
            sp = on["max"] - on["min"]
            entry = {"n": n, "table_width": width, "violators_per_row": report[:, 3].cpu().tolist(), "ms_online_step_rows": on, "ms_imitation_step_rows": im,
                     "difference_ms": round(im["median"] - on["median"], 4), "online_spread_ms": round(sp, 4),
                     "exceeds_three_spreads": im["median"] - on["median"] > 3 * sp,
                     "ms_gnnb_imitation_loss_call_with_its_output_allocations": round(a.elapsed_time(b) / 20, 5), "ms_k_trows_gather_per_launch": gather}
            out.append(entry)
            print(json.dumps(entry), flush=True)
    reset(choice, w0)
    return out


def one_run(lp, choice, w0, K, rounds, branching, imitate, trace=None):
    reset(choice, w0)
    stamps, stats = [], {}
    extra = {"strong_candidates": CANDIDATES} if (branching == "strong" or imitate) else {}
    if imitate:
        extra["imitate"] = imitate
    glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=8192,
                                                                log=lambda s: stamps.append(time.perf_counter()), stats=stats, trace=trace, branching=branching,
                                                                **extra)
    return {"ms_per_round": 1e3 * (stamps[-1] - stamps[0]) / max(done, 1), "rounds": done, "global_lb": glb, "global_ub": gub, "gap": gub - glb, "stop": reason,
            "imitation_steps": stats.get("imitation_steps", 0), "imitation_rows": stats.get("imitation_rows", 0)}


def run_timing(lp, choice, w0, ks, rounds, repeats):
    out = []
    for K in ks:
        for branching in ("gnn", "strong"):
            sides = {"off": None, "imitate_1": 1}
            for im in sides.values():
                one_run(lp, choice, w0, K, min(rounds, 3), branching, im)
            runs = {k: [] for k in sides}
            for _ in range(repeats):
                for k, im in sides.items():
                    runs[k].append(one_run(lp, choice, w0, K, rounds, branching, im))
            trace = []
            one_run(lp, choice, w0, K, rounds, branching, 1, trace=trace)
            regret = [statistics.mean(v for v in t["imitation_regret"] if not math.isnan(v)) if any(not math.isnan(v) for v in t.get("imitation_regret", [])) else None
                      for t in trace]
            entry = {"K": K, "branching": branching, "strong_candidates": CANDIDATES, "max_rounds": rounds, "mean_regret_per_round": regret,
                     "mean_violators_per_row_per_round": [statistics.mean(r[3] for r in t["imitation_report"]) if t.get("imitation_report") else None for t in trace]}
            for k in sides:
                last = runs[k][-1]
                entry[k] = {"ms_per_round": spread([r["ms_per_round"] for r in runs[k]]), **{q: last[q] for q in ("rounds", "global_lb", "global_ub", "gap", "stop",
                                                                                                                 "imitation_steps", "imitation_rows")}}
            out.append(entry)
            print(json.dumps(entry), flush=True)
    reset(choice, w0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imitation_timing.json"))
    ap.add_argument("--rows", default="1,4,16")
    ap.add_argument("--widths", default="16,all")
    ap.add_argument("--ks", default="1,16")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="calls per repeat of the step timing")
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
    rec = {"what": f"gnnb_imitation_step_rows beside gnnb_online_step_rows on {NET} (wall ms per call from an idle stream, {args.repeats} repeats of {args.calls} calls, "
                   f"the sides alternating), and branch_and_bound_frontier with imitate off / imitate=1 on eps {EPS}, property 3 vs 5, n_iter {N_ITER}, lr {LR}, "
                   f"BaB eps {EPS_BAB}, strong_candidates {CANDIDATES}: one image, N(0,1) boxes; a direction, not a rate",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "relu_nodes": eng.R,
           "step": [], "run": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    rec["step"] = step_timing(choice, w0, [int(v) for v in args.rows.split(",")], args.widths.split(","), args.repeats, args.calls)
    write()
    rec["run"] = run_timing(lp, choice, w0, [int(v) for v in args.ks.split(",")], args.rounds, args.repeats)
    write()
    print("written", args.out)


if __name__ == "__main__":
    main()
