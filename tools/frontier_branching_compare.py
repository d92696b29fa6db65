#!/usr/bin/env python
"""GNN branching against BaBSR branching and against strong branching, the GNN's teacher, inside the device-resident frontier (DESIGN.md
sections 7.10 and 7.11), on the same bounds, the same pick rule and the same K (GPU box).

Problems: toy_kw (the problem of tests/frontier_twin.py: property 2 vs 6 at eps 0.04) and cifar_base_kw, property 3 vs 5 at the demo's
default eps 0.03 on the seeded N(0,1) images of seeds 0..3 (examples/bab_demo.py --seed).  For each, at K = 1 and K = 16, with
decision_bound = 0, n_iter 20, lr 0.1, BaB eps 1e-4 and --rounds rounds at most: ``branching="gnn"`` against ``branching="babsr"`` and
against ``branching="strong"`` over the --candidates (16) undecided nodes of highest BaBSR score per parent.
Every one of those is decided at its root (no branch on either side), so two groups are run on top, marked "beyond_the_root": the same
problems with no decision bound (to the gap or --rounds), and cifar_base_kw at --hard-eps (0.09, the eps of tools/frontier_timing.py) on
the same seeds with decision_bound = 0.
Recorded per run: rounds, branches (parents expanded), domains bounded (strong: also the candidate children bounded), stop reason, final
lb / ub, and the median device ms per round --
HIP events around ``FrontierRun.launch_round`` (the round's launches, from the pick to the commit), the first two rounds of a run left
out as warm-up, after one untimed run of the same mode and K.  Nothing is asserted about who wins.

    python tools/frontier_branching_compare.py [--out profiles/frontier_branching_compare.json] [--ks 1,16] [--rounds 40] [--seeds 0,1,2,3] [--candidates 16]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import _lib, frontier, lp_producer, nets      # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice       # noqa: E402

N_ITER, LR, EPS_BAB, WARMUP_ROUNDS = 20, 0.1, 1e-4, 2
CKPT = os.path.join(ROOT, "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")


def one_run(lp, choice, K, rounds, branching, decision_bound, **mode):
    """``branch_and_bound_frontier``'s loop (``frontier._one_job_round`` decides every round) with an event pair around each launch_round."""
    run = frontier.FrontierRun(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, decision_bound=decision_bound, max_rounds=rounds,
                               branching=branching, **mode)
    st = run.root()
    done, bounded, branches, ms = 0, 1, 0, []
    while True:
        reason, k, compact = frontier._one_job_round(st, K, run.capacity, EPS_BAB, decision_bound, done, rounds)
        if reason is not None:
            break
        if compact:
            run.pool.compact(int(st[_lib.FS_N_OPEN]))
        in_use = int(st[_lib.FS_N_OPEN]) if compact else int(st[_lib.FS_IN_USE])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run.launch_round(k, in_use)
        b.record()
        st = run.read_state()                                     # (synchronises: both events have happened)
        frontier._check_record(st)
        ms.append(a.elapsed_time(b))
        done, branches = done + 1, branches + k
        bounded += int(st[_lib.FS_KEPT] + st[_lib.FS_CLOSED] + st[_lib.FS_INFEASIBLE])
    run.check_status()
    timed = ms[WARMUP_ROUNDS:]
    strong = {"strong_bounded": run.strong_bounded} if run.strong_on else {}
    return {"rounds": done, "branches": branches, "domains_bounded": bounded, **strong, "stop": reason, "global_lb": frontier._global_lb(st),
            "global_ub": st[_lib.FS_GLOBAL_UB], "timed_rounds": len(timed),
            "median_device_ms_per_round": round(statistics.median(timed), 4) if timed else None}


def problems(seeds, hard_eps):
    """(name, lp, choice, decision bounds): the first set's problems at decision_bound 0 and without one, then the harder boxes."""
    from tests.frontier_twin import toy
    lp, choice, _ = toy()
    yield "toy_kw property 2 vs 6 eps 0.04", lp, choice, (0.0, None)
    layers = nets.load_verified_net("cifar_base_kw", 3, 5)
    choice = None
    for eps, bounds in ((0.03, (0.0, None)), (hard_eps, (0.0,))):
        for seed in seeds:
            x = torch.from_numpy(np.random.RandomState(seed).standard_normal((3, 32, 32)).astype(np.float32))
            if choice is None:
                lp0 = lp_producer.LayerGraphLP(layers, x - eps, x + eps)
                choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
                choice.verbose = False
            yield f"cifar_base_kw property 3 vs 5 eps {eps} seed {seed}", lp_producer.LayerGraphLP(layers, x - eps, x + eps, bounds="kw_device",
                                                                                                engine=choice.model.engine()), choice, bounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_branching_compare.json"))
    ap.add_argument("--ks", default="1,16")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--seeds", default="0,1,2,3")
    ap.add_argument("--hard-eps", type=float, default=0.09)
    ap.add_argument("--candidates", type=int, default=16, help="strong_candidates of the strong mode")
    args = ap.parse_args()
    torch.set_num_threads(16)
    rec = {"what": f"branch_and_bound_frontier with branching='gnn' against branching='babsr' and branching='strong' (strong_candidates "
                   f"{args.candidates}): n_iter {N_ITER}, lr {LR}, BaB eps "
                   f"{EPS_BAB}, at most {args.rounds} rounds; device ms per round from HIP events around launch_round, median over a run's rounds but its "
                   f"first {WARMUP_ROUNDS}, after one untimed run of the same mode and K",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name, lp, choice, bounds in problems([int(s) for s in args.seeds.split(",")], args.hard_eps):
        for db in bounds:
            for K in (int(k) for k in args.ks.split(",")):
                entry = {"problem": name, "decision_bound": db, "K": K, "beyond_the_root": db is None or f"eps {args.hard_eps} " in name}
                for branching in frontier.BRANCHINGS:
                    mode = {"strong_candidates": args.candidates} if branching == "strong" else {}
                    one_run(lp, choice, K, min(args.rounds, WARMUP_ROUNDS + 1), branching, db, **mode)      # warm-up: allocations, first launches of every shape
                    entry[branching] = one_run(lp, choice, K, args.rounds, branching, db, **mode)
                rec["runs"].append(entry)
                print(json.dumps(entry), flush=True)
                with open(args.out, "w") as f:
                    json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
