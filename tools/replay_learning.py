#!/usr/bin/env python
"""Does learning from the teacher close the regret, and what does it do to the branch count?  (GPU box) ->
profiles/replay_learning.json.

cifar_base_kw, the shipped checkpoint, the seeded problems of tools/frontier_jobs_timing.py (eps 0.09, true class 3, the wrong class
cycling).  The problems 0 .. --collect - 1 are collected from with ``branching="strong"``, ``strong_candidates=Shortlist(babsr=--candidates,
gnn=--gnn-candidates)`` -- so that every table labels the scorer's own decision and the regret of a row is the regret of a split the scorer
would make -- and ``imitate=Replay(every=1, steps=0)``: a frozen scorer, --rounds rounds of K = --K each.  The newest 20 % of the entries are
held out (``ReplayBuffer.split``) and ``replay.train_epochs`` trains --epochs epochs from the checkpoint.  Recorded:

  * per epoch (0: before training) mean loss, regret, relative regret and top-1 agreement on the training entries and on the held-out ones;
  * on the problems --collect .. --collect + --test - 1, which nothing was collected from, at every eps of --test-eps, two
    ``branching="gnn"`` runs of up to --test-rounds rounds before and after training: "verdict" (decision bound 0: the branches it takes
    to decide the property, 0 when the root decides it) and "budget" (no decision bound: the bounds reached with the same rounds).

A few problems on one network: a direction, not a rate.  No figure is a pass / fail bar.

    python tools/replay_learning.py [--out profiles/replay_learning.json] [--collect 6] [--test 4] [--epochs 5] [--margin 100]
"""
import argparse
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import _lib                                               # noqa: E402
from gnn_branching_amd.frontier import ReplayBuffer, Shortlist, branch_and_bound_frontier      # noqa: E402
from gnn_branching_amd.replay import train_epochs                                # noqa: E402
from tools.frontier_jobs_timing import CKPT, EPS, EPS_BAB, LR, N_ITER, NET       # noqa: E402
from tools.train_scorer import collect, make_choice, problem                     # noqa: E402


def gnn_runs(choice, problems, K, rounds, eps_list):
    """Per problem and eps two "gnn" runs with the scorer as it stands (nothing learns): branches, rounds, the stop reason and the bounds."""
    out = []
    for eps in eps_list:
        for j in problems:
            lp = problem(j, choice.model.engine(), eps=eps)
            for mode, bound in (("verdict", 0.0), ("budget", None)):
                stats = {}
                glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                                                            decision_bound=bound, capacity=8192, log=lambda s: None, stats=stats)
                out.append({"problem": j, "eps": eps, "mode": mode, "branches": stats["branches"], "rounds": done, "domains_bounded": bounded, "stop": reason,
                            "global_lb": glb, "global_ub": gub})
                print(json.dumps(out[-1]), flush=True)
    return out


def totals(runs):
    """The branches of the verdict runs and how many of them reached a verdict; the branches and the mean lower bound of the budget runs."""
    budget = [r["global_lb"] for r in runs if r["mode"] == "budget"]
    return {"verdict_branches": sum(r["branches"] for r in runs if r["mode"] == "verdict"),
            "verdict_decided": sum(1 for r in runs if r["mode"] == "verdict" and r["stop"] in ("decision", "exhausted", "gap")),
            "budget_branches": sum(r["branches"] for r in runs if r["mode"] == "budget"), "budget_mean_global_lb": sum(budget) / max(1, len(budget))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_learning.json"))
    ap.add_argument("--collect", type=int, default=6, help="problems collected from")
    ap.add_argument("--test", type=int, default=4, help="problems the branch counts are taken on (not collected from)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--test-rounds", type=int, default=40)
    ap.add_argument("--test-eps", default="0.09,0.04,0.02")
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--gnn-candidates", type=int, default=4)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--margin", type=float, default=100.0, help="score units per unit of improvement (the checkpoint's scores lie 5..50 apart)")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--wd", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.set_num_threads(16)
    choice = make_choice(CKPT, args.lr, args.wd)
    eng = choice.model.engine()
    test = list(range(args.collect, args.collect + args.test))
    test_eps = [float(v) for v in args.test_eps.split(",")]
    before = gnn_runs(choice, test, args.K, args.test_rounds, test_eps)
    buffer = ReplayBuffer(eng, args.capacity)
    collected = collect(choice, range(args.collect), buffer, args.K, args.rounds, Shortlist(babsr=args.candidates, gnn=args.gnn_candidates))
    holdout = buffer.split(0.2)
    records = train_epochs(choice, buffer, args.epochs, batch=args.batch, margin=args.margin, seed=args.seed, holdout=holdout if holdout.filled else None)
    after = gnn_runs(choice, test, args.K, args.test_rounds, test_eps)
    rec = {"what": f"{NET}, shipped checkpoint, eps {EPS}, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}: problems 0..{args.collect - 1} collected with "
                   f"branching='strong', Shortlist(babsr={args.candidates}, gnn={args.gnn_candidates}), imitate=Replay(every=1, steps=0), K {args.K}, "
                   f"{args.rounds} rounds each; the newest 20 % of the entries held out; {args.epochs} epochs of batch {args.batch} at margin {args.margin}, "
                   f"Adam lr {args.lr} wd {args.wd}, draws seeded {args.seed}; 'gnn' runs (up to {args.test_rounds} rounds; 'verdict': decision bound 0, "
                   f"'budget': none) on problems {test[0]}..{test[-1]} at eps {test_eps} before and after.  A few problems, one network: a direction, not a rate",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(),
           "train_entries": buffer.filled, "holdout_entries": holdout.filled, "collected": collected, "epochs": records,
           "gnn_runs_before": before, "gnn_runs_after": after,
           "totals_before": totals(before), "totals_after": totals(after)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("train_entries", "holdout_entries", "totals_before", "totals_after")}, indent=1))
    print("written", args.out)


if __name__ == "__main__":
    main()
