#!/usr/bin/env python
"""Train the branching scorer offline from strong-branching tables (GPU box): collect -> split -> train -> save.

  collect   per problem (tools/frontier_jobs_timing.py's seeded jobs: the box of --eps around the N(0,1) image RandomState(100 + j), true
            class 3, the wrong class cycling) one ``branch_and_bound_frontier(branching="strong", strong_candidates=--candidates,
            imitate=Replay(every=1, buffer=..., steps=0))`` of --rounds rounds: the teacher runs, the scorer stays frozen, and every parent
            with at least two candidates goes into ONE device-resident ``ReplayBuffer`` with its table row.
  split     the newest --holdout share of the entries moves to a second buffer (``ReplayBuffer.split``).
  train     ``replay.train_epochs``: --epochs epochs of minibatch steps (``gnnb_replay_sample`` + ``gnnb_imitation_step_rows``) from the
            --checkpoint's parameters; after every epoch mean loss, regret, relative regret and top-1 agreement on both buffers.
  save      the module's state dict (the reference's key format, what ``GraphChoice(..., model_name)`` loads) to --out, the per-epoch
            records to --curve as JSON.

    python tools/train_scorer.py --out scorer.pt [--curve curve.json] [--problems 4] [--rounds 8] [--epochs 5] [--batch 8] [--margin 1.0]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_branching_amd import _lib, lp_producer, nets                          # noqa: E402
from gnn_branching_amd.frontier import Replay, ReplayBuffer, branch_and_bound_frontier      # noqa: E402
from gnn_branching_amd.graphnet.graph_score_online import GraphChoice         # noqa: E402
from gnn_branching_amd.replay import train_epochs                             # noqa: E402
from tools.frontier_jobs_timing import CKPT, EPS, EPS_BAB, GT, LR, N_ITER, NET      # noqa: E402

WRONG = [c for c in range(10) if c != GT]


def problem(j, eng, net=NET, eps=EPS):
    """Seeded problem number j on the engine's device bounds."""
    layers = nets.load_verified_net(net, GT, WRONG[j % 9])
    x = torch.from_numpy(np.random.RandomState(100 + j).standard_normal((3, 32, 32)).astype(np.float32))
    return lp_producer.LayerGraphLP(layers, x - eps, x + eps, bounds="kw_device", engine=eng)


def make_choice(checkpoint, lr, wd, net=NET):
    layers = nets.load_verified_net(net, GT, WRONG[0])
    x = torch.zeros(3, 32, 32)
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], checkpoint, lr=lr, wd=wd)
    choice.verbose = False
    choice._eng().bind(list(layers[:-1]), (3, 32, 32))
    return choice


def collect(choice, problems, buffer, K, rounds, candidates, branching="strong", net=NET, eps=EPS):
    """One collecting run per problem into ``buffer``; returns per problem its result and the buffer's counts."""
    out = []
    for j in problems:
        lp = problem(j, choice.model.engine(), net, eps)
        stats = {}
        glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                                                    capacity=8192, log=lambda s: None, stats=stats, strong_candidates=candidates,
                                                                    branching=branching, imitate=Replay(every=1, buffer=buffer, steps=0))
        out.append({"problem": j, "rounds": done, "global_lb": glb, "global_ub": gub, "stop": reason, "branches": stats["branches"],
                    "stored": stats["replay_stored"], "skipped": stats["replay_skipped"], "filled": stats["replay_filled"]})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="where the trained state dict goes")
    ap.add_argument("--curve", default=None, help="where the per-epoch records go (JSON)")
    ap.add_argument("--checkpoint", default=CKPT)
    ap.add_argument("--net", default=NET)
    ap.add_argument("--eps", type=float, default=EPS)
    ap.add_argument("--problems", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--holdout", type=float, default=0.2)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--wd", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.set_num_threads(16)
    choice = make_choice(args.checkpoint, args.lr, args.wd, args.net)
    buffer = ReplayBuffer(choice.model.engine(), args.capacity)
    collected = collect(choice, range(args.problems), buffer, args.K, args.rounds, args.candidates, net=args.net, eps=args.eps)
    holdout = buffer.split(args.holdout)
    records = train_epochs(choice, buffer, args.epochs, batch=args.batch, margin=args.margin, seed=args.seed, holdout=holdout if holdout.filled else None)
    torch.save(choice.model.state_dict(), args.out)
    rec = {"what": f"train_epochs on {args.net}: {args.problems} seeded problems collected with branching='strong' over {args.rounds} rounds each (K {args.K}, "
                   f"{args.candidates} candidates), the newest {args.holdout} held out, {args.epochs} epochs of batch {args.batch} at margin {args.margin}, "
                   f"lr {args.lr}, wd {args.wd}",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(),
           "train_entries": buffer.filled, "holdout_entries": holdout.filled, "collected": collected, "epochs": records, "checkpoint": os.path.basename(args.out)}
    if args.curve:
        with open(args.curve, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec["epochs"], indent=1))


if __name__ == "__main__":
    main()
