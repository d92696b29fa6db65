#!/usr/bin/env python
"""Strong branching inside the device-resident frontier, timed (GPU box).

The problem of tools/frontier_timing.py: cifar_base_kw, eps 0.09, seeded N(0,1) image (RandomState(4)), property 3 vs 5, n_iter 20, lr 0.1,
BaB eps 1e-4, no decision bound.  Per K in --ks, strong_candidates in --candidates ("all": every undecided node) and strong_chunk in
--chunks: ``branch_and_bound_frontier``'s loop with ``branching="strong"`` and a HIP event pair around every ``FrontierRun.launch_round``
(the round's launches from the pick to the commit; the read of the number of candidates lies inside), the first two rounds of a run left
out as warm-up, after one untimed run of the same configuration.  Recorded: the median ms per round, the candidates per round, the ms per
candidate child -- a round's ms over its 2 * candidates child rows, the median over the timed rounds; it carries the round's plain part
(gather, list, pick, the winners' 2k children bounded again, commit) -- and the bytes of the candidate rows ``ChS`` and of the three
workspaces the chunks share with the round.

The reference, in the same session: tools/frontier_timing.py's frontier run at K = 64 (``branching="gnn"``, a code path this mode does not
touch) and its ms per domain over the full rounds.  "ratio" is the best ms per candidate child over that figure.  One more run of the
--profile configuration and one of the reference, both with the library's per-launch profiling on (gnnb_profile_read), give the ms per
kernel class and per child row: where a ratio above 1 comes from.

    python tools/frontier_strong_timing.py [--out profiles/frontier_strong_timing.json] [--ks 1,4] [--candidates 8,32,all] [--chunks 32,64,128,256]
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
from tools.frontier_timing import CKPT, EPS, EPS_BAB, LR, N_ITER, NET, commit_id, frontier as plain_run      # noqa: E402

WARMUP_ROUNDS = 2


def strong_run(lp, choice, K, rounds, candidates, chunk, capacity):
    """``branch_and_bound_frontier``'s loop in strong mode with an event pair around each launch_round.  Returns (per round ms, per round
    candidates, the run)."""
    run = frontier.FrontierRun(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, capacity=capacity, max_rounds=rounds,
                               strong_candidates=candidates, strong_chunk=chunk, branching="strong")
    st = run.root()
    done, ms, cands = 0, [], []
    while True:
        reason, k, compact = frontier._one_job_round(st, K, run.capacity, EPS_BAB, None, done, rounds)
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
        cands.append(run.strong_n)
        done += 1
    run.check_status()
    return ms, cands, run


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def configuration(lp, choice, K, candidates, chunk, rounds, capacity):
    strong_run(lp, choice, K, min(rounds, WARMUP_ROUNDS + 1), candidates, chunk, capacity)      # untimed: allocations, first launches of every shape
    ms, cands, run = strong_run(lp, choice, K, rounds, candidates, chunk, capacity)
    timed = [(t, c) for t, c in list(zip(ms, cands))[WARMUP_ROUNDS:] if c > 0]
    S = run.ChS
    return {"K": K, "strong_candidates": candidates, "strong_chunk": chunk, "rounds": len(ms), "timed_rounds": len(timed),
            "candidates_per_round": cands,
            "median_ms_per_round": round(statistics.median(t for t, _ in timed), 4) if timed else None,
            "median_ms_per_candidate_child": round(statistics.median(t / (2 * c) for t, c in timed), 5) if timed else None,
            "bytes_candidate_rows": nbytes([S.mask, S.alpha, S.beta, S.split] + S.lb + S.ub + S.plb + S.pub),
            "bytes_ws_kw": run.ws_kw.numel(), "bytes_ws_dual": run.ws_dual.numel(), "bytes_ws_strong_list": run.ws_strong.numel()}


def per_class(eng, child_rows, body):
    """ms per kernel class of ``body()`` with per-launch profiling on, and the total over ``child_rows()`` rows bounded."""
    eng.profile_enable(True)
    try:
        eng.profile_read()
        body()
        counts = eng.profile_read()
    finally:
        eng.profile_enable(False)
    rows = child_rows()
    classes = {k: {"ms": round(ms, 3), "launches": n, "ms_per_child_row": round(ms / rows, 5)} for k, (ms, n) in counts.items() if n}
    return {"child_rows": rows, "ms_per_child_row": round(sum(v["ms"] for v in classes.values()) / rows, 5), "classes": classes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_strong_timing.json"))
    ap.add_argument("--ks", default="1,4")
    ap.add_argument("--candidates", default="8,32,all")
    ap.add_argument("--chunks", default="32,64,128,256")
    ap.add_argument("--rounds", type=int, default=8, help="rounds of a run with a candidate limit (the first two are warm-up)")
    ap.add_argument("--rounds-all", type=int, default=4, help="rounds of a run over all undecided nodes")
    ap.add_argument("--reference-k", type=int, default=64)
    ap.add_argument("--reference-rounds", type=int, default=30)
    ap.add_argument("--profile", default="4,32,256", help="K,strong_candidates,strong_chunk of the run with per-launch profiling")
    ap.add_argument("--capacity", type=int, default=8192, help="slots of the pool")
    args = ap.parse_args()
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    lp = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng)
    eng.bind(list(layers[:-1]), (3, 32, 32))
    rec = {"what": f"branch_and_bound_frontier(branching='strong') on {NET}, eps {EPS}, property 3 vs 5, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}: "
                   f"device ms per round from HIP events around launch_round, median over a run's rounds but its first {WARMUP_ROUNDS}, after one "
                   "untimed run of the same configuration; ms per candidate child = a round's ms / (2 * its candidates), which carries the round's plain part",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "commit": commit_id(),
           "library_build_id": _lib.library_build_id(), "relu_nodes": eng.R, "pool_capacity": args.capacity, "reference": None, "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ref = plain_run(lp, choice, args.reference_k, args.reference_rounds, args.capacity)
    rec["reference"] = {"what": f"tools/frontier_timing.py's frontier run at K = {args.reference_k}, branching='gnn' (host wall clock, rounds synchronised by the state read)",
                        **{k: ref[k] for k in ("K", "rounds", "full_rounds", "ms_per_full_round", "ms_per_domain_in_full_rounds", "ms_per_domain")}}
    print(rec["reference"], flush=True)
    write()
    for K in (int(k) for k in args.ks.split(",")):
        for c in args.candidates.split(","):
            for chunk in (int(v) for v in args.chunks.split(",")):
                cand = None if c == "all" else int(c)
                rec["runs"].append(configuration(lp, choice, K, cand, chunk, args.rounds_all if cand is None else args.rounds, args.capacity))
                print(json.dumps(rec["runs"][-1]), flush=True)
                write()
    timed = [r for r in rec["runs"] if r["median_ms_per_candidate_child"] is not None]
    ref_ms = rec["reference"]["ms_per_domain_in_full_rounds"]
    if timed and ref_ms:
        best = min(timed, key=lambda r: r["median_ms_per_candidate_child"])
        rec["best"] = {k: best[k] for k in ("K", "strong_candidates", "strong_chunk", "median_ms_per_candidate_child")}
        rec["ratio"] = round(best["median_ms_per_candidate_child"] / ref_ms, 3)
        by_chunk = {}
        for r in timed:
            by_chunk.setdefault(r["strong_chunk"], []).append(r["median_ms_per_candidate_child"])
        rec["median_ms_per_candidate_child_by_chunk"] = {k: round(statistics.median(v), 5) for k, v in sorted(by_chunk.items())}
    K, cand, chunk = (int(v) for v in args.profile.split(","))
    runs = []
    rec["profiled"] = {"strong": {"K": K, "strong_candidates": cand, "strong_chunk": chunk,
                                  **per_class(eng, lambda: runs[-1].strong_bounded + 2 * K * args.rounds,
                                              lambda: runs.append(strong_run(lp, choice, K, args.rounds, cand, chunk, args.capacity)[2]))},
                       "reference": {"K": args.reference_k,
                                     **per_class(eng, lambda: runs[-1], lambda: runs.append(plain_run(lp, choice, args.reference_k, args.reference_rounds,
                                                                                                      args.capacity)["domains_bounded"]))}}
    write()
    print(json.dumps({k: rec.get(k) for k in ("best", "ratio", "median_ms_per_candidate_child_by_chunk")}))
    print("written", args.out)


if __name__ == "__main__":
    main()
