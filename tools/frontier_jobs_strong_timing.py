#!/usr/bin/env python
"""Strong branching and the imitation step for many jobs in one pool, timed (GPU box).

The jobs of tools/frontier_jobs_timing.py: cifar_base_kw, job j the box of eps 0.09 around the seeded N(0,1) image RandomState(100 + j),
true class 3, the wrong class cycling; n_iter 20, lr 0.1, BaB eps 1e-4, no decision bound.  strong_candidates 16, K = 4, strong_chunk 256.
With section 7.11's method -- a HIP event pair around every ``launch_round`` (the round's launches from the pick to the commit; the read
of the candidate counts lies inside), the median over a run's rounds but its first two, after one untimed run of the same configuration --

  * TOGETHER: J = 1, 4 and 16 jobs in flight in one ``StrongJobsRun`` (segments = J): ms per round, candidates per round, ms per candidate
    child (a round's ms over its 2 * candidates child rows; it carries the round's plain part);
  * ONE AT A TIME, in the same session: the same J jobs through ``FrontierRun(branching="strong")`` one after the other: per job the same
    figures; "ms_per_round_of_all_jobs" is the sum of the jobs' median ms per round -- what it costs to advance every job by one round --
    and the ms per candidate child the median over the timed rounds of all jobs.

The step: a ``StrongJobsRun`` with ``imitate=1`` at J = 4 and J = 16 (n = 16 and 64 parent rows in a full round), an event pair around
``_imitate`` (one ``gnnb_imitation_step_rows``, which synchronises), the median over the rounds but the first two; the device memory the
step needs is the drop of the device's free memory (hipMemGetInfo) from before the run's first step to after each step -- the step's
buffers are the library's, outside torch's allocator, and grow with the rows of a step; the figure after a step over a full round (n =
4 J rows) is the one the record names.  A step that returns GNNB_E_NOMEM is recorded with its n.

No figure is a pass / fail bar.

    python tools/frontier_jobs_strong_timing.py [--out profiles/frontier_jobs_strong_timing.json] [--jobs 1,4,16] [--rounds 8]
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
from tools.frontier_jobs_timing import CKPT, EPS, EPS_BAB, GT, LR, N_ITER, NET, make_lps      # noqa: E402
from tools.frontier_strong_timing import WARMUP_ROUNDS, strong_run   # noqa: E402
from tools.frontier_timing import commit_id                          # noqa: E402

K, CANDIDATES, CHUNK = 4, 16, 256


def event_pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def jobs_run(lps, choice, rounds, capacity, imitate=None):
    """All the jobs of ``lps`` in flight in one ``StrongJobsRun``, an event pair around each launch_round and, with ``imitate``, around
    each step.  Returns (per round ms, per round candidates, per round parent rows, per step (rows, ms, the drop of the device's free
    memory since before the run's first step), run)."""
    J = len(lps)
    jobs = [frontier.FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps]
    extra = {} if imitate is None else {"imitate": imitate}
    run = frontier.StrongJobsRun(choice, lps[0].layers[:-1], jobs, tuple(lps[0].input_lb.shape), K, J, capacity, N_ITER, LR, EPS_BAB,
                                 strong_candidates=CANDIDATES, strong_chunk=CHUNK, **extra)
    for s in range(J):
        run.admit(s, s)
    run.launch_roots(list(range(J)))
    st = run.read_state()
    ms, cands, rows, steps, free0 = [], [], [], [], None
    for _ in range(rounds):
        entries, compact, stopped = frontier.plan_round([r if int(r[_lib.FS_N_OPEN]) > 0 and r[_lib.FS_GLOBAL_UB] - frontier._global_lb(r) > EPS_BAB else None
                                                         for r in st], K, capacity)
        if not entries or stopped:
            break
        if any(compact):
            run.compact(compact)
        a, b = event_pair()
        a.record()
        run.launch_round(entries)
        b.record()
        st = frontier.JobsRun.read_state(run)                     # (synchronises: both events have happened)
        ms.append(a.elapsed_time(b))
        cands.append(run.strong_n)
        rows.append(run.k)
        if run.imitate_pending:
            if free0 is None:
                free0 = torch.cuda.mem_get_info()[0]
            a, b = event_pair()
            a.record()
            run._imitate()
            b.record()
            torch.cuda.synchronize()
            steps.append((run.last_imitation, a.elapsed_time(b), free0 - torch.cuda.mem_get_info()[0]))
        for r in st:
            frontier._check_record(r)
    run.check_status()
    return ms, cands, rows, steps, run


def figures(ms, cands):
    timed = [(t, c) for t, c in list(zip(ms, cands))[WARMUP_ROUNDS:] if c > 0]
    return timed, {"rounds": len(ms), "timed_rounds": len(timed), "candidates_per_round": cands,
                   "median_ms_per_round": round(statistics.median(t for t, _ in timed), 4) if timed else None,
                   "median_ms_per_candidate_child": round(statistics.median(t / (2 * c) for t, c in timed), 5) if timed else None}


def together(lps, choice, rounds, capacity):
    jobs_run(lps, choice, WARMUP_ROUNDS + 1, capacity)            # untimed: allocations, first launches of every shape
    ms, cands, rows, _, run = jobs_run(lps, choice, rounds, capacity)
    return {"J": len(lps), "parent_rows_per_round": rows, **figures(ms, cands)[1]}


def one_at_a_time(lps, choice, rounds, capacity):
    strong_run(lps[0], choice, K, WARMUP_ROUNDS + 1, CANDIDATES, CHUNK, capacity)
    per_job, all_timed = [], []
    for lp in lps:
        ms, cands, _ = strong_run(lp, choice, K, rounds, CANDIDATES, CHUNK, capacity)
        timed, fig = figures(ms, cands)
        per_job.append(fig)
        all_timed += timed
    med = [f["median_ms_per_round"] for f in per_job if f["median_ms_per_round"] is not None]
    return {"J": len(lps), "ms_per_round_of_all_jobs": round(sum(med), 4) if med else None,
            "median_ms_per_candidate_child": round(statistics.median(t / (2 * c) for t, c in all_timed), 5) if all_timed else None, "per_job": per_job}


def step_figures(lps, rounds, capacity):
    """The step over the parent rows of J jobs: a fresh online choice (the run moves its parameters)."""
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice as OnlineChoice
    lp0 = lps[0]
    choice = OnlineChoice([torch.full((int(np.prod(lp0.shapes[i + 1])),), -1, dtype=torch.long) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    own = make_lps(len(lps), choice.model.engine())
    out = {"J": len(lps), "rows_of_a_full_round": len(lps) * K}
    try:
        ms, cands, rows, steps, run = jobs_run(own, choice, rounds, capacity, imitate=1)
    except RuntimeError as e:
        if "lower segments or K" not in str(e):
            raise
        return {**out, "GNNB_E_NOMEM": True, "message": str(e)}
    timed = steps[WARMUP_ROUNDS:]
    return {**out, "steps": len(steps), "rows_per_step": [n for n, _, _ in steps], "ms_per_step": [round(t, 4) for _, t, _ in steps],
            "median_ms_per_step": round(statistics.median(t for _, t, _ in timed), 4) if timed else None,
            "device_bytes_taken_since_before_the_first_step": [b for _, _, b in steps],
            "device_bytes_at_full_rounds": max((b for n, _, b in steps if n == len(lps) * K), default=None),
            "median_round_ms_without_the_step": figures(ms, cands)[1]["median_ms_per_round"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_jobs_strong_timing.json"))
    ap.add_argument("--jobs", default="1,4,16")
    ap.add_argument("--step-jobs", default="4,16", help="jobs in flight of the runs that learn (n = 4 J parent rows in a full round)")
    ap.add_argument("--rounds", type=int, default=8, help="rounds of a run (the first two are warm-up)")
    ap.add_argument("--capacity", type=int, default=129, help="slots per job, on both sides")
    args = ap.parse_args()
    torch.set_num_threads(16)
    Js = [int(v) for v in args.jobs.split(",")]
    step_Js = [int(v) for v in args.step_jobs.split(",") if v]
    layers = nets.load_verified_net(NET, GT, 5)
    x = torch.zeros(3, 32, 32)
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    lps = make_lps(max(Js + step_Js), eng)
    rec = {"what": f"verify_properties_strong's run (StrongJobsRun, all J jobs in flight, segments = J) vs the same jobs one at a time through "
                   f"branch_and_bound_frontier(branching='strong'), {NET}, eps {EPS}, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, K {K}, strong_candidates "
                   f"{CANDIDATES}, strong_chunk {CHUNK}, {args.capacity} slots per job: device ms per round from HIP events around launch_round, median over a "
                   f"run's rounds but its first {WARMUP_ROUNDS}, after one untimed run; ms per candidate child = a round's ms / (2 * its candidates)",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(), "commit": commit_id(),
           "library_build_id": _lib.library_build_id(), "relu_nodes": None, "together": [], "one_at_a_time": [], "imitation_step": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    for J in Js:
        rec["together"].append(together(lps[:J], choice, args.rounds, args.capacity))
        rec["relu_nodes"] = eng.R
        print(json.dumps(rec["together"][-1]), flush=True)
        rec["one_at_a_time"].append(one_at_a_time(lps[:J], choice, args.rounds, args.capacity))
        print(json.dumps({k: v for k, v in rec["one_at_a_time"][-1].items() if k != "per_job"}), flush=True)
        write()
    for J in step_Js:
        rec["imitation_step"].append(step_figures(lps[:J], args.rounds, args.capacity))
        print(json.dumps(rec["imitation_step"][-1]), flush=True)
        write()
    print("written", args.out)


if __name__ == "__main__":
    main()
