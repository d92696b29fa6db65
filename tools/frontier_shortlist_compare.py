#!/usr/bin/env python
"""What shortlisting the strong-branching candidates by the GNN's own scores changes (GPU box).

Problems and settings of tools/frontier_branching_compare.py's harder group: cifar_base_kw, property 3 vs 5 at eps 0.09 on the seeded N(0,1)
images of --seeds, decision_bound 0, n_iter 20, lr 0.1, BaB eps 1e-4, K = 1 and 16, --rounds rounds at most, the shipped checkpoint.

(1) ``branching="gnn"`` with ``strong_audit``: ``strong_candidates=16`` (the option off) against ``Shortlist(babsr=16, gnn=G)``, G in --gs.
    An audit changes no decision, so every one of these runs visits the same parents.  Per run: the HOLE, the share of parents whose
    committed (GNN) decision lies outside BaBSR's top 16 (off: it has no entry in the table; union: its source is 2); the share of parents
    whose decision has an entry; the regret of the committed decision, best_improvement - improvement over the parents where both are
    numbers (off: "best" is the best of BaBSR's 16 only, so it can be negative), mean and worst over the run and the worst per round;
    candidates per parent; the median device ms per round.
(2) ``branching="strong"`` over ``Shortlist(gnn=4)`` against ``branching="gnn"`` and ``branching="strong"`` with ``strong_candidates=16``:
    global_lb / global_ub after equal rounds and ms per round.
(3) with --parent-tree (a checkout of the parent commit with its library built): the option-off run of (1) on seed --seeds[0] by the parent
    tree, the parent tree again and this tree, --repeats times in that alternation; the spread of the parent's own medians is the yardstick,
    and a difference counts as real only beyond three times it.

ms per round: HIP events around ``FrontierRun.launch_round``, the first two rounds of a run left out, after one untimed run of the same mode
and K; the audit's device-to-host copies lie behind the second event.  Nothing is asserted.

    python tools/frontier_shortlist_compare.py [--out profiles/frontier_shortlist.json] [--ks 1,16] [--rounds 40] [--seeds 0,1,2,3] [--gs 1,4,8]
                                               [--parent-tree DIR] [--repeats 3]
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET, EPS, N_ITER, LR, EPS_BAB, WARMUP_ROUNDS, M = "cifar_base_kw", 0.09, 20, 0.1, 1e-4, 2, 16
CKPT = os.path.join("models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")


# ---- the worker: one tree, one process, one run per line of stdin (the parent commit's tree serves the option-off run only) -------------
def worker(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from gnn_branching_amd import _lib, frontier, lp_producer, nets
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    made = {}

    def problem(seed):
        if seed not in made:
            x = torch.from_numpy(np.random.RandomState(seed).standard_normal((3, 32, 32)).astype(np.float32))
            if "choice" not in made:
                lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
                made["choice"] = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], os.path.join(tree, CKPT))
                made["choice"].verbose = False
            made[seed] = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=made["choice"].model.engine())
        return made[seed], made["choice"]

    def one_run(cmd):
        lp, choice = problem(cmd["seed"])
        K, rounds, gnn = cmd["K"], cmd["rounds"], cmd["gnn"]
        mode = {}
        if cmd["babsr"] or gnn:
            mode["strong_candidates"] = frontier.Shortlist(babsr=cmd["babsr"], gnn=gnn) if gnn else cmd["babsr"]
        audit = [] if cmd["audit"] else None
        run = frontier.FrontierRun(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, decision_bound=0.0, max_rounds=rounds,
                                   branching=cmd["branching"], strong_audit=audit, **mode)
        off = [0]
        for s in run.eng.sizes[1:-1]:
            off.append(off[-1] + s)
        st = run.root()
        done, branches, ms, per_round = 0, 0, [], []
        while True:
            reason, k, compact = frontier._one_job_round(st, K, run.capacity, EPS_BAB, 0.0, done, rounds)
            if reason is not None:
                break
            if compact:
                run.pool.compact(int(st[_lib.FS_N_OPEN]))
            in_use = int(st[_lib.FS_N_OPEN]) if compact else int(st[_lib.FS_IN_USE])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run.launch_round(k, in_use)
            b.record()
            n0 = len(audit) if audit is not None else 0
            frontier._report_launched(run, None, 0, 0, k, {})       # (the audit's copies: behind the second event)
            st = run.read_state()
            frontier._check_record(st)
            ms.append(a.elapsed_time(b))
            done, branches = done + 1, branches + k
            if audit is not None:
                per_round.append(audit[n0:])
        run.check_status()
        timed = ms[WARMUP_ROUNDS:]
        out = {"rounds": done, "branches": branches, "stop": reason, "global_lb": frontier._global_lb(st), "global_ub": st[_lib.FS_GLOBAL_UB],
               "timed_rounds": len(timed), "median_device_ms_per_round": round(statistics.median(timed), 4) if timed else None}
        if run.strong_on:
            out["candidates_per_parent"] = round(run.strong_bounded / 2 / max(branches, 1), 3)
        if audit is not None:
            outside = labelled = 0
            regrets, worst_per_round = [], []
            for rows in per_round:
                of_round = []
                for a in rows:
                    flat = off[a["decision"][0]] + a["decision"][1] if a["decision"][0] >= 0 else -1
                    has = flat in a["candidates"]
                    labelled += has
                    outside += (a["sources"][a["candidates"].index(flat)] == 2) if "sources" in a and has else (not has)
                    r = a["best_improvement"] - a["improvement"]
                    if r == r:
                        of_round.append(r)
                regrets += of_round
                worst_per_round.append(round(max(of_round), 6) if of_round else None)
            n = max(len(audit), 1)
            out.update(parents=len(audit), decision_outside_babsr_top=outside, hole_share=round(outside / n, 4), decision_labelled_share=round(labelled / n, 4),
                       regret_parents=len(regrets), regret_mean=round(statistics.mean(regrets), 6) if regrets else None,
                       regret_worst=round(max(regrets), 6) if regrets else None, regret_worst_per_round=worst_per_round)
        return out
    print(json.dumps({"ready": True, "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id()}), flush=True)
    for line in sys.stdin:
        print(json.dumps(one_run(json.loads(line))), flush=True)


class Worker:
    def __init__(self, tree):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                  cwd=tree)
        self.info = self._read()

    def _read(self):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"the worker ended (exit status {self.p.wait()})")
            if line.startswith("{"):
                return json.loads(line)

    def run(self, seed, K, rounds, branching="gnn", babsr=None, gnn=None, audit=False):
        self.p.stdin.write(json.dumps({"seed": seed, "K": K, "rounds": rounds, "branching": branching, "babsr": babsr, "gnn": gnn, "audit": audit}) + "\n")
        self.p.stdin.flush()
        return self._read()

    def timed(self, seed, K, rounds, **mode):
        self.run(seed, K, min(rounds, WARMUP_ROUNDS + 1), **mode)      # warm-up: allocations, first launches of every shape
        return self.run(seed, K, rounds, **mode)

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", help="(internal) serve runs on the tree at this path")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_shortlist.json"))
    ap.add_argument("--ks", default="1,16")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--seeds", default="0,1,2,3")
    ap.add_argument("--gs", default="1,4,8")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    seeds, ks, gs = ([int(v) for v in s.split(",")] for s in (args.seeds, args.ks, args.gs))
    new = Worker(ROOT)
    old = Worker(os.path.abspath(args.parent_tree)) if args.parent_tree else None
    rec = {"what": f"{NET}, property 3 vs 5, eps {EPS}, decision_bound 0, n_iter {N_ITER}, lr {LR}, BaB eps {EPS_BAB}, at most {args.rounds} rounds: (1) "
                   f"branching='gnn' audited with strong_candidates={M} against Shortlist(babsr={M}, gnn=G); (2) branching='strong' over Shortlist(gnn=4) "
                   f"against 'gnn' and 'strong' with strong_candidates={M}; (3) the option-off run against the parent commit's tree.  Device ms per round: HIP "
                   f"events around launch_round, median over a run's rounds but its first {WARMUP_ROUNDS}, after one untimed run of the same mode and K",
           "date": datetime.date.today().isoformat(), "device": new.info["device"], "library_build_id": new.info["library_build_id"],
           "parent_commit_library_build_id": old.info["library_build_id"] if old else None, "audited_gnn": [], "look_ahead": [], "against_parent": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    try:
        for seed in seeds:
            for K in ks:
                entry = {"seed": seed, "K": K, "off": new.timed(seed, K, args.rounds, babsr=M, audit=True)}
                for G in gs:
                    entry[f"gnn{G}"] = new.timed(seed, K, args.rounds, babsr=M, gnn=G, audit=True)
                rec["audited_gnn"].append(entry)
                print(json.dumps(entry), flush=True)
                entry = {"seed": seed, "K": K, "gnn": new.timed(seed, K, args.rounds), "strong_babsr16": new.timed(seed, K, args.rounds, branching="strong", babsr=M),
                         "strong_gnn4": new.timed(seed, K, args.rounds, branching="strong", gnn=4)}
                rec["look_ahead"].append(entry)
                print(json.dumps(entry), flush=True)
                save()
        if old:
            for K in ks:
                mode = {"babsr": M, "audit": True}
                old.timed(seeds[0], K, args.rounds, **mode)
                new.timed(seeds[0], K, args.rounds, **mode)
                runs = {"parent_a": [], "parent_b": [], "branch": []}
                for _ in range(args.repeats):
                    runs["parent_a"].append(old.run(seeds[0], K, args.rounds, **mode))
                    runs["parent_b"].append(old.run(seeds[0], K, args.rounds, **mode))
                    runs["branch"].append(new.run(seeds[0], K, args.rounds, **mode))
                ms = {side: [r["median_device_ms_per_round"] for r in rs] for side, rs in runs.items()}
                parents = ms["parent_a"] + ms["parent_b"]
                spread = max(parents) - min(parents)
                diff = statistics.median(ms["branch"]) - statistics.median(parents)
                key = lambda r: (r["global_lb"], r["global_ub"], r["rounds"], r["branches"], r.get("regret_mean"))      # noqa: E731
                entry = {"seed": seeds[0], "K": K, "median_device_ms_per_round": ms, "parent_spread_ms": round(spread, 4),
                         "branch_minus_parent_ms": round(diff, 4), "beyond_three_spreads": abs(diff) > 3 * spread,
                         "same_result_on_both_sides": all(key(r) == key(runs["branch"][0]) for rs in runs.values() for r in rs)}
                rec["against_parent"].append(entry)
                print(json.dumps(entry), flush=True)
                save()
    finally:
        new.close()
        if old:
            old.close()
    save()
    print("written", args.out)


if __name__ == "__main__":
    main()
