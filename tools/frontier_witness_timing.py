#!/usr/bin/env python
"""The witness of the upper bound and the descent on the network inside the device-resident frontier, timed (GPU box).

cifar_base_kw, eps 0.09, seeded N(0,1) image (RandomState(4)), property 3 vs 5, n_iter 20, lr 0.1, eps_bab 1e-4, no decision bound,
branching_threshold 0.2: the set-up of tools/frontier_threshold_timing.py (section 7.5).  Per K in --ks, at a fixed max_rounds, the sides

    parent        the parent commit: --parent-tree, a checkout of it with its library built, run by a worker process of its own
    off           this tree, witness=None, pgd_steps=None
    witness       witness=[...]
    pgd4, pgd16   witness=[...] with pgd_steps 4 and 16 (--pgd)

one warm-up run per side, then --repeats timed runs per side with the sides alternating; wall time between the root's log line and the last
round's (every round ends with the host's read of the state record).  Each tree runs in ONE worker process that lives for the whole
measurement (this file with --worker; it imports the package of the tree it is given), so at most two processes hold the GPU, and the
driver alternates between them run by run.

(a) "off" against "parent": no launch, read or argument of a round changed, so the ratio of the medians should lie inside the parent's own
    (max - min) / median; bounds and counts must be identical.
(b) the other sides: ms per round, global_ub, the gap and the domains bounded after the same number of rounds, and, in a run of their own
    under gnnb_profile_enable, the ms per launch of k_net_descend (against k_net_eval's with the options off) and of k_frontier_witness.

    python tools/frontier_witness_timing.py --parent-tree PATH [--out profiles/frontier_witness_timing.json] [--ks 1,16,64] [--rounds 60,40,30]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET, EPS, N_ITER, LR, EPS_BAB = "cifar_base_kw", 0.09, 20, 0.1, 1e-4
CKPT = os.path.join("models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
KERNELS = ("k_net_eval", "k_net_descend", "k_frontier_witness")


# ---- the worker: one tree, one process, one run per line of stdin ---------------------------------------------------------------------
def worker(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from gnn_branching_amd import _lib, lp_producer, nets
    from gnn_branching_amd.frontier import branch_and_bound_frontier
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], os.path.join(tree, CKPT))
    choice.verbose = False
    eng = choice.model.engine()
    lp = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng)
    eng.bind(list(layers[:-1]), (3, 32, 32))
    print(json.dumps({"ready": True, "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id()}), flush=True)
    for line in sys.stdin:
        cmd = json.loads(line)
        options = dict(cmd["options"])
        if options.pop("witness", False):
            options["witness"] = []
        stamps, stats = [], {}
        if cmd["profile"]:
            eng.profile_enable(1)
            eng.profile_read(reset=True)
        glb, gub, done, bounded, reason = branch_and_bound_frontier(lp, choice, lp.layers, K=cmd["K"], n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=cmd["rounds"],
                                                                    capacity=cmd["capacity"], log=lambda s: stamps.append(time.perf_counter()),
                                                                    branching_threshold=cmd["threshold"], stats=stats, **options)
        out = {"seconds": stamps[-1] - stamps[0], "rounds": done, "domains_bounded": bounded - 1, "stop": reason, "global_lb": glb, "global_ub": gub,
               "stats": stats}
        if cmd["profile"]:
            prof = eng.profile_read(reset=True)
            eng.profile_enable(0)
            out["kernels"] = {k: {"launches": int(prof[k][1]), "ms_per_launch": round(prof[k][0] / prof[k][1], 5) if prof[k][1] else None}
                              for k in KERNELS if k in prof}
        print(json.dumps(out), flush=True)


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

    def run(self, K, rounds, capacity, threshold, options, profile=False):
        self.p.stdin.write(json.dumps({"K": K, "rounds": rounds, "capacity": capacity, "threshold": threshold, "options": options, "profile": profile}) + "\n")
        self.p.stdin.flush()
        return self._read()

    def close(self):
        self.p.stdin.close()
        self.p.wait()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def summary(runs):
    last = runs[-1]
    key = lambda r: (r["global_lb"], r["global_ub"], r["domains_bounded"], r["rounds"])          # noqa: E731
    return {"ms_per_round": spread([1e3 * r["seconds"] / max(r["rounds"], 1) for r in runs]), "rounds": last["rounds"],
            "domains_bounded": last["domains_bounded"], "stop": last["stop"], "global_lb": last["global_lb"], "global_ub": last["global_ub"],
            "gap": last["global_ub"] - last["global_lb"], "kw_pairs_bounded": last["stats"].get("kw_bounded"), "kw_pairs_used": last["stats"].get("kw_used"),
            "same_result_in_every_repeat": all(key(r) == key(last) for r in runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", help="(internal) serve runs on the tree at this path")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_witness_timing.json"))
    ap.add_argument("--ks", default="1,16,64")
    ap.add_argument("--rounds", default="60,40,30")
    ap.add_argument("--pgd", default="4,16")
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=8192, help="slots of the pool")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    new = Worker(ROOT)
    old = Worker(os.path.abspath(args.parent_tree)) if args.parent_tree else None
    sides = {"off": {}, "witness": {"witness": True}}
    sides.update({f"pgd{n}": {"witness": True, "pgd_steps": int(n)} for n in args.pgd.split(",") if n})
    rec = {"what": f"branch_and_bound_frontier(branching_threshold={args.threshold}) on {NET}, eps {EPS}, property 3 vs 5, n_iter {N_ITER}, lr {LR}, BaB eps "
                   f"{EPS_BAB}: the parent commit, the options off, witness only, witness with pgd_steps {args.pgd} (pgd_step 1/64); wall clock on the host, "
                   f"every round synchronised by its state read; one warm-up run per side, then {args.repeats} repeats per side, the sides alternating; "
                   f"median and min / max over the repeats",
           "device": new.info["device"], "library_build_id": new.info["library_build_id"],
           "parent_commit_library_build_id": old.info["library_build_id"] if old else None, "pool_capacity": args.capacity,
           "branching_threshold": args.threshold, "frontier": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        for K, rounds in zip([int(k) for k in args.ks.split(",")], [int(r) for r in args.rounds.split(",")]):
            common = (K, rounds, args.capacity, args.threshold)
            if old:
                old.run(K, min(rounds, 4), args.capacity, args.threshold, {})
            for options in sides.values():                            # warm-up: allocations, first launches
                new.run(K, min(rounds, 4), args.capacity, args.threshold, options)
            runs = {side: [] for side in ["parent"] + list(sides)}
            for _ in range(args.repeats):
                if old:
                    runs["parent"].append(old.run(*common, {}))
                for side, options in sides.items():                   # alternating
                    runs[side].append(new.run(*common, options))
            entry = {"K": K, "max_rounds": rounds}
            entry.update({side: summary(r) for side, r in runs.items() if r})
            entry["kernels_in_runs_of_their_own"] = {side: new.run(*common, options, profile=True)["kernels"] for side, options in sides.items()}
            off = entry["off"]
            if old:
                p = entry["parent"]
                width = round((p["ms_per_round"]["max"] - p["ms_per_round"]["min"]) / p["ms_per_round"]["median"], 4)
                ratio = off["ms_per_round"]["median"] / p["ms_per_round"]["median"]
                same = ("global_lb", "global_ub", "domains_bounded", "rounds", "kw_pairs_bounded", "kw_pairs_used")
                entry["off_against_parent"] = {"ms_per_round_ratio": round(ratio, 4), "parent_spread_of_its_repeats": width,
                                               "inside_the_parent_spread": abs(ratio - 1) <= width,
                                               "bounds_and_counts_identical": all(off[k] == p[k] for k in same)}
            for side in sides:
                if side != "off":
                    entry[side]["ms_per_round_over_off"] = round(entry[side]["ms_per_round"]["median"] / off["ms_per_round"]["median"], 3)
            rec["frontier"].append(entry)
            print(json.dumps(entry), flush=True)
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
    finally:
        new.close()
        if old:
            old.close()
    print("written", args.out)


if __name__ == "__main__":
    main()
