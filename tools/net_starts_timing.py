#!/usr/bin/env python
"""The upper bound from many starts, timed (GPU box).

cifar_base_kw, eps 0.09, seeded N(0,1) image (RandomState(4)), property 3 vs 5: the set-up of tools/frontier_witness_timing.py (section 7.8).

(a) the tile kernel against what exists.  B in --bs root-box rows (start 0 a seeded uniform point of the box, per row) x n_starts in
    --starts (S = gnnb_net_descend_starts_tile()), 4 steps of 1/64: gnnb_net_descend_starts against the unchanged gnnb_net_descend fed the same
    B * n_starts points as a flat batch.  The results are asserted identical first (every start's value and steps, the winner's point).  One
    warm-up, then --repeats timed repeats per side, the sides alternating; a repeat is the wall time of --calls back-to-back calls between two
    synchronisations, per call.  Median (min - max) and the A/A spread (max - min) / median of each side.  The flat batch is the baseline: the
    tile form counts as a gain only where flat / tile - 1 exceeds three times the larger spread.  k_net_starts, k_net_descend_tile and
    k_net_starts_pick per launch under gnnb_profile_enable, in a run of their own.
(b) the frontier.  K in --ks, n_iter 20, branching_threshold 0.2, at a fixed max_rounds, the sides

    parent        the parent commit: --parent-tree, a checkout of it with its library built, run by a worker process of its own
    off           this tree, every option off
    pgd4          witness with pgd_steps 4
    pgd4_r16      ... and pgd_restarts 16
    pgd0_r64      pgd_steps 0 and pgd_restarts 64 (the reference's random upper bound with the LP point added)

    one warm-up run per side, then --repeats timed runs per side with the sides alternating; ms per round, global_ub, the gap and the domains
    bounded.  "off" against "parent": the ratio of the medians beside the parent's own spread; bounds and counts must be identical.

    python tools/net_starts_timing.py --parent-tree PATH [--out profiles/net_starts_timing.json]

--parent-lib PATH (the walk of the bound network as one template, gnnb_k_net.h): this tree against the PARENT COMMIT'S LIBRARY
(tools/mklib.sh <parent> parent), a worker of this tree with GNNB_LIB set -- the Python side is the same on both.  (a) gnnb_net_eval, the flat
gnnb_net_descend and gnnb_net_descend_starts at the same B x n_starts sizes, the results asserted identical between the libraries first; (b) the
sides off, pgd4 and pgd4_r16, each against the parent's library under the same options: bounds and counts must be identical.  The sides
alternate repeat by repeat.  The bar at every size and side: this tree's median no more than three times the larger A/A spread of the two above
the parent's.

    python tools/net_starts_timing.py --parent-lib tools/ablate/parent.so --repeats 9 [--out profiles/net_walk_refactor_timing.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET, EPS, N_ITER, LR, EPS_BAB = "cifar_base_kw", 0.09, 20, 0.1, 1e-4
CKPT = os.path.join("models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
KERNELS = ("k_net_eval", "k_net_descend", "k_net_starts", "k_net_descend_tile", "k_net_starts_pick", "k_frontier_witness")
STEPS, STEP, SEED = 4, 1.0 / 64, 0


def spread(values, digits=4):
    med = statistics.median(values)
    return {"median": round(med, digits), "min": round(min(values), digits), "max": round(max(values), digits),
            "aa_spread": round((max(values) - min(values)) / med, 4)}


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
    fixed = list(layers[:-1])
    eng.bind(fixed, (3, 32, 32))
    print(json.dumps({"ready": True, "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id()}), flush=True)

    def kernels(prof):
        return {k: {"launches": int(prof[k][1]), "ms_per_launch": round(prof[k][0] / prof[k][1], 5) if prof[k][1] else None} for k in KERNELS if k in prof}

    def walk_calls(B, n):
        """(starts, x0, lo, hi, {call: closure}) of part (a): B root-box rows x n starts"""
        dev, f64 = eng.device, torch.float64
        lo = (x - EPS).reshape(1, -1).to(dev, f64).expand(B, -1).contiguous()
        hi = (x + EPS).reshape(1, -1).to(dev, f64).expand(B, -1).contiguous()
        u = torch.rand((B, lo.shape[1]), generator=torch.Generator().manual_seed(B), dtype=f64).to(dev)
        x0 = torch.minimum(torch.maximum((lo + (hi - lo) * u).float(), lo.float()), hi.float()).reshape(B, 3, 32, 32).contiguous()
        pw = layers[-1].weight.detach().reshape(1, -1).to(dev, torch.float32).expand(B, -1).contiguous()
        pb = layers[-1].bias.detach().reshape(1).to(dev, torch.float32).expand(B).contiguous()
        starts = eng.net_starts(fixed, x0, lo, hi, n - 1, SEED)
        rep = lambda t: t.repeat_interleave(n, dim=0).contiguous()          # noqa: E731
        flat_args = (fixed, None, starts.reshape(B * n, 3, 32, 32), rep(lo), rep(hi), STEPS, STEP)
        flat_prop = (rep(pw), rep(pb))
        flat = lambda: eng.net_descend(*flat_args, prop=flat_prop, want_steps=True)          # noqa: E731
        tile = lambda: eng.net_descend_starts(fixed, None, starts, lo, hi, STEPS, STEP, prop=(pw, pb), want_index=True, want_values=True,  # noqa: E731
                                              want_steps=True, in_shape=(3, 32, 32))
        ev = lambda: eng.net_eval(fixed, None, flat_args[2], prop=flat_prop)          # noqa: E731
        return starts, x0, lo, hi, {"eval": ev, "flat": flat, "tile": tile}

    def timed(f, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    def tile_against_flat(cmd):
        B, n, calls, repeats = cmd["B"], cmd["n_starts"], cmd["calls"], cmd["repeats"]
        starts, x0, lo, hi, call = walk_calls(B, n)
        flat, tile, dev = call["flat"], call["tile"], eng.device
        fx, fv, _, fs = flat()
        x_best, value, index, values, steps = tile()
        torch.cuda.synchronize()
        fx, fv, fs = fx.reshape(B, n, -1), fv.reshape(B, n), fs.reshape(B, n)
        same = bool(torch.equal(values.view(torch.int64), fv.view(torch.int64)) and torch.equal(steps, fs))
        rows = torch.arange(B, device=dev)
        same = same and bool(torch.equal(x_best, fx[rows, index.long()]) and torch.equal(value.view(torch.int64), fv[rows, index.long()].view(torch.int64)))
        assert same, ("gnnb_net_descend_starts and the flat batch of gnnb_net_descend differ", B, n)

        timed(flat, calls), timed(tile, calls)                             # warm-up
        ms = {"flat": [], "tile": []}
        for _ in range(repeats):                                            # alternating
            ms["flat"].append(timed(flat, calls))
            ms["tile"].append(timed(tile, calls))
        eng.profile_enable(1)
        eng.profile_read(reset=True)
        eng.net_starts(fixed, x0, lo, hi, n - 1, SEED, starts=starts)
        tile(), flat()
        prof = eng.profile_read(reset=True)
        eng.profile_enable(0)
        out = {"B": B, "n_starts": n, "points": B * n, "steps": STEPS, "identical": same, "least_value_of_row_0": float(value[0]),
               "start_0_value_of_row_0": float(values[0, 0]), "rows_where_a_random_start_wins": int((index != 0).sum()),
               "flat_ms": spread(ms["flat"]), "tile_ms": spread(ms["tile"]), "kernels": kernels(prof)}
        gain = out["flat_ms"]["median"] / out["tile_ms"]["median"]
        bar = 3 * max(out["flat_ms"]["aa_spread"], out["tile_ms"]["aa_spread"])
        out.update(flat_over_tile=round(gain, 3), three_times_the_larger_spread=round(bar, 4), gain_beyond_three_spreads=bool(gain - 1 > bar))
        return out

    walk = {}

    def walk_setup(cmd):
        """the three calls at one size, warmed up; a digest of everything they return"""
        walk.clear()
        walk.update(walk_calls(cmd["B"], cmd["n_starts"])[4])
        h = hashlib.sha256()
        for name in sorted(walk):
            out = walk[name]()
            for t in (out if isinstance(out, tuple) else (out,)):
                if t is not None:
                    h.update(t.contiguous().cpu().numpy().tobytes())
            timed(walk[name], cmd["calls"])
        return {"results_sha256": h.hexdigest()}

    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd.get("what") == "walk_setup":
            print(json.dumps(walk_setup(cmd)), flush=True)
            continue
        if cmd.get("what") == "walk_repeat":
            print(json.dumps({name: timed(f, cmd["calls"]) for name, f in sorted(walk.items())}), flush=True)
            continue
        if cmd.get("what") == "tile":
            print(json.dumps({"tile": eng.lib.gnnb_net_descend_starts_tile()}), flush=True)
            continue
        if cmd.get("what") == "kernel":
            print(json.dumps(tile_against_flat(cmd)), flush=True)
            continue
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
            out["kernels"] = kernels(prof)
        print(json.dumps(out), flush=True)


class Worker:
    def __init__(self, tree, lib=None):
        env = dict(os.environ, GNNB_LIB=os.path.abspath(lib)) if lib else None
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                  cwd=tree, env=env)
        self.info = self._read()

    def _read(self):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"the worker ended (exit status {self.p.wait()})")
            if line.startswith("{"):
                return json.loads(line)

    def ask(self, cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        return self._read()

    def run(self, K, rounds, capacity, threshold, options, profile=False):
        return self.ask({"K": K, "rounds": rounds, "capacity": capacity, "threshold": threshold, "options": options, "profile": profile})

    def close(self):
        self.p.stdin.close()
        self.p.wait()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def summary(runs):
    last = runs[-1]
    key = lambda r: (r["global_lb"], r["global_ub"], r["domains_bounded"], r["rounds"])          # noqa: E731
    return {"ms_per_round": spread([1e3 * r["seconds"] / max(r["rounds"], 1) for r in runs]), "rounds": last["rounds"],
            "domains_bounded": last["domains_bounded"], "stop": last["stop"], "global_lb": last["global_lb"], "global_ub": last["global_ub"],
            "gap": last["global_ub"] - last["global_lb"], "kw_pairs_bounded": last["stats"].get("kw_bounded"), "kw_pairs_used": last["stats"].get("kw_used"),
            "same_result_in_every_repeat": all(key(r) == key(last) for r in runs)}


def against(new, old):
    """the project's bar: this tree's median no more than three times the larger A/A spread of the two sides above the parent's"""
    ratio, width = new["median"] / old["median"], 3 * max(new["aa_spread"], old["aa_spread"])
    return {"tree_over_parent": round(ratio, 4), "three_times_the_larger_spread": round(width, 4), "within_the_bar": bool(ratio - 1 <= width)}


def refactor(args):
    """this tree against the parent commit's library: part (a)'s three calls, part (b)'s sides off / pgd4 / pgd4_r16"""
    libs = {"tree": Worker(ROOT), "parent": Worker(ROOT, lib=args.parent_lib)}
    S = libs["tree"].ask({"what": "tile"})["tile"]
    sides = {"off": {}, "pgd4": {"witness": True, "pgd_steps": 4}, "pgd4_r16": {"witness": True, "pgd_steps": 4, "pgd_restarts": 16}}
    rec = {"what": f"{NET}, eps {EPS}, property 3 vs 5: this tree (the walk of the bound network as one template) against the parent commit's library, "
                   f"one worker process per library, the same Python.  kernel: gnnb_net_eval, gnnb_net_descend on B * n_starts points and "
                   f"gnnb_net_descend_starts (S = {S}), {STEPS} steps of 1/64, root-box rows; ms per call, wall clock on the host around {args.calls} "
                   f"back-to-back calls; one warm-up, {args.repeats} repeats per side, the sides alternating repeat by repeat; median, min / max and "
                   f"the A/A spread (max - min) / median.  frontier: branch_and_bound_frontier(branching_threshold={args.threshold}), n_iter {N_ITER}, "
                   f"lr {LR}, BaB eps {EPS_BAB}, each side on both libraries, alternating.  The bar: tree / parent - 1 <= three times the larger spread",
           "device": libs["tree"].info["device"], "library_build_id": libs["tree"].info["library_build_id"],
           "parent_commit_library_build_id": libs["parent"].info["library_build_id"], "tile": S, "kernel": [], "frontier": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        rec["every_size_within_the_bar"] = all(v["within_the_bar"] for e in rec["kernel"] + rec["frontier"] for v in e["against_parent"].values())
        rec["every_result_identical"] = all(e["identical"] for e in rec["kernel"] + rec["frontier"])
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    try:
        if args.skip != "kernel":
            for B in [int(b) for b in args.bs.split(",")]:
                for n in [S if n == "S" else int(n) for n in args.starts.split(",")]:
                    size = {"B": B, "n_starts": n, "calls": args.calls}
                    digests = {lib: w.ask({"what": "walk_setup", **size})["results_sha256"] for lib, w in libs.items()}
                    ms = {lib: {} for lib in libs}
                    for _ in range(args.repeats):                         # alternating
                        for lib, w in libs.items():
                            for call, v in w.ask({"what": "walk_repeat", "calls": args.calls}).items():
                                ms[lib].setdefault(call, []).append(v)
                    entry = {"B": B, "n_starts": n, "points": B * n, "identical": digests["tree"] == digests["parent"],
                             "ms": {lib: {call: spread(v) for call, v in m.items()} for lib, m in ms.items()}}
                    entry["against_parent"] = {call: against(entry["ms"]["tree"][call], entry["ms"]["parent"][call]) for call in entry["ms"]["tree"]}
                    rec["kernel"].append(entry)
                    print(json.dumps(entry), flush=True)
                    save()
        if args.skip != "frontier":
            same = ("global_lb", "global_ub", "domains_bounded", "rounds", "stop", "kw_pairs_bounded", "kw_pairs_used", "same_result_in_every_repeat")
            for K, rounds in zip([int(k) for k in args.ks.split(",")], [int(r) for r in args.rounds.split(",")]):
                common = (K, rounds, args.capacity, args.threshold)
                entry = {"K": K, "max_rounds": rounds, "sides": {}, "against_parent": {}, "identical": True}
                for side, options in sides.items():
                    for w in libs.values():                               # warm-up: allocations, first launches
                        w.run(K, min(rounds, 4), args.capacity, args.threshold, options)
                    runs = {lib: [] for lib in libs}
                    for _ in range(args.repeats):                         # alternating
                        for lib, w in libs.items():
                            runs[lib].append(w.run(*common, options))
                    sums = {lib: summary(r) for lib, r in runs.items()}
                    entry["sides"][side] = sums
                    entry["against_parent"][side] = against(sums["tree"]["ms_per_round"], sums["parent"]["ms_per_round"])
                    entry["identical"] = entry["identical"] and all(sums["tree"][k] == sums["parent"][k] for k in same)
                rec["frontier"].append(entry)
                print(json.dumps(entry), flush=True)
                save()
    finally:
        for w in libs.values():
            w.close()
    print("written", args.out, "every size within the bar:", rec.get("every_size_within_the_bar"), "identical:", rec.get("every_result_identical"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's library (tools/mklib.sh): the record of the one-template walk, this tree against it")
    ap.add_argument("--worker", help="(internal) serve runs on the tree at this path")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_starts_timing.json"))
    ap.add_argument("--bs", default="2,32,128")
    ap.add_argument("--starts", default="S,17,65")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--ks", default="1,16,64")
    ap.add_argument("--rounds", default="60,40,30")
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=8192, help="slots of the pool")
    ap.add_argument("--skip", default="", help="'kernel' or 'frontier': leave that part out")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    if args.parent_lib:
        return refactor(args)
    new = Worker(ROOT)
    old = Worker(os.path.abspath(args.parent_tree)) if args.parent_tree and args.skip != "frontier" else None
    S = new.ask({"what": "tile"})["tile"]
    sides = {"off": {}, "pgd4": {"witness": True, "pgd_steps": 4}, "pgd4_r16": {"witness": True, "pgd_steps": 4, "pgd_restarts": 16},
             "pgd0_r64": {"witness": True, "pgd_steps": 0, "pgd_restarts": 64}}
    rec = {"what": f"{NET}, eps {EPS}, property 3 vs 5.  kernel: gnnb_net_descend_starts (S = {S} starts per workgroup) against gnnb_net_descend on the "
                   f"same B * n_starts points as a flat batch, {STEPS} steps of 1/64, root-box rows; ms per call, wall clock on the host around {args.calls} "
                   f"back-to-back calls; one warm-up, {args.repeats} repeats per side, the sides alternating; median, min / max and the A/A spread "
                   f"(max - min) / median.  frontier: branch_and_bound_frontier(branching_threshold={args.threshold}), n_iter {N_ITER}, lr {LR}, BaB eps "
                   f"{EPS_BAB}: the parent commit, the options off, witness with pgd_steps 4, the same with 16 restarts, pgd_steps 0 with 64 restarts; "
                   f"one warm-up run per side, then {args.repeats} repeats per side, the sides alternating",
           "device": new.info["device"], "library_build_id": new.info["library_build_id"],
           "parent_commit_library_build_id": old.info["library_build_id"] if old else None, "tile": S, "pool_capacity": args.capacity,
           "branching_threshold": args.threshold, "kernel": [], "frontier": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    try:
        if args.skip != "kernel":
            for B in [int(b) for b in args.bs.split(",")]:
                for n in [S if n == "S" else int(n) for n in args.starts.split(",")]:
                    entry = new.ask({"what": "kernel", "B": B, "n_starts": n, "calls": args.calls, "repeats": args.repeats})
                    rec["kernel"].append(entry)
                    print(json.dumps(entry), flush=True)
                    save()
        if args.skip != "frontier":
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
                    width = p["ms_per_round"]["aa_spread"]
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
                save()
    finally:
        new.close()
        if old:
            old.close()
    print("written", args.out)


if __name__ == "__main__":
    main()
