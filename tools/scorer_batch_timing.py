#!/usr/bin/env python
"""Host-side cost of the scorer's batch plumbing, this tree against another checkout of the project (GPU box).

Everything that feeds gnnb_forward checks and marshals its batch on the host in front of the launches; this times those paths on
cifar_base_kw with the shipped GNN, after warm-up, wall clock on the host:

    forward_host B = 1, 2      ms per call (synchronous: the BaB loop's per-decision call)
    forward_host B = 256       ms per call (the staging block is copied by the handle's helper threads)
    hostfed pageable / pinned  ms per HostFedPipeline.submit, compact, B = 256, a stream of submits synchronised once at the end
    forward enqueue B = 1      ms of host time to enqueue one device-resident forward (no synchronisation inside the timed region)
    bench.py                   its own ms_per_step (--steps 20 --warmup 3)

With --parent DIR (a built checkout of the commit to compare against) the two trees run alternately, --runs times each, every run a
fresh process; per figure the median and the spread (max - min) of each side, and whether this tree is slower than the parent by more
than three times the larger spread.

    python tools/scorer_batch_timing.py --parent ../parent [--out profiles/scorer_batch_refactor_timing.json] [--runs 3]
    python tools/scorer_batch_timing.py --one [--tree DIR]          # one run of one tree: a JSON line
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = "cifar_base_kw"


def one(tree):
    sys.path.insert(0, tree)
    import torch
    from gnn_branching_amd import _lib, engine as E, synth
    from tests.common import shipped_state
    torch.set_num_threads(16)
    eng = E.ScorerEngine(shipped_state())
    out = {"library_build_id": _lib.library_build_id()}

    def per_call(f, n, warm):
        for _ in range(warm):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 5)

    for B, n in ((1, 400), (2, 400), (256, 20)):
        args = synth.make_batch(NET, B, seed=7).forward_args()
        out[f"forward_host_B{B}_ms"] = per_call(lambda: eng.forward_host(*args), n, 5)
    big = synth.make_batch(NET, 256, seed=8).forward_args()
    pinned = [[t.pin_memory() for t in g] if isinstance(g, list) else g for g in big]
    pinned[4], pinned[6] = big[4].pin_memory(), big[6].pin_memory()
    with torch.no_grad():
        for name, args in (("pageable", big), ("pinned", pinned)):
            pipe = E.HostFedPipeline(eng, compact=True)
            out[f"hostfed_{name}_B256_ms"] = per_call(lambda: pipe.submit(*args), 30, 5)
        a = synth.make_batch(NET, 1, seed=9).forward_args()
        dev = [[t.to(eng.device) for t in g] if isinstance(g, list) else g for g in a]
        dev[4], dev[6] = a[4].to(eng.device), a[6].to(eng.device)
        for _ in range(5):
            eng.forward(*dev)
        spent = 0.0
        for _ in range(20):                       # 20 forwards enqueued, then the queue drained outside the timed region
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                eng.forward(*dev)
            spent += time.perf_counter() - t0
        torch.cuda.synchronize()
        out["forward_enqueue_B1_ms"] = round(1e3 * spent / 400, 5)
    print(json.dumps(out), flush=True)


def child(tree, argv):
    r = subprocess.run([sys.executable] + argv, cwd=tree, stdout=subprocess.PIPE, text=True, check=True)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scorer_batch_refactor_timing.json"))
    args = ap.parse_args()
    if args.one:
        return one(os.path.abspath(args.tree))
    sides = {"this": ROOT}
    if args.parent:
        sides = {"parent": os.path.abspath(args.parent), "this": ROOT}
    runs = {s: [] for s in sides}
    for _ in range(args.runs):
        for side, tree in sides.items():          # alternating
            rec = child(tree, [os.path.abspath(__file__), "--one", "--tree", tree])
            b = child(tree, ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"])
            rec["bench_ms_per_step"] = b["ms_per_step"]
            runs[side].append(rec)
            print(side, json.dumps(rec), flush=True)
    table = {}
    for key in [k for k in runs["this"][0] if k.endswith("_ms") or k == "bench_ms_per_step"]:
        row = {s: {"median": statistics.median(r[key] for r in runs[s]), "spread": round(max(r[key] for r in runs[s]) - min(r[key] for r in runs[s]), 5),
                   "runs": [r[key] for r in runs[s]]} for s in sides}
        if args.parent:
            bar = 3 * max(row["parent"]["spread"], row["this"]["spread"])
            row["this_minus_parent"] = round(row["this"]["median"] - row["parent"]["median"], 5)
            row["bar_3x_larger_spread"] = round(bar, 5)
            row["slower_beyond_bar"] = row["this_minus_parent"] > bar
        table[key] = row
    import torch
    rec = {"what": f"host wall clock per call on {NET}, shipped GNN, after warm-up; {args.runs} fresh processes per side, the sides alternating; "
                   "median and spread (max - min) over the processes; bar: this tree no slower than the parent by more than 3x the larger spread",
           "device": torch.cuda.get_device_name(), "library_build_id": {s: runs[s][0]["library_build_id"] for s in sides}, "table": table}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(table, indent=1))
    print("written", args.out)


if __name__ == "__main__":
    main()
