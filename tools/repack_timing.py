#!/usr/bin/env python3
"""What a learning step costs with the scorer's packs rebuilt on the host (repack mode 0) and on the device (mode 1; DESIGN.md section
7.15), on one MI355X -> profiles/repack_timing.json.

Two measurements:
  step    gnnb_online_step_rows at n = 1 on cifar_base_kw (one subproblem, apply = 1), per call:
            call_ms    host wall time of the call itself (mode 0 ends in its own stream synchronisations, mode 1 only issues the launches);
            event_ms   HIP-event time on the stream from in front of the first launch to behind the last (behind the pack rebuild);
            done_ms    host wall time from the call to the end of a stream synchronise behind it (what a caller who waits pays).
  repack  gnnb_repack alone (k_repack_fold + k_repack_emit), HIP-event time of the pair.  (The two launches have no profile class of
          their own -- the class list is pinned -- so gnnb_profile_enable does not see them.)
Sides, in one session, alternating: mode 0 and mode 1 of this tree, and with --parent-tree (a checkout of the parent commit with its
library built, served by a worker process of its own) the parent's step, which has the host rebuild only.  One warm-up run per side,
then --repeats runs per side of --calls calls each; a run's figure is the median over its calls; the record holds the median and
min / max over the runs, and both build ids.

    python tools/repack_timing.py [--parent-tree DIR] [--repeats 5] [--calls 40]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET, SEED, LR, WD = "cifar_base_kw", 7, 1e-4, 1e-4


# ---- the worker: one tree, one process, one run per line of stdin ---------------------------------------------------------------------
def worker(tree):
    sys.path.insert(0, tree)
    import ctypes as C
    import numpy as np
    import torch
    from gnn_branching_amd import _lib, nets, synth
    from gnn_branching_amd.engine import ScorerEngine, make_batch
    torch.set_num_threads(16)
    d = dict(np.load(os.path.join(nets.ASSETS, "cifar_trained_gnn.npz")))
    state = {k: d[k] for k in [str(k) for k in d.pop("__order__")]}
    eng = ScorerEngine(state, T=2)
    eng.online_create(LR, WD)
    dev = eng.device
    batch = synth.make_batch(NET, 1, seed=SEED)
    m = eng._marshal(*batch.forward_args())
    cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
    scored = batch.masks[0].reshape(-1).nonzero().view(-1)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = torch.tensor([int(scored[len(scored) // 2])], dtype=torch.int32, device=dev)
    imp = torch.tensor([0.1], dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    w0 = eng.get_weights().copy()
    has_modes = hasattr(eng, "set_repack")
    print(json.dumps({"ready": True, "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "repack_modes": has_modes,
                      "relu_nodes": int(eng.R), "scored_nodes": int(scored.numel())}), flush=True)

    def timed(call, n):
        out = {"call_ms": [], "event_ms": [], "done_ms": []}
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out["call_ms"].append(1e3 * (t1 - t0))
            out["done_ms"].append(1e3 * (t2 - t0))
            out["event_ms"].append(a.elapsed_time(b))
        return {k: statistics.median(v) for k, v in out.items()}

    def step():
        eng.online_step_rows(cb, 1, rows, kw, imp, loss=loss, status=status, apply=True)

    for line in sys.stdin:
        cmd = json.loads(line)
        with torch.cuda.device(dev):
            if cmd["what"] == "step":
                if has_modes:
                    eng.set_repack("device" if cmd["mode"] == 1 else "host")
                eng.set_weights(w0)                               # every run starts from the same parameters
                out = timed(step, cmd["calls"])
                out["status"] = int(status.cpu()[0])
                out["loss_finite"] = bool(torch.isfinite(loss).all())
            else:
                out = timed(eng.repack, cmd["calls"])
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

    def run(self, what, calls, mode=None):
        self.p.stdin.write(json.dumps({"what": what, "calls": calls, "mode": mode}) + "\n")
        self.p.stdin.flush()
        return self._read()

    def close(self):
        self.p.stdin.close()
        self.p.wait()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", help="(internal) serve runs on the tree at this path")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repack_timing.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    if args.repeats < 3:
        ap.error("--repeats: at least 3 runs per side")
    new = Worker(ROOT)
    old = Worker(os.path.abspath(args.parent_tree)) if args.parent_tree else None
    sides = [("mode0", new, 0), ("mode1", new, 1)] + ([("parent", old, None)] if old else [])
    try:
        for _, w, mode in sides:                                  # warm-up: allocations, first launches
            w.run("step", 3, mode)
        new.run("repack", 3)
        runs = {name: [] for name, _, _ in sides}
        repack = []
        for _ in range(args.repeats):
            for name, w, mode in sides:
                runs[name].append(w.run("step", args.calls, mode))
            repack.append(new.run("repack", args.calls))
    finally:
        new.close()
        if old:
            old.close()
    assert all(r["status"] == 0 and r["loss_finite"] for rs in runs.values() for r in rs), "a step was refused"
    rec = {"what": f"gnnb_online_step_rows (n = 1, apply = 1) on {NET}, shipped checkpoint, one subproblem of {new.info['scored_nodes']} scored nodes: repack mode 0 "
                   f"(host builder), mode 1 (device builder) and the parent commit's library, alternating in one session; one warm-up run per side, then "
                   f"{args.repeats} runs per side of {args.calls} calls each; a run's figure is the median over its calls; median and min / max over the runs.  "
                   "call_ms: host wall time of the call; event_ms: HIP-event time from in front of the first launch to behind the last; done_ms: host wall "
                   "time from the call to the end of a stream synchronise behind it.  repack_alone: gnnb_repack (k_repack_fold + k_repack_emit), the same figures.",
           "device": new.info["device"], "library_build_id": new.info["library_build_id"],
           "parent_commit_library_build_id": old.info["library_build_id"] if old else None,
           "step": {name: {k: spread([r[k] for r in rs]) for k in ("call_ms", "event_ms", "done_ms")} for name, rs in runs.items()},
           "repack_alone": {k: spread([r[k] for r in repack]) for k in ("call_ms", "event_ms", "done_ms")}}
    if old:
        a, b = rec["step"]["mode0"]["done_ms"], rec["step"]["parent"]["done_ms"]
        rec["mode0_within_the_spread_of_the_parent"] = bool(a["min"] <= b["max"] and b["min"] <= a["max"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
