#!/usr/bin/env python3
"""What the replay buffer costs, on one MI355X -> profiles/replay_timing.json.

tools/imitation_timing.py's problem (cifar_base_kw, eps 0.09, the seeded N(0,1) image, property 3 vs 5, n_iter 20, lr 0.1, BaB eps 1e-4,
strong_candidates 16, K = --K), every run from the checkpoint's parameters and a fresh optimizer.  Three measurements, one session:

  round    wall ms per round of ``branch_and_bound_frontier`` with ``imitate=1`` against ``imitate=Replay(every=1, steps=1, batch=K)``, for
           "gnn" and "strong" and both repack modes, the sides alternating: every round is a learning round, so the difference is the
           push, the 16-byte read, the draw and a step on min(K, filled) drawn rows instead of the round's own k.
  kernels  ``gnnb_replay_push`` (16 rows of a synthetic batch, all stored, into C = 4096) and ``gnnb_replay_sample`` (n = 8 of filled =
           1024; n = 256 of filled = 65536) alone, HIP-event time per call over --calls calls.
  off      with --parent-tree (a checkout of the parent commit with its library built, served by a worker process of its own): the option
           OFF -- a plain "gnn" run and an ``imitate=1`` run -- on this tree and on the parent's, alternating; "within_spread" says whether
           this tree's median lies inside the min..max of the parent's repeats, "ranges_overlap" whether the two min..max ranges meet.

One warm-up run per side, then --repeats runs per side; median and min / max over the runs; both build ids.

    python tools/replay_timing.py [--parent-tree DIR] [--repeats 5] [--rounds 8] [--K 4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES = 16


# ---- the worker: one tree, one process, one run per line of stdin ---------------------------------------------------------------------
def worker(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from gnn_branching_amd import _lib, frontier, lp_producer, nets, synth
    from gnn_branching_amd.engine import make_batch
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice
    from tools.frontier_online_timing import CKPT, EPS, EPS_BAB, LR, N_ITER, NET, reset
    torch.set_num_threads(16)
    layers = nets.load_verified_net(NET, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    lp0 = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS)
    choice = GraphChoice([torch.zeros(int(np.prod(lp0.shapes[i + 1]))) for i in lp0.pre_relu_indices], CKPT)
    choice.verbose = False
    eng = choice._eng()
    w0 = eng.get_weights().copy()
    lp = lp_producer.LayerGraphLP(layers, x - EPS, x + EPS, bounds="kw_device", engine=eng)
    eng.bind(list(layers[:-1]), (3, 32, 32))
    has_replay = hasattr(frontier, "Replay")
    print(json.dumps({"ready": True, "device": torch.cuda.get_device_name(), "library_build_id": _lib.library_build_id(), "replay": has_replay}), flush=True)

    def run(cmd):
        reset(choice, w0)
        stamps, stats, K = [], {}, cmd["K"]
        extra = {}
        if cmd["imitate"] == "replay":
            extra["imitate"] = frontier.Replay(every=1, capacity=1024, batch=K, steps=1)
        elif cmd["imitate"]:
            extra["imitate"] = cmd["imitate"]
        if extra or cmd["branching"] == "strong":
            extra["strong_candidates"] = CANDIDATES
        if cmd.get("repack"):
            extra["repack"] = cmd["repack"]
        glb, gub, done, bounded, reason = frontier.branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                                                                             max_rounds=cmd["rounds"], capacity=8192, stats=stats, branching=cmd["branching"],
                                                                             log=lambda s: stamps.append(time.perf_counter()), **extra)
        return {"ms_per_round": 1e3 * (stamps[-1] - stamps[0]) / max(done, 1), "rounds": done, "global_lb": glb, "stop": reason,
                "imitation_steps": stats.get("imitation_steps", 0), "imitation_rows": stats.get("imitation_rows", 0), "replay_stored": stats.get("replay_stored")}

    def kernels(cmd):
        dev, calls = eng.device, cmd["calls"]
        batch = synth.make_batch(NET, 16, seed=31)
        m = eng._marshal(*batch.forward_args())
        cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
        masks = batch.masks.numpy()
        g, tab = np.random.RandomState(7), np.full(masks.shape, float("nan"))
        for b in range(16):
            idx = g.choice(np.flatnonzero(masks[b]), size=CANDIDATES, replace=False)
            tab[b, idx] = g.uniform(0.0, 1.0, idx.size)
        table, rows = torch.from_numpy(tab).to(dev), torch.arange(16, dtype=torch.int32, device=dev)
        buf = frontier.ReplayBuffer(eng, 4096)
        idx = torch.zeros(256, dtype=torch.int32, device=dev)

        def timed(f):
            f()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                f()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / calls
        out = {"push_16_rows_ms": timed(lambda: buf.push(cb, 16, rows, 16, table)), "bytes_per_entry": eng.replay_bytes(1)}
        assert buf.read_state()[2:] == [16, 0]
        state = torch.tensor([0, 1024, 0, 0], dtype=torch.int32).to(dev)
        out["sample_8_of_1024_ms"] = timed(lambda: eng.replay_sample(state, 4096, 8, 1, 2, idx))
        state[1] = 65536
        out["sample_256_of_65536_ms"] = timed(lambda: eng.replay_sample(state, 65536, 256, 1, 2, idx))
        return out

    for line in sys.stdin:
        cmd = json.loads(line)
        with torch.cuda.device(eng.device):
            out = run(cmd) if cmd["what"] == "run" else kernels(cmd)
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

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        return self._read()

    def close(self):
        self.p.stdin.close()
        self.p.wait()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def alternating(sides, repeats, rounds):
    """sides: {name: (worker, command)}; one warm-up run per side, then ``repeats`` rounds of runs with the sides alternating."""
    for w, cmd in sides.values():
        w.ask(what="run", **{**cmd, "rounds": min(rounds, 3)})
    runs = {name: [] for name in sides}
    for _ in range(repeats):
        for name, (w, cmd) in sides.items():
            runs[name].append(w.ask(what="run", rounds=rounds, **cmd))
    return {name: {"ms_per_round": spread([r["ms_per_round"] for r in rs]), **{k: rs[-1][k] for k in rs[-1] if k != "ms_per_round"}} for name, rs in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", help="(internal) serve runs on the tree at this path")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_timing.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--K", type=int, default=4)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    if args.repeats < 3:
        ap.error("--repeats: at least 3 runs per side")
    new = Worker(ROOT)
    old = Worker(os.path.abspath(args.parent_tree)) if args.parent_tree else None
    rec = {"what": f"cifar_base_kw, shipped checkpoint, eps 0.09, property 3 vs 5, K {args.K}, strong_candidates {CANDIDATES}, {args.rounds} rounds per run, "
                   f"{args.repeats} runs per side after one warm-up, the sides alternating; wall ms per round (median, min / max over the runs).  round: "
                   "imitate=1 against imitate=Replay(every=1, steps=1, batch=K).  kernels: HIP-event ms per call.  off: this tree against the parent "
                   "commit's checkout and library, the option off",
           "device": new.info["device"], "library_build_id": new.info["library_build_id"],
           "parent_commit_library_build_id": old.info["library_build_id"] if old else None, "round": [], "kernels": None, "off": None}
    try:
        for branching in ("gnn", "strong"):
            for repack in ("host", "device"):
                base = {"branching": branching, "repack": repack, "K": args.K}
                entry = {"branching": branching, "repack": repack,
                         **alternating({"imitate_1": (new, {**base, "imitate": 1}), "replay": (new, {**base, "imitate": "replay"})}, args.repeats, args.rounds)}
                entry["difference_ms"] = round(entry["replay"]["ms_per_round"]["median"] - entry["imitate_1"]["ms_per_round"]["median"], 4)
                rec["round"].append(entry)
                print(json.dumps(entry), flush=True)
        rec["kernels"] = {k: round(v, 5) for k, v in new.ask(what="kernels", calls=args.calls).items()}
        print(json.dumps(rec["kernels"]), flush=True)
        if old:
            rec["off"] = []
            for branching, imitate in (("gnn", None), ("strong", None), ("gnn", 1)):
                cmd = {"branching": branching, "imitate": imitate, "K": args.K}
                entry = {"branching": branching, "imitate": imitate, **alternating({"this_tree": (new, cmd), "parent": (old, cmd)}, args.repeats, args.rounds)}
                a, b = entry["this_tree"]["ms_per_round"], entry["parent"]["ms_per_round"]
                entry["within_spread"] = bool(b["min"] <= a["median"] <= b["max"])
                entry["ranges_overlap"] = bool(a["min"] <= b["max"] and b["min"] <= a["max"])
                entry["same_result"] = entry["this_tree"]["global_lb"] == entry["parent"]["global_lb"]
                rec["off"].append(entry)
                print(json.dumps(entry), flush=True)
    finally:
        new.close()
        if old:
            old.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
