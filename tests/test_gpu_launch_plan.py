"""The launch plan of gnnb_forward, pinned: for every network, batch size, handle option and half-pass limit below, the kernel
classes one forward launches (in launch order, from gnnb_profile_trace), gnnb_describe and gnnb_workspace_bytes must equal
tests/golden/forward_launch_plans.json.  Every option is its own implementation of the same scores (the parity tests compare them);
this test pins WHICH launches each one makes, so that a change to the host orchestration cannot move work between kernels unseen.

Recording (GPU; GNNB_LIB selects the library to record from, e.g. the parent revision's build):
    python -m tests.test_gpu_launch_plan
"""
import json
import os
from functools import lru_cache

import pytest
import torch

from tests.common import ARCHS, GOLDEN, random_state, register_toy_archs

GOLDEN_FILE = os.path.join(GOLDEN, "forward_launch_plans.json")

CIFAR = ["cifar_base_kw", "cifar_wide_kw", "cifar_deep_kw"]
NET_BATCHES = {**{n: (1, 40, 200) for n in CIFAR}, **{n: (1, 40) for n in ARCHS}}     # B = 200 > TOP_SPLIT_MAXB
# each option on its own, away from its default ("gather" and "dense_lds" shape the bind: a fresh engine per setting)
SETTINGS = {"default": {}, **{f"{k}={v}": {k: v} for k, v in (
    ("bf3", 0), ("fuse", 0), ("top", 0), ("gather", 0), ("embed_fuse", 0), ("dense_lds", 0), ("tail_max_b", 0), ("top_split", 1),
    ("top_fuse_upd", 0), ("clspre_max_b", 0))}}
LIMIT_NETS = ("cifar_base_kw", "toy_conv3")      # half-pass limits 1..4 (inspection runs) on the defaults
GROUPS = [(net, s) for net in NET_BATCHES for s in SETTINGS]


@lru_cache(None)
def _batch(net, B):
    from gnn_branching_amd import synth
    return synth.make_batch(net, B, seed=5)


def _trace(eng, args):
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True)
        eng.profile_trace(65536)
        with torch.no_grad():
            eng.forward(*args).check()
        eng.profile_read(reset=True)
        return [c for c, _ in eng.profile_trace(65536)]
    finally:
        eng.profile_enable(False)


def record(net, setting):
    """{describe, cases: {"B=..[,limit=..]": {trace, workspace_bytes}}} of one network under one option setting, or {bind_error}."""
    from gnn_branching_amd.engine import ScorerEngine
    register_toy_archs()
    eng = ScorerEngine(random_state(), options=SETTINGS[setting])
    out = {"cases": {}}
    for B in NET_BATCHES[net]:
        args = _batch(net, B).forward_args()
        try:
            eng.bind(args[5]["fixed_layers"], tuple(args[0][0].shape[1:]))
        except RuntimeError as e:
            return {"bind_error": str(e)}
        out["describe"] = eng.describe()
        limits = (0, 1, 2, 3, 4) if setting == "default" and net in LIMIT_NETS else (0,)
        for n in limits:
            eng.set_halfpass_limit(n)
            try:
                trace = _trace(eng, args)
            finally:
                eng.set_halfpass_limit(0)
            out["cases"][f"B={B}" + (f",limit={n}" if n else "")] = {
                "trace": trace, "workspace_bytes": int(eng.lib.gnnb_workspace_bytes(eng.h, B))}
    return out


@lru_cache(None)
def _golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("net,setting", GROUPS, ids=[f"{n}-{s}" for n, s in GROUPS])
def test_forward_launch_plan_matches_golden(net, setting):
    want = _golden()[f"{net}|{setting}"]
    got = record(net, setting)
    for case, w in want.get("cases", {}).items():
        assert got.get("cases", {}).get(case) == w, case
    assert got == want


if __name__ == "__main__":
    torch.cuda.set_device(0)
    golden = {f"{net}|{s}": record(net, s) for net, s in GROUPS}
    with open(GOLDEN_FILE, "w") as f:
        json.dump(golden, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{GOLDEN_FILE}: {len(golden)} groups, {sum(len(g.get('cases', {})) for g in golden.values())} forwards")
