"""k_top derives the liveness of layer L's nodes once, keeps W_prop[b] in LDS and has the property node's operands requested ahead of
their use, with the hidden layer's k-split on waves 4..7 (gnnb_k_edges.h top_sample).  None of it changes a sum, so on the same batch, on a
NaN-poisoned workspace:
  * the default handle gives, for one, two and four workgroups per sample (option top_split), scores, decisions and status IDENTICAL to
    those the commit before this change gave: tests/golden/top_roundtrips/<case>.npz holds each case's batch (in the layout of
    tests/common.py load_golden) and what that commit's library returned for it on an MI355X (`parent_scores`, `parent_decisions`,
    `parent_status`; S = 1, 2, 4 were equal there).  The fixtures are written by `python -m tests.test_gpu_top_roundtrips DIR` with the library
    to be pinned loaded; they change only with a change that is meant to move a sum.
  * the handle that runs the top of the network as its separate kernels (option top = 0, as
    test_gpu_parity.py::test_separate_top_kernels_path_matches) gives the same status and decisions and scores within 4e-7.  That twin is
    other arithmetic (the separate dense kernels add in another order), so it cannot be bit-equal: it is a second fp32 evaluation of scores
    that lie in [-1, 0.05], and two such evaluations differ by the fp32 noise tests/common.py states for these weights (2-4e-7, the
    reference's own).  On the commit before this change the two differed in 2-340 of a case's scores by at most 1.2e-7.

Networks: conv, conv, Linear (K -> N), Linear, so that the last ReLU layer hangs on a Linear edge, k_top runs and carries the backward update
of layer L-1 (L = 3).  K = 8 H W nodes in layer L-1:
  K = 40     under one wave of the list build's 512-node pass
  K = 512    exactly one 512-node pass
  K = 520    a second pass of 8 nodes; no multiple of 32 or 64
  K = 1000   two passes, no multiple of 32 or 64
N = 1, 100, 128 nodes in layer L (one node; the CIFAR size; every lane of the update waves), B = 1 and 3.
Bounds of layers L-1 and L are overwritten per sample (PATTERNS): all dead (K_eff = 0), all live, one live node at index 0, one at index
K - 1, a run of lb = ub = 0 nodes (live by the predicate; their ratio is 0/0), a run of lb < 0 = ub nodes (dead), and one NaN upper bound.
lb = ub = 0 and NaN make embeddings NaN in the reference as here: every handle then raises status bit 0 and NaN counts as equal."""
from functools import lru_cache

import os

import numpy as np
import pytest
import torch

from gnn_branching_amd import nets, synth
from gnn_branching_amd.engine import _or_reduce
from tests.common import GOLDEN, load_golden, state_of
from tests.test_gpu_blocktap import PROPS

gpu = pytest.mark.gpu
SHAPES = {40: (1, 5), 512: (8, 8), 520: (5, 13), 1000: (5, 25)}          # K = 8 H W
NS = (1, 100, 128)
PATTERNS = ("dead", "live", "first", "last", "zero", "neg0", "nan", "mixed")


def arch_name(K, N):
    return f"trt_K{K}_N{N}"


def register():
    for i, (K, (H, W)) in enumerate(SHAPES.items()):
        for j, N in enumerate(NS):
            spec = [("conv", 3, 8, 3, 1, 1), ("relu",), ("conv", 8, 8, 3, 1, 1), ("relu",), ("flatten",), ("linear", K, N), ("relu",), ("linear", N, 10)]
            nets.register_arch(arch_name(K, N), spec, seed=900 + 10 * i + j)


# case -> (K, N, B, patterns of layer L-1 by sample, patterns of layer L by sample)
CASES = {}
for K in SHAPES:
    CASES[f"K{K}_N100_B3_a"] = (K, 100, 3, ("dead", "live", "first"), ("live", "mixed", "dead"))
    CASES[f"K{K}_N100_B3_b"] = (K, 100, 3, ("last", "zero", "neg0"), ("mixed", "live", "mixed"))
    CASES[f"K{K}_N100_B1"] = (K, 100, 1, ("mixed",), ("mixed",))
    CASES[f"K{K}_N128_B3"] = (K, 128, 3, ("mixed", "last", "live"), ("dead", "mixed", "live"))
    CASES[f"K{K}_N1_B3"] = (K, 1, 3, ("first", "mixed", "dead"), ("live", "dead", "live"))
CASES["K520_N100_B3_nan"] = (520, 100, 3, ("mixed", "nan", "live"), ("mixed", "mixed", "nan"))
CASES["K1000_N128_B1_nan"] = (1000, 128, 1, ("nan",), ("zero",))
CASES["K40_N1_B1_dead"] = (40, 1, 1, ("dead",), ("dead",))
HAS_NAN = {c for c, v in CASES.items() if {"zero", "nan"} & (set(v[3]) | set(v[4]))}


def is_live(lb, ub):
    """node_is_live of gnnb_k_gather.h: not blocked (a NaN upper bound counts as live)."""
    return ~(ub <= 0) | (lb >= 0)


def paint(lb, ub, pattern, rng):
    """Overwrite one sample's flat bounds of one layer (views into the batch) with a pattern."""
    n = lb.numel()
    if pattern in ("dead", "first", "last"):
        lb[:], ub[:] = -1.0, -0.25
        if pattern == "first":
            lb[0], ub[0] = -0.5, 0.25
        if pattern == "last":
            lb[n - 1], ub[n - 1] = -0.5, 0.25
    elif pattern == "live":
        dead = ~is_live(lb, ub)
        lb[dead], ub[dead] = -0.5, 0.25
    else:                                                       # mixed, with a run of special nodes in it
        dead = torch.from_numpy(rng.uniform(size=n) < 0.45)
        lb[dead], ub[dead] = -1.0, -0.25
        fix = ~dead & ~is_live(lb, ub)
        lb[fix], ub[fix] = -0.5, 0.25
        lo, hi = n // 3, n // 3 + max(1, n // 8)
        if pattern == "zero":
            lb[lo:hi], ub[lo:hi] = 0.0, 0.0                     # live, ratio 0/0
        if pattern == "neg0":
            lb[lo:hi], ub[lo:hi] = -1.0, 0.0                    # dead
        if pattern == "nan":
            ub[n // 2] = float("nan")                            # live


TWIN_ATOL = 4e-7              # see the module docstring


@lru_cache(None)
def golden_of(case):
    register()
    return load_golden("top_roundtrips/" + case)


def batch_of(case):
    return golden_of(case)[1]


def synth_batch(case):
    """The case's batch as the fixtures were made from it (write_golden)."""
    register()
    K, N, B, pat_m, pat_l = CASES[case]
    H, W = SHAPES[K]
    rng = np.random.RandomState(sum(map(ord, case)))
    batch = synth.make_batch(arch_name(K, N), B, seed=int(rng.randint(1 << 20)), eps=0.02, props=(PROPS * 2)[:B], input_shape=(3, H, W))
    for k, pats in ((2, pat_m), (3, pat_l)):
        lb, ub = batch.lower_bounds_all[k].reshape(B, -1), batch.upper_bounds_all[k].reshape(B, -1)
        for b in range(B):
            paint(lb[b], ub[b], pats[b], rng)
    for k, m in enumerate(batch.bab_masks):
        l2, u2 = batch.lower_bounds_all[k + 1].reshape(B, -1), batch.upper_bounds_all[k + 1].reshape(B, -1)
        m.zero_()
        m[(l2 < 0) & (u2 > 0)] = -1
        m[l2 >= 0] = 1
    batch.masks = torch.cat([(m == -1).float() for m in batch.bab_masks], 1)
    return batch


@pytest.mark.parametrize("case", list(CASES))
def test_batches_hold_the_patterns(case):
    """Conditions on the inputs (CPU): layer sizes and, per pattern, the live set it promises."""
    batch = batch_of(case)
    K, N, B, pat_m, pat_l = CASES[case]
    for k, size, pats in ((2, K, pat_m), (3, N, pat_l)):
        lb, ub = batch.lower_bounds_all[k].reshape(B, -1), batch.upper_bounds_all[k].reshape(B, -1)
        assert lb.shape[1] == size
        live = is_live(lb, ub).numpy()
        for b, p in enumerate(pats):
            lo, hi = size // 3, size // 3 + max(1, size // 8)
            if p == "dead":
                assert not live[b].any()
            elif p == "live":
                assert live[b].all()
            elif p == "first":
                assert live[b, 0] and live[b].sum() == 1
            elif p == "last":
                assert live[b, size - 1] and live[b].sum() == 1
            elif p == "zero":
                assert live[b, lo:hi].all() and (lb[b, lo:hi] == 0).all() and (ub[b, lo:hi] == 0).all()
            elif p == "neg0":
                assert not live[b, lo:hi].any() and (ub[b, lo:hi] == 0).all()
            elif p == "nan":
                assert np.isnan(ub[b, size // 2].item()) and live[b, size // 2]
            if p in ("zero", "neg0", "nan", "mixed") and size >= 40:
                assert live[b].any() and not live[b].all()


HANDLES = {"default": {}, "top0": {"top": 0}}


def run_case(case, handle, S, batch=None):
    """{scores, decisions, status, kernels} of one case on one handle: a forward on a NaN-poisoned workspace."""
    from gnn_branching_amd.engine import ScorerEngine
    batch = batch_of(case) if batch is None else batch
    B = batch.batch_size
    eng = ScorerEngine(state_of("random"), options=dict(HANDLES[handle], top_split=S))
    with torch.no_grad():
        eng.forward(*batch.forward_args())                                  # (binds the network, allocates the workspace)
        torch.cuda.synchronize()
        eng.workspace(B).view(torch.float32).fill_(float("nan"))            # exchange buffers and counters included
        res = eng.forward(*batch.forward_args())
        torch.cuda.synchronize()
    return {"scores": res.scores.cpu().numpy(), "decisions": res.decisions.cpu().numpy(), "status": _or_reduce(res.status),
            "kernels": [u["kernel"] for u in eng.describe()["updates"]]}


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_default_is_the_parent_bit_for_bit_and_close_to_the_separate_kernels(case):
    nan = case in HAS_NAN
    g = golden_of(case)[0]
    want, want_dec, want_status = g["parent_scores"], g["parent_decisions"], int(g["parent_status"])
    runs = {("default", S): run_case(case, "default", S) for S in (1, 2, 4)}
    runs[("top0", 1)] = run_case(case, "top0", 1)
    assert any("k_top" in k for k in runs[("default", 1)]["kernels"]), runs[("default", 1)]["kernels"]
    assert not any("k_top" in k for k in runs[("top0", 1)]["kernels"]), runs[("top0", 1)]["kernels"]
    assert want_status == (1 if nan else 0), (case, want_status)
    fin = np.isfinite(want)
    if not nan:
        assert np.array_equal(fin, batch_of(case).masks.numpy() != 0), case          # every scored node got a score, on poisoned memory
    bad = []
    for key, r in runs.items():
        diff = r["scores"] != want
        if nan:
            diff &= ~(np.isnan(r["scores"]) & np.isnan(want))
        both = fin & np.isfinite(r["scores"])
        delta = float(np.abs(r["scores"][both] - want[both]).max()) if both.any() else 0.0
        print(f"{case} {key[0]} S={key[1]}: status {r['status']}, scores differing from the parent's: {int(diff.sum())} of {diff.size} "
              f"(max |delta| {delta:.3e}), decisions equal: {np.array_equal(r['decisions'], want_dec)}")
        # the same entries finite / -inf / NaN everywhere; identical for the default handle, inside the bar for the twin
        same_kind = np.array_equal(np.isfinite(r["scores"]), fin) and np.array_equal(np.isnan(r["scores"]), np.isnan(want))
        close = not diff.any() if key[0] == "default" else delta <= TWIN_ATOL
        if r["status"] != want_status or not same_kind or not close or not np.array_equal(r["decisions"], want_dec):
            bad.append(key)
    assert not bad, (case, bad)


def write_golden(outdir):
    """Fixtures of every case from the library that is loaded (GNNB_LIB or the tree's): the batch and what the default handle returns."""
    import os
    os.makedirs(outdir, exist_ok=True)
    for case, (K, N, B, _, _) in CASES.items():
        batch = synth_batch(case)
        runs = [run_case(case, "default", S, batch) for S in (1, 2, 4)]
        for r in runs[1:]:
            assert np.array_equal(r["scores"], runs[0]["scores"], equal_nan=True) and np.array_equal(r["decisions"], runs[0]["decisions"])
            assert r["status"] == runs[0]["status"]
        nl = len(batch.lower_bounds_all)
        assert len(batch.dual_vars) == nl - 2 and len(batch.bab_masks) == nl - 2
        rec = {"net": np.array(arch_name(K, N)), "B": np.array(B), "props": np.array((PROPS * 2)[:B], dtype=np.int64),
               "primal_input": batch.primal_inputs.numpy(), "masks": batch.masks.numpy().astype(np.uint8),
               "parent_scores": runs[0]["scores"], "parent_decisions": runs[0]["decisions"], "parent_status": np.array(runs[0]["status"])}
        for i in range(nl):
            rec[f"lb{i}"], rec[f"ub{i}"] = batch.lower_bounds_all[i].numpy(), batch.upper_bounds_all[i].numpy()
        for i in range(nl - 2):
            rec[f"dual{i}"], rec[f"bab{i}"] = batch.dual_vars[i].numpy(), batch.bab_masks[i].numpy().astype(np.int8)
        for i, t in enumerate(batch.primals):
            rec[f"primal{i}"] = t.numpy()
        np.savez_compressed(os.path.join(outdir, case + ".npz"), **rec)
        print(case, "status", runs[0]["status"], os.path.getsize(os.path.join(outdir, case + ".npz")), "bytes")


if __name__ == "__main__":
    import sys
    write_golden(sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "top_roundtrips"))
