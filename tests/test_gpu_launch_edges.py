"""-m gpu: what a launch does at its opening and closing -- the staged weight image of k_gather_update_q, k_pre's single staging
phase, the dealing of k_scored_tail's score tiles -- against the handle options that bypass each of them, bit for bit.

  fuse = 0          k_gather + k_node_update instead of k_gather_update_q (no staged image, no chain wave waiting for a stage)
  tail_max_b = 0    k_gather_scored + k_node_update + k_score instead of k_scored_tail (k_score's own tile dealing)
  clspre_max_b      k_classify_pre (its two staging phases) instead of k_classify + k_pre: the P' rows both leave in the workspace

Batches: cifar_base_kw at B = 1, 3, 9 (workgroups with no, one and several tiles, a partly filled last ring tile), a batch whose layers
2..L have no scored node (k_scored_tail has no tile to deal), a batch with a layer without ambiguous nodes (k_pre: a layer of zero tiles
in both directions between two that have some) and cifar_deep_kw at B = 2 (the POST launch and the others through the same staging)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.common import state_of

pytestmark = pytest.mark.gpu

CASES = [("cifar_base_kw", 1, "plain"), ("cifar_base_kw", 3, "plain"), ("cifar_base_kw", 9, "plain"),
         ("cifar_base_kw", 3, "layer1_only_scored"), ("cifar_base_kw", 3, "layer2_not_ambiguous"), ("cifar_deep_kw", 2, "plain")]
IDS = [f"{n}-B{b}-{v}" for n, b, v in CASES]


def make_model():
    from gnn_branching_amd.graphnet.graph_conv import GraphNet
    m = GraphNet(2, 64)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state_of("random").items()})      # (the shipped forward weights are subnormal)
    return m.eval()


def ambiguous(lb, ub):
    """The nodes the classification lists as ambiguous: beta > 0 of the reference's compute_ratio, in its fp32 operations (a subset of
    lb < 0 < ub: the product may underflow)."""
    lower, upper = lb - torch.relu(lb), torch.relu(ub)
    return -1.0 * lower * (upper / (upper - lower)) > 0


@lru_cache(None)
def batch_args(net, B, variant):
    """The forward's arguments (never modified afterwards) and the number of ambiguous nodes per ReLU layer."""
    from gnn_branching_amd import synth
    batch = synth.make_batch(net, B, seed=70 + B)
    lbs, ubs = [t.clone() for t in batch.lower_bounds_all], list(batch.upper_bounds_all)
    masks = batch.masks.clone()
    sizes = [int(np.prod(t.shape[1:])) for t in lbs[1:-1]]
    if variant == "layer1_only_scored":
        masks[:, sizes[0]:] = 0
    elif variant == "layer2_not_ambiguous":             # its ambiguous nodes become stable-active ones (lb = 0), and are not scored
        amb = (lbs[2] < 0) & (ubs[2] > 0)
        assert int(amb.sum()) > 0
        lbs[2][amb] = 0.0
        masks[:, sizes[0]:sizes[0] + sizes[1]] = 0
    n_amb = [int(ambiguous(l, u).sum()) for l, u in zip(lbs[1:-1], ubs[1:-1])]
    assert masks.sum() > 0
    return (lbs, ubs, batch.dual_vars, batch.primals, batch.primal_inputs, batch.layers, masks), n_amb


def run(monkeypatch, env, net, B, variant, want_pre_rows=False):
    """One forward of a fresh engine under the environment `env`, on a workspace full of NaNs: scores, decisions, status word (and
    the P' rows of k_pre / k_classify_pre as bit patterns)."""
    for name in ("GNNB_FUSE", "GNNB_TAIL_MAX_B", "GNNB_CLSPRE_MAX_B"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    args, n_amb = batch_args(net, B, variant)
    model = make_model()
    eng = model.engine()
    with torch.no_grad():
        model.forward_device(*args).check()             # (binds the network: the workspace exists behind it)
        eng.workspace(B).view(torch.float32).fill_(float("nan"))
        res = model.forward_device(*args).check()
    out = {"scores": res.scores.cpu(), "decisions": res.decisions.cpu(), "status": int(res.status.cpu()[0]), "describe": eng.describe()}
    if want_pre_rows:
        out["pre_rows"] = pre_rows(eng, B, n_amb)
    return out


def pre_rows(eng, B, n_amb):
    """The P' rows (forward, backward) per ReLU layer as int32 bit patterns.  The workspace keeps them behind the embeddings and the
    aggregate buffer, every region a multiple of 64 floats (gnnb.hip ws_layout).  That the regions are where this says is checked on the
    contents: on a workspace of NaNs exactly the rows of the ambiguous nodes are written."""
    import ctypes as C

    def align64(n):
        return (n + 63) & ~63
    N, K = eng.sizes, len(eng.sizes) - 1
    off, n = C.c_size_t(), C.c_size_t()
    assert eng.lib.gnnb_mu_location(eng.h, B, K, C.byref(off), C.byref(n)) == 0
    pos = off.value // 4 + align64(B * N[K] * 64) + align64(B * max(N[:K]) * 64)
    ws = eng.workspace(B).view(torch.float32)
    rows = []
    for d in range(2):
        for k in range(1, K):
            r = ws[pos:pos + B * N[k] * 64].view(B * N[k], 64).cpu()
            pos += align64(B * N[k] * 64)
            written = ~torch.isnan(r).any(1)
            assert int(written.sum()) == n_amb[k - 1] and bool(torch.isfinite(r[written]).all()), (d, k, int(written.sum()), n_amb[k - 1])
            rows.append(r.view(torch.int32).clone())
    return rows


def same(a, b):
    assert a["status"] == 0 and b["status"] == 0, (a["status"], b["status"])
    assert torch.equal(a["scores"], b["scores"])
    assert torch.equal(a["decisions"], b["decisions"])
    assert bool(torch.isfinite(a["scores"]).any())


@pytest.mark.parametrize("net,B,variant", CASES, ids=IDS)
def test_staged_weight_image_of_the_fused_halfpass(monkeypatch, net, B, variant):
    """k_gather_update_q's chain waves start their first tile behind the first stage of the weight image and ask for the later stages
    block by block; fuse = 0 runs the same node update as k_node_update behind a barrier."""
    fused = run(monkeypatch, {"GNNB_FUSE": "1"}, net, B, variant)
    plain = run(monkeypatch, {"GNNB_FUSE": "0"}, net, B, variant)
    kernels = lambda o: [u["kernel"] for u in o["describe"]["updates"]]      # noqa: E731
    assert any(k == "k_gather_update" for k in kernels(fused)) and not any(k == "k_gather_update" for k in kernels(plain))
    same(fused, plain)


@pytest.mark.parametrize("net,B,variant", CASES, ids=IDS)
def test_score_tiles_dealt_over_the_gather_waves(monkeypatch, net, B, variant):
    """k_scored_tail deals the other layers' score tiles round-robin over the workgroups' gather waves; tail_max_b = 0 scores them in
    k_score.  Scores, decisions (the per-sample keys) and the status word are the same."""
    tail = run(monkeypatch, {}, net, B, variant)
    three = run(monkeypatch, {"GNNB_TAIL_MAX_B": "0"}, net, B, variant)
    same(tail, three)


@pytest.mark.parametrize("net,B,variant", CASES, ids=IDS)
def test_pre_rows_of_the_single_staging_phase(monkeypatch, net, B, variant):
    """k_pre stages once (the forward W23 block waits in W53's place, W53 in registers); k_classify_pre keeps two staging phases.  Both
    leave the same P' rows, forward and backward, for every ambiguous node, and nothing else in those regions."""
    pre = run(monkeypatch, {"GNNB_CLSPRE_MAX_B": "0"}, net, B, variant, want_pre_rows=True)
    cls = run(monkeypatch, {"GNNB_CLSPRE_MAX_B": str(1 << 30)}, net, B, variant, want_pre_rows=True)
    same(pre, cls)
    assert len(pre["pre_rows"]) == len(cls["pre_rows"]) > 0
    for a, b in zip(pre["pre_rows"], cls["pre_rows"]):
        assert torch.equal(a, b)
