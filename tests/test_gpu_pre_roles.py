"""-m gpu: k_pre with its workgroups split into forward and backward ones (each stages its own direction's image as one batch of
requests, tiles strided over all 16 waves of the role's workgroups) against k_classify_pre, which keeps its own dealing (a block's own
nodes) and its two staging phases: the P' rows both leave in a workspace of NaNs, bit for bit, and the scores, decisions and status word
behind them.

  GNNB_CLSPRE_MAX_B = 0        k_classify + k_pre for every batch size
  GNNB_CLSPRE_MAX_B = 1 << 30  k_classify_pre for every batch size

Cases (cifar_base_kw, random weights, unless said): B = 1 and B = 2 (a grid of one workgroup -- no roles -- or of a few: one forward
workgroup), B = 3 with every node of every ReLU layer ambiguous (many more tiles than waves in both roles: both strided loops run
several rounds), a layer without ambiguous nodes between two that have some, layer 3 with exactly 32 and exactly 33
ambiguous nodes at B = 1 (a full last tile; a last tile with one valid lane), cifar_deep_kw at B = 2 (more layers in the tile -> layer
walk)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.test_gpu_launch_edges import ambiguous, make_model, pre_rows, same

pytestmark = pytest.mark.gpu

CASES = [("cifar_base_kw", 1, "plain"), ("cifar_base_kw", 2, "plain"), ("cifar_base_kw", 3, "all_ambiguous"),
         ("cifar_base_kw", 3, "layer2_not_ambiguous"), ("cifar_base_kw", 1, "layer3_32_ambiguous"), ("cifar_base_kw", 1, "layer3_33_ambiguous"),
         ("cifar_deep_kw", 2, "plain")]
IDS = [f"{n}-B{b}-{v}" for n, b, v in CASES]
EPS = 1e-3


@lru_cache(None)
def batch_args(net, B, variant):
    """The forward's arguments (never modified afterwards) and the number of ambiguous nodes per ReLU layer."""
    from gnn_branching_amd import synth
    batch = synth.make_batch(net, B, seed=170 + B)
    lbs, ubs = [t.clone() for t in batch.lower_bounds_all], [t.clone() for t in batch.upper_bounds_all]
    masks = batch.masks.clone()
    sizes = [int(np.prod(t.shape[1:])) for t in lbs[1:-1]]
    starts = [sum(sizes[:k]) for k in range(len(sizes))]
    if variant == "all_ambiguous":
        for k in range(1, len(lbs) - 1):
            lbs[k], ubs[k] = -lbs[k].abs() - EPS, ubs[k].abs() + EPS
    elif variant == "layer2_not_ambiguous":              # its ambiguous nodes become stable-active ones (lb = 0), and are not scored
        amb = (lbs[2] < 0) & (ubs[2] > 0)
        assert int(amb.sum()) > 0
        lbs[2][amb] = 0.0
        masks[:, starts[1]:starts[1] + sizes[1]] = 0
    elif variant.startswith("layer3_"):                  # layer 3: the first n nodes ambiguous, the others stable-active and not scored
        n = int(variant.split("_")[1])
        assert B == 1 and sizes[2] > n
        lb, ub = (-lbs[3].abs() - EPS).reshape(1, -1), (ubs[3].abs() + EPS).reshape(1, -1)
        lb[:, n:] = 0.0
        lbs[3], ubs[3] = lb.reshape(lbs[3].shape), ub.reshape(ubs[3].shape)
        masks[:, starts[2] + n:starts[2] + sizes[2]] = 0
    n_amb = [int(ambiguous(l, u).sum()) for l, u in zip(lbs[1:-1], ubs[1:-1])]
    if variant == "all_ambiguous":
        assert n_amb == [B * s for s in sizes]
    elif variant == "layer2_not_ambiguous":
        assert n_amb[0] > 0 and n_amb[1] == 0 and n_amb[2] > 0
    elif variant.startswith("layer3_"):
        assert n_amb[2] == int(variant.split("_")[1])
    assert masks.sum() > 0
    return (lbs, ubs, batch.dual_vars, batch.primals, batch.primal_inputs, batch.layers, masks), n_amb


def run(monkeypatch, clspre_max_b, net, B, variant):
    """One forward of a fresh engine on a workspace full of NaNs: scores, decisions, status word, the launched kernels' names and the
    P' rows as bit patterns (pre_rows asserts that exactly the ambiguous nodes' rows are written and that they are finite)."""
    for name in ("GNNB_FUSE", "GNNB_TAIL_MAX_B", "GNNB_CLSPRE_MAX_B"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("GNNB_CLSPRE_MAX_B", str(clspre_max_b))
    args, n_amb = batch_args(net, B, variant)
    model = make_model()
    eng = model.engine()
    with torch.no_grad():
        model.forward_device(*args).check()              # (binds the network: the workspace exists behind it)
        eng.workspace(B).view(torch.float32).fill_(float("nan"))
        res = model.forward_device(*args).check()
    return {"scores": res.scores.cpu(), "decisions": res.decisions.cpu(), "status": int(res.status.cpu()[0]),
            "pre_rows": pre_rows(eng, B, n_amb)}


@pytest.mark.parametrize("net,B,variant", CASES, ids=IDS)
def test_pre_rows_of_the_role_split(monkeypatch, net, B, variant):
    pre = run(monkeypatch, 0, net, B, variant)
    cls = run(monkeypatch, 1 << 30, net, B, variant)
    same(pre, cls)
    assert len(pre["pre_rows"]) == len(cls["pre_rows"]) > 0
    for a, b in zip(pre["pre_rows"], cls["pre_rows"]):
        assert torch.equal(a, b)
