"""Wong-Kolter intermediate bounds of a batch of BaB domains on the MI355X (gnnb_kw_bounds, ScorerEngine.kw_bounds,
LayerGraphLP(bounds="kw_device")) against the host's fp64 LayerGraphLP.kw_bounds: root parity on the three networks, batched = single bit
for bit, the incremental form of a child, soundness on sampled points, infeasible domains, fp32 outputs that feed the scorers directly,
a NaN-poisoned workspace, and the threshold loop with either bounds mode."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import lp_producer, nets

pytestmark = pytest.mark.gpu

EPS = {"cifar_base_kw": 0.09, "cifar_wide_kw": 0.05, "cifar_deep_kw": 0.05}


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    return ScorerEngine(None)


def make_lp(name, engine, bounds="kw_device"):
    layers = nets.load_verified_net(name, 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    return lp_producer.LayerGraphLP(layers, x - EPS[name], x + EPS[name], bounds=bounds, engine=engine)


def root_mask(lp):
    return [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]


def assert_close(lp, got, want):
    """Every entry of the bounds list within 1e-9 max(1, max|bound| of the layer); ambiguous / decided sets identical."""
    for side in (0, 1):
        assert len(got[side]) == len(want[side])
        for i, (g, w) in enumerate(zip(got[side], want[side])):
            assert g.shape == w.shape and g.dtype == torch.float64, i
            tol = 1e-9 * max(1.0, float(w.abs().max()))
            err = float((g - w).abs().max())
            assert err <= tol, (side, i, err, tol)
    for i in lp.pre_relu_indices:
        gl, gu, wl, wu = got[0][i], got[1][i], want[0][i], want[1][i]
        assert torch.equal((gl < 0) & (gu > 0), (wl < 0) & (wu > 0)), i
        assert torch.equal(gl >= 0, wl >= 0) and torch.equal(gu <= 0, wu <= 0), i


def split_masks(lp, parent, n, seed):
    """n different valid split masks: a few nodes that are ambiguous under ``parent`` forced passing or blocked."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        m = root_mask(lp)
        for r, i in enumerate(lp.pre_relu_indices):
            amb = torch.nonzero((parent[0][i].reshape(-1) < 0) & (parent[1][i].reshape(-1) > 0)).reshape(-1).numpy()
            for node in rng.choice(amb, size=min(2, len(amb)), replace=False):
                m[r][int(node)] = int(rng.randint(2))
        out.append(m)
    return out


@pytest.mark.parametrize("name", ["cifar_base_kw", "cifar_wide_kw", "cifar_deep_kw"])
def test_root_bounds_match_the_host(name, engine):
    lp = make_lp(name, engine)
    mask = root_mask(lp)
    assert_close(lp, lp.bounds(mask), lp.kw_bounds(mask))


def test_batched_rows_equal_single_calls_and_the_host(engine):
    lp = make_lp("cifar_base_kw", engine)
    root = lp.kw_bounds(root_mask(lp))
    masks = split_masks(lp, root, 7, seed=11)
    batched = lp.kw_device_bounds([(m, None, None) for m in masks])
    for m, got in zip(masks, batched):
        single = lp.kw_device_bounds([(m, None, None)])[0]
        for side in (0, 1):
            assert all(torch.equal(a, b) for a, b in zip(got[side], single[side]))
        assert_close(lp, got, lp.kw_bounds(m))


def test_children_are_incremental(engine):
    lp = make_lp("cifar_base_kw", engine)
    parent = lp.kw_bounds(root_mask(lp))
    items = []
    for s, i in enumerate(lp.pre_relu_indices):
        amb = torch.nonzero((parent[0][i].reshape(-1) < 0) & (parent[1][i].reshape(-1) > 0)).reshape(-1)
        assert len(amb), s
        for choice in (0, 1):
            m = root_mask(lp)
            m[s][int(amb[len(amb) // 2])] = choice
            items.append((m, parent, s))
    got = lp.kw_device_bounds(items)
    for (m, p, s), g in zip(items, got):
        want = lp.kw_bounds(m, p, s)
        assert_close(lp, g, want)
        keep = lp.pre_relu_indices[s]
        for side in (0, 1):
            for i in range(1, keep + 1):                 # at or below the split: the parent's, bit for bit (the split node clamped)
                assert torch.equal(g[side][i], want[side][i]), (s, side, i)


def test_bounds_are_sound_on_sampled_points(engine):
    lp = make_lp("cifar_base_kw", engine)
    lbs, ubs = lp.bounds(root_mask(lp))
    rng = np.random.RandomState(3)
    lo, hi = lp.input_lb.numpy(), lp.input_ub.numpy()
    x = torch.from_numpy(lo + (hi - lo) * rng.uniform(0, 1, (300,) + lo.shape))
    with torch.no_grad():
        a = x
        for i, l in enumerate(lp.layers):
            a = copy.deepcopy(l).double()(a) if isinstance(l, (nn.Conv2d, nn.Linear)) else l(a)
            assert bool((a >= lbs[i + 1][None] - 1e-9).all()) and bool((a <= ubs[i + 1][None] + 1e-9).all()), i


def test_infeasible_domain_is_flagged(engine):
    lp = make_lp("cifar_base_kw", engine)
    root = lp.kw_bounds(root_mask(lp))
    i0 = lp.pre_relu_indices[0]
    dead = torch.nonzero(root[1][i0].reshape(-1) < -1e-6).reshape(-1)
    assert len(dead)
    m = root_mask(lp)
    m[0][int(dead[0])] = 1                               # forced passing a node that is always blocked
    masks = torch.stack([torch.cat([t.reshape(-1) for t in mk]) for mk in (root_mask(lp), m)]).to(torch.int8)
    x_lo = lp.input_lb[None].expand(2, *lp.shapes[0])
    x_hi = lp.input_ub[None].expand(2, *lp.shapes[0])
    res = engine.kw_bounds(lp.layers[:-1], [lp.layers[-1]] * 2, x_lo, x_hi, masks)
    assert res.infeasible.cpu().tolist() == [0, 1]
    assert lp.solve(m) is None
    assert make_lp("cifar_base_kw", engine, bounds="kw").solve(m) is None


def test_fp32_outputs_feed_the_scorers_directly():
    from gnn_branching_amd import synth
    from tests.test_gpu_parity import make_model
    batch = synth.make_batch("cifar_base_kw", 4, seed=5, eps=0.03)
    eng = make_model("shipped").engine()
    fixed, props = batch.layers["fixed_layers"], batch.layers["prop_layers"]
    B, R = 4, int(batch.masks.shape[1])
    res = eng.kw_bounds(fixed, props, batch.lower_bounds_all[0].double(), batch.upper_bounds_all[0].double(),
                        torch.full((B, R), -1, dtype=torch.int8), want_fp32=True)
    assert torch.equal(res.lb32[0].cpu(), batch.lower_bounds_all[0]) and torch.equal(res.ub32[0].cpu(), batch.upper_bounds_all[0])
    for k in range(1, len(res.lb32)):
        assert torch.equal(res.lb32[k].cpu(), res.lb[k - 1].float().cpu()) and torch.equal(res.ub32[k].cpu(), res.ub[k - 1].float().cpu())
    amb = torch.cat([((l < 0) & (u > 0)).float() for l, u in zip(res.lb32[1:-1], res.ub32[1:-1])], 1)
    layers = {"fixed_layers": fixed, "prop_layers": props}
    with torch.no_grad():
        dev = eng.babsr(res.lb32, res.ub32, layers, amb)
        host = eng.babsr([t.cpu() for t in res.lb32], [t.cpu() for t in res.ub32], layers, amb.cpu())
        assert torch.equal(dev.scores.cpu(), host.scores.cpu()) and torch.equal(dev.intercepts.cpu(), host.intercepts.cpu())
        args = dict(dual_vars=batch.dual_vars, primals=batch.primals, primal_inputs=batch.primal_inputs, layers=layers)
        fd = eng.forward(res.lb32, res.ub32, masks=amb, **args).check()
        fh = eng.forward([t.cpu() for t in res.lb32], [t.cpu() for t in res.ub32], masks=amb.cpu(), **args).check()
        assert np.array_equal(fd.scores.cpu().numpy(), fh.scores.cpu().numpy(), equal_nan=True)
        assert torch.equal(fd.decisions.cpu(), fh.decisions.cpu())


def test_workspace_contents_do_not_matter(engine):
    lp = make_lp("cifar_deep_kw", engine)
    parent = lp.kw_bounds(root_mask(lp))
    items = [(m, parent, 1) for m in split_masks(lp, parent, 3, seed=2)]
    for m, _, _ in items:
        m[0][:] = -1                                     # the split is on ReLU layer 1: nothing below it changes
    first = lp.kw_device_bounds(items)
    engine.kw_workspace(len(items)).fill_(0xFF)          # all-ones bytes: NaN doubles
    again = lp.kw_device_bounds(items)
    for a, b in zip(first, again):
        for side in (0, 1):
            assert all(torch.equal(x, y) for x, y in zip(a[side], b[side]))


def test_threshold_loop_takes_the_same_decisions(engine):
    import os
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
    nets.register_arch("toy_lp", [("conv", 3, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 8 * 16 * 16, 32), ("relu",), ("linear", 32, 10)],
                       seed=321)
    layers = nets.load_verified_net("toy_lp", 3, 5)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 32, 32)).astype(np.float32))
    ckpt = os.path.join(os.path.dirname(__file__), "..", "models", "cifar_trained_gnn",
                        "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")
    runs = []
    for mode in ("kw", "kw_device"):
        lp = lp_producer.LayerGraphLP(layers, x - 0.03, x + 0.03, bounds=mode, engine=engine if mode == "kw_device" else None)
        choice = GraphChoice(lp.solve(root_mask(lp)).mask, ckpt)
        choice.verbose = False
        decisions = []

        def gnn(sub, fixed):
            d = lp_producer.gnn_scorer(choice, lp)(sub, fixed)
            decisions.append(("gnn", list(d)))
            return d

        def kw(sub, icp, order, sparsest):
            d, icp = choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, order, sparsest)
            decisions.append(("kw", list(d)))
            return d, icp
        res = lp_producer.branch_and_bound_threshold(lp, gnn, kw, layers, max_branches=4, branching_threshold=0.5, log=lambda s: None)
        runs.append((decisions, res))
    (da, ra), (db, rb) = runs
    assert len(da) >= 2 and da == db
    assert ra[2:] == rb[2:]
    assert abs(ra[0] - rb[0]) <= 1e-6 and abs(ra[1] - rb[1]) <= 1e-6
