"""Dual ascent on the subproblem LPs on the MI355X (ScorerEngine.dual_ascent -> gnnb_dual_ascent) against its host twin in torch fp64
(LayerGraphLP.dual_ascent_host / dual_recover) on the small geometries of tests/common.py KW_ARCHS, B = 4 mixed domains per network, each
with its own box and property row: a root, a domain with nodes forced passing and blocked in every ReLU layer, and two children (split on
the first ReLU layer, blocked; on the last, passing).  Both sides read the SAME intermediate bounds (the device's gnnb_kw_bounds), so
what is compared is the ascent alone.  Then HiGHS on the toy network of tests/test_lp_producer.py, the scorer fed from device arrays
only, the threshold loop with child_lp="dual_device", and the limits."""
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

from gnn_branching_amd import lp_producer
from tests.common import register_kw_archs, register_toy_archs
from tests.test_dual_ascent_cpu import toy_kw_domains
from tests.test_gpu_kw_geometry import Net, graph_index, mixed_batch, run_device, seeded_domain

pytestmark = pytest.mark.gpu

NETS = ["kwg_mlp", "kwg_rect", "kwg_gap", "kwg_single", "kwg_s1", "kwg_deep8"]
LR = 0.1
CKPT = os.path.join(os.path.dirname(__file__), "..", "models", "cifar_trained_gnn", "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    return ScorerEngine(None)


def host_bounds(lp, kw, b):
    """Row b of a KwBoundsResult in the host's list form (only the affine outputs, which is all the twin reads)."""
    full = [[None] * (len(lp.layers) + 1) for _ in range(2)]
    for g, i in enumerate(graph_index(lp)):
        full[0][i], full[1][i] = kw.lb[g][b].cpu(), kw.ub[g][b].cpu()
    return tuple(full)


class Case:
    """One network's batch: the domains, their device bounds (one gnnb_kw_bounds call) and the same bounds on the host."""

    def __init__(self, engine, name, doms=None):
        self.net = Net(name)
        if doms is None:
            six = mixed_batch(self.net)
            doms = [six[0], six[2], six[4], six[5]]
        self.doms = doms
        self.kw = run_device(engine, doms, want_fp32=True)
        self.bounds = [host_bounds(d.lp, self.kw, b) for b, d in enumerate(doms)]
        self.x_lo = torch.stack([d.x_lo for d in doms])
        self.x_hi = torch.stack([d.x_hi for d in doms])
        self.masks = torch.stack([torch.cat([m.reshape(-1) for m in d.mask]) for d in doms]).to(torch.int8)
        self.props = [self.net.prop(d.gt, d.cls) for d in doms]
        self.R = int(self.masks.shape[1])
        self._runs = {}

    def device(self, engine, n_iter, rows=None, **kw):
        sel = slice(None) if rows is None else rows
        return engine.dual_ascent(self.net.fixed, self.props[sel], self.x_lo[sel], self.x_hi[sel], self.masks[sel], [t[sel] for t in self.kw.lb],
                                  [t[sel] for t in self.kw.ub], n_iter, LR, **kw)

    def default_run(self, engine, n_iter):
        """From the default start, with the scorer's inputs; computed once per (network, n_iter)."""
        if n_iter not in self._runs:
            self._runs[n_iter] = self.device(engine, n_iter, want_scorer_inputs=True)
        return self._runs[n_iter]


_cases = {}


def case(engine, name):
    if name not in _cases:
        _cases[name] = Case(engine, name)
    return _cases[name]


def near_kinks(d, bounds, alpha, beta):
    """Nodes and inputs whose branch the twin decides on a |lambda| below 1e-12 without being exactly zero on both sides' rule."""
    rec = d.lp.dual_recover(bounds, d.mask, alpha, beta)
    lam = torch.cat(rec["lam"])
    return int(((lam != 0) & (lam.abs() < 1e-12)).sum()), int(((rec["lam0"] != 0) & (rec["lam0"].abs() < 1e-12)).sum())


def test_the_batches_are_mixed(engine):
    for name in NETS:
        c = case(engine, name)
        m = c.masks
        assert not bool((m[0] != -1).any())
        assert int((m[1] != -1).sum()) >= 2
        assert int((m[2] == 0).sum()) == 1 and int((m[3] == 1).sum()) == 1 and int((m[2:] != -1).sum()) == 2
        assert len({(d.gt, d.cls) for d in c.doms}) == 4


@pytest.mark.parametrize("name", NETS)
def test_value_and_supergradient_at_a_random_point(name, engine):
    """n_iter = 0, warm: bound within 1e-9 max(1, |g|) of the twin (the project's fp64 KW tolerance), grad_alpha / grad_beta within
    1e-9 max(1, max|grad|).  Entries of nodes whose branch hangs on a |lambda| below 1e-12 are left out, 1 % of a domain's at most."""
    c = case(engine, name)
    g = torch.Generator().manual_seed(17)
    alpha = torch.rand(len(c.doms), c.R, generator=g, dtype=torch.float64)
    beta = torch.rand(len(c.doms), c.R, generator=g, dtype=torch.float64)
    res = c.device(engine, 0, alpha=alpha, beta=beta, want_grad=True)
    for b, d in enumerate(c.doms):
        want = d.lp.dual_ascent_host(c.bounds[b], d.mask, 0, alpha=alpha[b], beta=beta[b])
        got = float(res.bound[b])
        print(f"{name} row {b}: g {want.bound:.12f} device - twin {got - want.bound:.3e}")
        assert abs(got - want.bound) <= 1e-9 * max(1.0, abs(want.bound)), (name, b, got, want.bound)
        assert torch.equal(res.alpha[b].cpu(), want.alpha) and torch.equal(res.beta[b].cpu(), want.beta)      # the projection of the entry point
        rec = d.lp.dual_recover(c.bounds[b], d.mask, want.alpha, want.beta)
        lam = torch.cat(rec["lam"])
        skip = lam.abs() < 1e-12
        skip &= lam != 0                                                        # (an exact zero takes the alpha branch on both sides)
        n0 = int(((rec["lam0"] != 0) & (rec["lam0"].abs() < 1e-12)).sum())
        assert int(skip.sum()) + n0 <= c.R // 100, (name, b, int(skip.sum()), n0)
        for what, dev, ref in (("alpha", res.grad_alpha[b].cpu(), want.grad_alpha), ("beta", res.grad_beta[b].cpu(), want.grad_beta)):
            tol = 1e-9 * max(1.0, float(ref.abs().max()))
            err = float((dev - ref)[~skip].abs().max())
            print(f"    grad_{what}: max |grad| {float(ref.abs().max()):.3e} max err {err:.3e} left out {int(skip.sum())} inputs near 0 {n0}")
            assert err <= tol, (name, b, what, err, tol, n0)
        assert float(want.grad_alpha.abs().max()) > 0 and (b == 0 or float(want.grad_beta.abs().max()) > 0)


@pytest.mark.parametrize("name", NETS)
def test_five_iterations_from_the_default_start(name, engine):
    """bound, alpha and beta within 1e-8 of the twin's (Adam amplifies rounding a little: a step is lr g / (|g| + 1e-8) at first)."""
    c = case(engine, name)
    res = c.default_run(engine, 5)
    for b, d in enumerate(c.doms):
        want = d.lp.dual_ascent_host(c.bounds[b], d.mask, 5, lr=LR)
        kinks = near_kinks(d, c.bounds[b], want.alpha, want.beta)
        eb = abs(float(res.bound[b]) - want.bound)
        ea = float((res.alpha[b].cpu() - want.alpha).abs().max())
        ebeta = float((res.beta[b].cpu() - want.beta).abs().max())
        print(f"{name} row {b}: values {want.values[0]:.6f} -> {want.bound:.6f}; |bound| {eb:.3e} |alpha| {ea:.3e} |beta| {ebeta:.3e}; near kinks {kinks}")
        msg = (name, b, eb, ea, ebeta, "nodes / inputs with 0 < |lambda| < 1e-12 at the twin's point:", kinks)
        assert eb <= 1e-8 and ea <= 1e-8 and ebeta <= 1e-8, msg
        assert want.bound > want.values[0]


@pytest.mark.parametrize("name", NETS)
def test_best_so_far_is_monotone(name, engine):
    c = case(engine, name)
    b0, b5, b25 = (c.default_run(engine, n).bound.cpu() for n in (0, 5, 25))
    assert bool((b0 <= b5).all()) and bool((b5 <= b25).all()), (b0, b5, b25)
    assert bool((b0 < b25).all())


@pytest.mark.parametrize("name", NETS)
def test_a_domain_alone_equals_its_row_in_the_batch(name, engine):
    """Row 2 of B = 4 and the same domain as B = 1: bound, alpha, beta and every scorer input bit for bit."""
    c = case(engine, name)
    four = c.default_run(engine, 5)
    one = c.device(engine, 5, rows=slice(2, 3), want_scorer_inputs=True)
    B = len(c.doms)
    for a, b in ((four.bound, one.bound), (four.alpha, one.alpha), (four.beta, one.beta), (four.x_lp, one.x_lp)):
        assert torch.equal(a[2:3], b)
    for a, b in zip(four.dual + four.primals, one.dual + one.primals):
        if a.numel() > 1:
            assert torch.equal(a.reshape(B, -1)[2:3], b.reshape(1, -1))


@pytest.mark.parametrize("name", NETS)
def test_scorer_inputs(name, engine):
    """After 25 iterations: dual[:, 0] = 0, dual[:, 1] >= 0 >= dual[:, 2], never both, zero on decided nodes; x_lp a corner of the box;
    every pre-activation the fp64 affine image of the post-activation below within fp32 rounding; every post-activation inside its
    node's triangle within 1e-6; all of it the twin's recovery pass at the device's (alpha, beta)."""
    c = case(engine, name)
    res = c.default_run(engine, 25)
    B = len(c.doms)
    u = 2.0 ** -23
    for b, d in enumerate(c.doms):
        lp = d.lp
        x = res.x_lp[b].cpu()
        lo32, hi32 = d.x_lo.float(), d.x_hi.float()
        assert bool(((x == lo32) | (x == hi32)).all()) and bool((x >= lo32).all()) and bool((x <= hi32).all())
        rec = lp.dual_recover(c.bounds[b], d.mask, res.alpha[b].cpu(), res.beta[b].cpu())
        assert abs(rec["g"] - float(res.bound[b])) <= 1e-9 * max(1.0, abs(rec["g"]))
        q, qa, r = x.double(), x.double().abs(), 0
        for i, l in enumerate(lp.layers[:-1]):
            if type(l) in (nn.Conv2d, nn.Linear):
                q = lp._affine(l, q)
                if type(l) is nn.Conv2d:
                    qa = F.conv2d(qa[None], l.weight.double().abs(), l.bias.double().abs(), l.stride, l.padding)[0]
                else:
                    qa = l.weight.double().abs() @ qa + l.bias.double().abs()
            elif type(l) is nn.ReLU:
                pre = res.primals[i - 1].reshape(B, -1)[b].cpu().double()
                post = res.primals[i].reshape(B, -1)[b].cpu().double()
                dual = res.dual[r].reshape(B, -1, 3)[b].cpu().double()
                err = (pre - q.reshape(-1)).abs()
                assert bool((err <= u * qa.reshape(-1) + 1e-30).all()), (name, b, r, float(err.max()))
                lo, up, m = c.bounds[b][0][i].reshape(-1), c.bounds[b][1][i].reshape(-1), d.mask[r]
                amb = (m == -1) & (lo < 0) & (up > 0)
                passing = (m == 1) | ((m == -1) & (lo >= 0))
                blocked = ~amb & ~passing
                s = up / (up - lo)
                assert bool((post[amb] >= pre[amb].clamp(min=0) - 1e-6).all()), (name, b, r, float((pre[amb].clamp(min=0) - post[amb]).max()))
                assert bool((post[amb] <= (s * (pre - lo))[amb] + 1e-6).all()), (name, b, r, float((post - s * (pre - lo))[amb].max()))
                assert bool(((post - pre)[passing].abs() <= 1e-6).all()) and not bool(post[blocked].any())
                assert not bool(dual[:, 0].any()) and bool((dual[:, 1] >= 0).all()) and bool((dual[:, 2] <= 0).all())
                assert not bool(((dual[:, 1] != 0) & (dual[:, 2] != 0)).any()) and not bool(dual[~amb].any())
                for got, want in ((pre, rec["pre"][r]), (post, rec["post"][r]), (dual, rec["dual"][r])):
                    assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max())), (name, b, r)
                q = post.reshape(q.shape)
                qa = post.abs().reshape(q.shape)
                r += 1
            else:
                q, qa = q.reshape(-1), qa.reshape(-1)
        out = float(res.primals[-1][b])
        assert abs(out - rec["out"]) <= 1e-6 * max(1.0, abs(rec["out"]))
        assert float(res.bound[b]) <= rec["out"] + 1e-6 or bool((c.masks[b] != -1).any())


def test_against_the_lp_on_the_toy_network(engine):
    """toy_kw, the root and the two children of its layer-1 split, 100 iterations: the device bound is at most HiGHS' optimum + 1e-6 and
    within 1e-3 (LP - iteration 0) of the twin's final value."""
    lp, doms = toy_kw_domains()
    doms = [doms[0], doms[3], doms[4]]
    B, gidx = len(doms), graph_index(lp)
    lbs = [torch.stack([b[0][i].reshape(-1) for _, _, b in doms]) for i in gidx]
    ubs = [torch.stack([b[1][i].reshape(-1) for _, _, b in doms]) for i in gidx]
    masks = torch.stack([torch.cat(m) for _, m, _ in doms]).to(torch.int8)
    x_lo, x_hi = lp.input_lb[None].expand(B, -1, -1, -1), lp.input_ub[None].expand(B, -1, -1, -1)
    res = engine.dual_ascent(lp.layers[:-1], [lp.layers[-1]] * B, x_lo, x_hi, masks, lbs, ubs, 100, LR)
    for row, (name, mask, b) in enumerate(doms):
        opt = lp._solve_lp([t.clone() for t in mask], b[0], b[1]).lb
        twin = lp.dual_ascent_host(b, mask, 100, lr=LR)
        got = float(res.bound[row])
        gap = opt - twin.values[0]
        print(f"{name}: LP {opt:.6f} iteration 0 {twin.values[0]:.6f} twin {twin.bound:.6f} device {got:.6f} closed {(got - twin.values[0]) / gap:.5f}")
        assert got <= opt + 1e-6, (name, got, opt)
        assert abs(got - twin.bound) <= 1e-3 * gap, (name, got, twin.bound, gap)


def test_kw_bounds_dual_ascent_and_the_scorer_on_device_arrays_only(engine):
    """gnnb_kw_bounds -> gnnb_dual_ascent -> gnnb_forward without a host round trip (the bound lands in the property entry of lb32):
    status 0, and the decisions GraphChoice.decision takes when fed the same arrays from the host."""
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    net = Net("cifar_base_kw")
    doms = [seeded_domain(net, i, seed0=3) for i in range(2)]
    choice = GraphChoice(doms[0].mask, CKPT)
    choice.verbose = False
    eng = choice.model.engine()
    c = Case(eng, "cifar_base_kw", doms)
    kw = c.kw
    da = eng.dual_ascent(c.net.fixed, c.props, c.x_lo, c.x_hi, c.masks, kw.lb, kw.ub, 20, LR, want_scorer_inputs=True,
                         lb32_prop=kw.lb32[-1])
    assert torch.equal(kw.lb32[-1].reshape(-1), da.bound.float())
    layers = {"fixed_layers": c.net.fixed, "prop_layers": c.props}
    amb = (c.masks == -1).float().to(eng.device)
    fwd = eng.forward(kw.lb32, kw.ub32, da.dual, da.primals, da.x_lp, layers, amb)
    assert int(fwd.status.cpu()[0]) == 0
    dec = fwd.decisions.cpu().tolist()
    B = len(c.doms)
    for b, d in enumerate(c.doms):
        host = choice.decision([t[b:b + 1].cpu() for t in kw.lb32], [t[b:b + 1].cpu() for t in kw.ub32],
                               [t.reshape(B, -1, 3)[b].cpu() for t in da.dual], da.x_lp[b:b + 1].cpu(),
                               [t.reshape(B, -1)[b].cpu() if t.numel() > 1 else t.cpu() for t in da.primals],
                               {"fixed_layers": c.net.fixed, "prop_layers": [c.props[b]]}, d.mask)
        assert dec[b] == host and dec[b][0] >= 0, (b, dec[b], host)


def test_threshold_loop_with_dual_device_children(engine):
    """branch_and_bound_threshold(child_lp="dual_device") on toy_kw: children bounded by dual ascent (sound, at or below their LPs) leave
    global_lb <= global_ub, at or below the network's output at every sampled point, and no verdict the LP loop contradicts."""
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
    lp0, _ = toy_kw_domains()
    runs = {}
    for mode in ("highs", "dual_device"):
        lp = lp_producer.LayerGraphLP(lp0.layers, lp0.input_lb.float(), lp0.input_ub.float(), bounds="kw_device", engine=engine)
        root_mask = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
        choice = GraphChoice(root_mask, CKPT)
        choice.verbose = False

        def kw(sub, icp, order, sparsest):
            return choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, order, sparsest)
        runs[mode] = lp_producer.branch_and_bound_threshold(lp, lp_producer.gnn_scorer(choice, lp), kw, lp.layers, max_branches=3,
                                                            log=lambda s: None, child_lp=mode)
    (hl, hu, hs, *_), (dl, du, ds, *_) = runs["highs"], runs["dual_device"]
    print("highs", runs["highs"], "dual_device", runs["dual_device"])
    assert ds >= 2 and dl <= du
    with torch.no_grad():                                  # the minimum lies at or below every sampled output
        x = lp0.input_lb.float() + (lp0.input_ub - lp0.input_lb).float() * torch.rand((256,) + lp0.shapes[0], generator=torch.Generator().manual_seed(0))
        for l in lp0.layers:
            x = l(x)
    assert dl <= float(x.min()) + 1e-5
    assert dl <= hu + 1e-6 and hl <= du + 1e-6             # each run's lower bound is below the other's upper bound: no verdict of one (lb >= 0:
    #                                                        the property holds; ub < 0: a counter-example) contradicts the other's


def test_limits(engine):
    """4096 nodes run; 4097 are refused before a launch and the handle stays usable; a short workspace is GNNB_E_NOMEM (-4); a negative
    iteration count GNNB_E_INVALID (-1)."""
    net = Net("kwg_cap")
    cap = Case(engine, "kwg_cap", [seeded_domain(net, i, seed0=51) for i in range(2)])
    res = cap.device(engine, 3)
    for b, d in enumerate(cap.doms):
        want = d.lp.dual_ascent_host(cap.bounds[b], d.mask, 3, lr=LR)
        assert abs(float(res.bound[b]) - want.bound) <= 1e-8 * max(1.0, abs(want.bound)), (b, float(res.bound[b]), want.bound)
    over = Net("kwg_over")
    d = seeded_domain(over, 0)
    hb = d.lp.kw_bounds(d.mask)
    gidx = graph_index(d.lp)
    mask = torch.cat(d.mask)[None].to(torch.int8)
    args = (over.fixed, [over.prop(d.gt, d.cls)], d.x_lo[None], d.x_hi[None], mask, [hb[0][i].reshape(1, -1) for i in gidx],
            [hb[1][i].reshape(1, -1) for i in gidx])
    with pytest.raises(RuntimeError, match=r"gnnb_dual_ascent failed \(-1\).*4097 nodes needs 65552 bytes of LDS"):
        engine.dual_ascent(*args, 3)
    with pytest.raises(RuntimeError, match=r"gnnb_dual_ascent failed \(-1\)"):
        cap.device(engine, -1)
    short = torch.empty(engine.dual_workspace(2).numel() - 8, dtype=torch.uint8, device=engine.device)
    with pytest.raises(RuntimeError, match=r"gnnb_dual_ascent failed \(-4\)"):
        cap.device(engine, 3, workspace=short)
    again = cap.device(engine, 3)
    assert torch.equal(again.bound, res.bound) and torch.equal(again.alpha, res.alpha)


def test_workspace_contents_do_not_matter(engine):
    c = case(engine, "kwg_rect")
    first = c.device(engine, 5, want_scorer_inputs=True, want_grad=True)
    engine.dual_workspace(len(c.doms)).fill_(0xFF)          # all-ones bytes: NaN doubles
    again = c.device(engine, 5, want_scorer_inputs=True, want_grad=True)
    for a, b in zip([first.bound, first.alpha, first.beta, first.grad_alpha, first.grad_beta, first.x_lp] + first.dual + first.primals,
                    [again.bound, again.alpha, again.beta, again.grad_alpha, again.grad_beta, again.x_lp] + again.dual + again.primals):
        assert torch.equal(a, b)
