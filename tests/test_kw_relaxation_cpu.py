"""The host Wong-Kolter bounds (LayerGraphLP._kw_layer, the reference tests/test_gpu_kw_geometry.py holds the device to) pinned to their
definition, on the CPU.  With the pre-activation bounds (l, u) of the ReLU layers below an affine layer fixed, every ambiguous ReLU is
relaxed to y = d z + t with d = u / (u - l) and t in [0, -d l], a passing one (l >= 0) to y = z and a blocked one to y = 0.  That network
is affine in (x, t), so its min / max over the input box x the t box is its value at (x_lo, 0) plus the Jacobian's entries times the
box widths, taken by sign.  _kw_layer computes the same numbers by the dual network's backward pass; here they come from
torch.autograd.functional.jacobian of the relaxed network's forward, in fp64, and the argmin is evaluated to show the bound is attained."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from gnn_branching_amd import lp_producer, nets
from tests.common import KW_ARCHS, register_kw_archs

SMALL_CONV = [("conv", 3, 8, 3, 1, 1), ("relu",), ("conv", 8, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 8 * 4 * 4, 16), ("relu",),
              ("linear", 16, 10)]


def network(name):
    if name == "kwg_relax_conv":
        nets.register_arch(name, SMALL_CONV, seed=401)
    else:
        register_kw_archs()
    return nets.load_verified_net(name, 2, 7), (3, 8, 8)


def make_lp(name, eps=0.05):
    layers, shape = network(name)
    x = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, shape))
    return lp_producer.LayerGraphLP(layers, x - eps, x + eps)


def relaxed_forward(lp, q, lbs, ubs, x, ts):
    """Output of affine layer q of the relaxed network at input x (flat) and offsets ts (one flat tensor per ReLU below q)."""
    a = x.reshape(lp.shapes[0])
    r = 0
    for i, l in enumerate(lp.layers[:q + 1]):
        if type(l) is nn.Conv2d:
            a = F.conv2d(a[None], l.weight.double(), l.bias.double(), l.stride, l.padding)[0]
        elif type(l) is nn.Linear:
            a = l.weight.double() @ a + l.bias.double()
        elif type(l) is nn.ReLU:
            lo, up = lbs[i].reshape(-1), ubs[i].reshape(-1)
            amb = (lo < 0) & (up > 0)
            d = torch.where(lo >= 0, torch.ones_like(lo), torch.zeros_like(lo))
            d = torch.where(amb, up / (up - lo), d)
            a = (d * a.reshape(-1) + torch.where(amb, ts[r], torch.zeros_like(lo))).reshape(a.shape)
            r += 1
        else:
            a = a.reshape(-1)
    return a.reshape(-1)


def relaxation_bounds(lp, q, lbs, ubs):
    """(lower, upper, argmin point) of affine layer q's outputs over the box x the t ranges, from the Jacobian."""
    relus = [i for i in lp.pre_relu_indices if i < q]
    gains = []
    for i in relus:
        lo, up = lbs[i].reshape(-1), ubs[i].reshape(-1)
        amb = (lo < 0) & (up > 0)
        gains.append(torch.where(amb, -(up / (up - lo)) * lo, torch.zeros_like(lo)))
    xl, xu = lp.input_lb.reshape(-1), lp.input_ub.reshape(-1)
    t0 = [torch.zeros_like(g) for g in gains]

    def f(x, *ts):
        return relaxed_forward(lp, q, lbs, ubs, x, list(ts))
    with torch.no_grad():
        base = f(xl, *t0)
    jac = torch.autograd.functional.jacobian(f, (xl, *t0))
    jx, jts = jac[0], jac[1:]
    wx = (xu - xl)[None]
    lower = base + (jx.clamp(max=0) * wx).sum(1)
    upper = base + (jx.clamp(min=0) * wx).sum(1)
    for jt, g in zip(jts, gains):
        lower = lower + (jt.clamp(max=0) * g[None]).sum(1)
        upper = upper + (jt.clamp(min=0) * g[None]).sum(1)
    # the argmin of node j: x_hi where its input gradient is negative, the top of t's range where its t gradient is
    arg_x = torch.where(jx < 0, xu[None], xl[None])
    arg_t = [torch.where(jt < 0, g[None], torch.zeros_like(jt)) for jt, g in zip(jts, gains)]
    return lower, upper, arg_x, arg_t


def domains(lp):
    """The root and a child split on ReLU layer 0 (one ambiguous node forced per ReLU layer, bounds intersected with the root's)."""
    root_mask = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
    root = lp.kw_bounds(root_mask)
    child_mask = [m.clone() for m in root_mask]
    for r, i in enumerate(lp.pre_relu_indices):
        amb = torch.nonzero((root[0][i].reshape(-1) < 0) & (root[1][i].reshape(-1) > 0)).reshape(-1)
        assert len(amb), r
        child_mask[r][int(amb[len(amb) // 2])] = r % 2
        child_mask[r][int(amb[0])] = 1 - r % 2
    return [("root", root), ("split", lp.kw_bounds(child_mask, root, 0))]


@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_relax_conv"])
def test_kw_layer_is_the_relaxations_min_and_max(name):
    lp = make_lp(name)
    checked = 0
    for dom, (lbs, ubs) in domains(lp):
        for q, l in enumerate(lp.layers):
            if type(l) not in (nn.Conv2d, nn.Linear):
                continue
            kl, ku = lp._kw_layer(q, lbs + [None], ubs + [None])
            lower, upper, arg_x, arg_t = relaxation_bounds(lp, q, lbs, ubs)
            scale = max(1.0, float(lower.abs().max()), float(upper.abs().max()))
            assert float((kl.reshape(-1) - lower).abs().max()) <= 1e-10 * scale, (dom, q)
            assert float((ku.reshape(-1) - upper).abs().max()) <= 1e-10 * scale, (dom, q)
            # the lower bound is attained: the relaxed network at node j's argmin gives node j's bound
            with torch.no_grad():
                for j in np.random.RandomState(q).choice(len(lower), size=min(24, len(lower)), replace=False):
                    v = relaxed_forward(lp, q, lbs, ubs, arg_x[j], [t[j] for t in arg_t])[j]
                    assert abs(float(v) - float(lower[j])) <= 1e-10 * scale, (dom, q, int(j))
            checked += 1
    assert checked == 2 * sum(1 for l in lp.layers if type(l) in (nn.Conv2d, nn.Linear))


def test_kw_archs_shapes():
    """Every KW_ARCHS entry builds, folds and has the layer sizes its comment promises (host side, no GPU)."""
    register_kw_archs()
    for name, (shape, _) in KW_ARCHS.items():
        layers = nets.load_verified_net(name, 3, 5)
        lp = lp_producer.LayerGraphLP(layers, torch.zeros(shape), torch.ones(shape))
        widest = max(int(np.prod(lp.shapes[i + 1])) for i in lp.pre_relu_indices)
        assert widest == {"kwg_cap": 4096, "kwg_over": 4097}.get(name, min(widest, 4096)), name
    assert len(make_lp("kwg_deep8").pre_relu_indices) == 8
