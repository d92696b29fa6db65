"""Wong-Kolter bounds on the MI355X (ScorerEngine.kw_bounds -> gnnb_kw_bounds) against the host fp64 LayerGraphLP.kw_bounds on every
geometry of tests/common.py KW_ARCHS and the three CIFAR networks.  Unlike tests/test_gpu_kw_bounds.py, every domain of a batch has its own
input box and its own folded property layer, and the host reference is built per domain with them: a kernel that read one domain's box
or property for another fails here.  Also: a split at every ReLU layer, a parent intersection that binds, B = 300, the infeasible flag in a
mixed batch, the 4096-node LDS limit on both sides, and the argument checks of kw_bounds / bounds."""
import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import lp_producer, nets
from tests import margins
from tests.common import KW_ARCHS, register_kw_archs, register_toy_archs

pytestmark = pytest.mark.gpu

CIFAR = ["cifar_base_kw", "cifar_wide_kw", "cifar_deep_kw"]
EPS = (0.01, 0.03, 0.05)


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    return ScorerEngine(None)


def input_shape(name):
    return KW_ARCHS[name][0] if name in KW_ARCHS else nets.INPUT_SHAPE


class Net:
    """One network: its fixed layers (shared by every domain) and its folded property layers by (gt, cls)."""

    def __init__(self, name, layers=None):
        self.name, self.shape = name, input_shape(name)
        self.base = layers if layers is not None else nets.build_net(name)
        self.fixed = self.base[:-1]
        self._props = {}

    def prop(self, gt, cls):
        if (gt, cls) not in self._props:
            self._props[(gt, cls)] = nets.fold_property(self.base, gt, cls)[-1]
        return self._props[(gt, cls)]

    def lp(self, x_lo, x_hi, gt, cls):
        return lp_producer.LayerGraphLP(self.fixed + [self.prop(gt, cls)], x_lo, x_hi)


class Domain:
    """One BaB domain: box, property, split mask, optional parent bounds (host list form) and split layer."""

    def __init__(self, net, seed, eps, gt, cls):
        x = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, net.shape))
        self.net, self.gt, self.cls = net, gt, cls
        self.x_lo, self.x_hi = x - eps, x + eps
        self.lp = net.lp(self.x_lo, self.x_hi, gt, cls)
        self.mask = [torch.full((int(np.prod(self.lp.shapes[i + 1])),), -1, dtype=torch.long) for i in self.lp.pre_relu_indices]
        self.parent = self.split = None

    def host(self):
        return self.lp.kw_bounds(self.mask, self.parent, self.split)


def seeded_domain(net, i, seed0=0):
    gt = i % 10
    return Domain(net, seed0 + 97 * i + 1, EPS[i % 3], gt, (gt + 1 + i // 10) % 10)


def force_nodes(dom, rng, per_layer):
    """Force `per_layer` nodes of each ReLU layer that interval arithmetic leaves ambiguous (passing or blocked at random)."""
    il, iu = dom.lp.interval_bounds(dom.mask)
    for r, i in enumerate(dom.lp.pre_relu_indices):
        amb = torch.nonzero((il[i].reshape(-1) < 0) & (iu[i].reshape(-1) > 0)).reshape(-1).numpy()
        for node in rng.choice(amb, size=min(per_layer, len(amb)), replace=False):
            dom.mask[r][int(node)] = int(rng.randint(2))


def graph_index(lp):
    return list(lp.pre_relu_indices) + [len(lp.layers)]


def run_device(engine, doms, want_fp32=False):
    """One gnnb_kw_bounds call for the domains, each with its own box, property, mask and parent."""
    net = doms[0].net
    B = len(doms)
    x_lo = torch.stack([d.x_lo for d in doms])
    x_hi = torch.stack([d.x_hi for d in doms])
    masks = torch.stack([torch.cat([m.reshape(-1) for m in d.mask]) for d in doms]).to(torch.int8)
    parents = split = None
    gidx = graph_index(doms[0].lp)
    if any(d.parent is not None for d in doms):
        sizes = [int(np.prod(doms[0].lp.shapes[i])) for i in gidx]
        parents = tuple([torch.stack([d.parent[side][i].reshape(-1) if d.parent is not None else torch.zeros(n, dtype=torch.float64)
                                      for d in doms]) for i, n in zip(gidx, sizes)] for side in (0, 1))
        split = torch.tensor([d.split if d.parent is not None else -1 for d in doms], dtype=torch.int32)
    res = engine.kw_bounds(net.fixed, [net.prop(d.gt, d.cls) for d in doms], x_lo, x_hi, masks, parents, split, want_fp32=want_fp32)
    return res


def device_row(res, b):
    return [t[b].cpu() for t in res.lb], [t[b].cpu() for t in res.ub]


def compare(lp, got, want, what):
    """Every graph layer within 1e-9 max(1, max|bound| of the layer); ambiguous / decided sets identical except for nodes whose bound
    lies within that bar of 0.  Returns the number of such nodes."""
    near = 0
    gidx = graph_index(lp)
    for side in (0, 1):
        for g, i in enumerate(gidx):
            w = want[side][i].reshape(-1)
            tol = 1e-9 * max(1.0, float(w.abs().max()))
            err = float((got[side][g] - w).abs().max())
            assert err <= tol, (what, side, g, err, tol)
    for g, i in enumerate(gidx[:-1]):
        gl, gu, wl, wu = got[0][g], got[1][g], want[0][i].reshape(-1), want[1][i].reshape(-1)
        tol = 1e-9 * max(1.0, float(wl.abs().max()), float(wu.abs().max()))
        edge = ((wl != 0) & (wl.abs() <= tol)) | ((wu != 0) & (wu.abs() <= tol))       # (a clamped bound is 0 exactly on both sides)
        near += int(edge.sum())
        keep = ~edge
        assert torch.equal(((gl < 0) & (gu > 0))[keep], ((wl < 0) & (wu > 0))[keep]), (what, g)
        assert torch.equal((gl >= 0)[keep], (wl >= 0)[keep]) and torch.equal((gu <= 0)[keep], (wu <= 0)[keep]), (what, g)
    return near


def mixed_batch(net, seed0=0):
    """B = 6: two roots, two domains with 2-3 forced nodes per ReLU layer, two children with a parent and a split; every domain has
    its own centre, eps and (gt, cls)."""
    rng = np.random.RandomState(seed0 + 5)
    doms = [seeded_domain(net, i, seed0) for i in range(6)]
    for d in doms[2:4]:
        force_nodes(d, rng, 2 + int(rng.randint(2)))
    L = len(doms[0].mask)
    for j, d in enumerate(doms[4:]):
        d.parent = d.lp.kw_bounds(d.mask)
        d.split = (j * (L - 1)) if L > 1 else 0           # the first and the last ReLU layer
        i = d.lp.pre_relu_indices[d.split]
        amb = torch.nonzero((d.parent[0][i].reshape(-1) < 0) & (d.parent[1][i].reshape(-1) > 0)).reshape(-1)
        if len(amb):
            d.mask[d.split][int(amb[len(amb) // 2])] = j % 2
    return doms


GEOMETRIES = [n for n in KW_ARCHS if n != "kwg_over"] + CIFAR


@pytest.mark.parametrize("name", GEOMETRIES)
def test_mixed_batch_matches_the_host_per_domain(name, engine):
    net = Net(name)
    doms = mixed_batch(net)
    res = run_device(engine, doms)
    near = 0
    for b, d in enumerate(doms):
        near += compare(d.lp, device_row(res, b), d.host(), (name, b))
    margins.record("kw_geometry", name, n_rows=len(doms), n_near_zero=near)
    assert near <= 3, near


@pytest.mark.parametrize("name", GEOMETRIES)
def test_split_at_every_relu_layer(name, engine):
    net = Net(name)
    root = seeded_domain(net, 2, seed0=11)
    parent = root.host()
    doms = []
    for s, i in enumerate(root.lp.pre_relu_indices):
        amb = torch.nonzero((parent[0][i].reshape(-1) < 0) & (parent[1][i].reshape(-1) > 0)).reshape(-1)
        assert len(amb), s
        for choice in (0, 1):
            d = seeded_domain(net, 2, seed0=11)
            d.mask[s][int(amb[len(amb) // 3])] = choice
            d.parent, d.split = parent, s
            doms.append(d)
    res = run_device(engine, doms)
    for b, d in enumerate(doms):
        want = d.host()
        got = device_row(res, b)
        compare(d.lp, got, want, (name, d.split))
        for g, i in enumerate(graph_index(d.lp)):
            if i <= d.lp.pre_relu_indices[d.split]:       # at or below the split: the parent's, bit for bit (the split node clamped)
                for side in (0, 1):
                    assert torch.equal(got[side][g], want[side][i].reshape(-1)), (name, d.split, side, g)


@pytest.mark.parametrize("name", ["kwg_s1", "kwg_rect", "kwg_deep8", "cifar_base_kw"])
def test_a_binding_parent_intersection(name, engine):
    """The parent is the child's own fresh bounds, each shrunk 10 % toward its midpoint above the split layer: the intersection must
    change the recomputed bounds, on the device as on the host."""
    net = Net(name)
    d = seeded_domain(net, 4, seed0=23)
    force_nodes(d, np.random.RandomState(1), 1)
    d.mask = [m.clone() for m in d.mask]
    fresh = d.lp.kw_bounds(d.mask)
    split = 0
    keep = d.lp.pre_relu_indices[split]
    plb, pub = [], []
    for i, (lo, up) in enumerate(zip(*fresh)):
        if i > keep:
            w = up - lo
            lo, up = lo + 0.05 * w, up - 0.05 * w
        plb.append(lo.clone())
        pub.append(up.clone())
    d.parent, d.split = (plb, pub), split
    want = d.host()
    res = run_device(engine, [d])
    compare(d.lp, device_row(res, 0), want, name)
    for i in graph_index(d.lp):
        if i > keep:
            changed = (want[0][i] != fresh[0][i]) | (want[1][i] != fresh[1][i])
            assert bool(changed.any()), (name, i)
    infeasible = any(bool((lo > up + 1e-9).any()) for lo, up in zip(*want))
    assert res.infeasible.cpu().tolist() == [int(infeasible)]


def test_batch_of_300(engine):
    """blockIdx.y past the CU count: sampled rows equal their own B = 1 call bit for bit and the host."""
    net = Net("cifar_base_kw")
    rng = np.random.RandomState(7)
    doms = []
    for i in range(300):
        d = seeded_domain(net, i, seed0=31)
        if i % 3 == 1:
            force_nodes(d, rng, 2)
        doms.append(d)
    roots = run_device(engine, doms)                      # the children's parents: their own root bounds (any parent does)
    for i in range(2, 300, 3):
        d = doms[i]
        lbs, ubs = device_row(roots, i)
        gidx = graph_index(d.lp)
        full = [[None] * (len(d.lp.layers) + 1) for _ in range(2)]
        for g, k in enumerate(gidx):
            full[0][k], full[1][k] = lbs[g], ubs[g]
        d.parent, d.split = tuple(full), i % len(d.mask)
        s = d.lp.pre_relu_indices[d.split]
        amb = torch.nonzero((lbs[gidx.index(s)] < 0) & (ubs[gidx.index(s)] > 0)).reshape(-1)
        if len(amb):
            d.mask[d.split][int(amb[0])] = i % 2
    res = run_device(engine, doms)
    for b in (0, 1, 2, 149, 298, 299):
        one = run_device(engine, [doms[b]])
        for side in (0, 1):
            assert all(torch.equal(x[b], y[0]) for x, y in zip((res.lb, res.ub)[side], (one.lb, one.ub)[side])), (b, side)
        want = doms[b].lp.kw_bounds(doms[b].mask, *(_host_parent(doms[b])))
        compare(doms[b].lp, device_row(res, b), want, b)


def _host_parent(d):
    """A parent in the host's list form (kw_bounds reads the affine outputs of the list only)."""
    if d.parent is None:
        return None, None
    lbs, ubs = d.parent
    out = ([], [])
    for side, src in ((0, lbs), (1, ubs)):
        for i, t in enumerate(src):
            out[side].append(t.reshape(d.lp.shapes[i]).double() if t is not None else None)
    return out, d.split


def test_infeasible_flag_in_a_mixed_batch(engine):
    """Rows [feasible, infeasible by split, infeasible by box, feasible] -> [0, 1, 1, 0], as LayerGraphLP.solve decides."""
    net = Net("kwg_mlp")
    doms = [seeded_domain(net, i, seed0=41) for i in range(4)]
    root = doms[1].host()
    i0 = doms[1].lp.pre_relu_indices[0]
    dead = torch.nonzero(root[1][i0].reshape(-1) < -1e-6).reshape(-1)
    assert len(dead)
    doms[1].mask[0][int(dead[0])] = 1                     # forced passing a node that is always blocked
    doms[2].x_lo = doms[2].x_lo.clone()
    doms[2].x_lo.view(-1)[17] = doms[2].x_hi.view(-1)[17] + 1e-8 + 1e-9
    doms[2].lp = net.lp(doms[2].x_lo, doms[2].x_hi, doms[2].gt, doms[2].cls)
    res = run_device(engine, doms)
    assert res.infeasible.cpu().tolist() == [0, 1, 1, 0]
    for mode in ("kw", "kw_device"):
        solved = [lp_producer.LayerGraphLP(d.lp.layers, d.x_lo, d.x_hi, bounds=mode, engine=engine).solve(d.mask) for d in doms]
        assert [s is None for s in solved] == [False, True, True, False], mode


def test_lds_limit_accepts_4096_nodes(engine):
    net = Net("kwg_cap")
    doms = [seeded_domain(net, i, seed0=51) for i in range(3)]
    force_nodes(doms[2], np.random.RandomState(2), 3)
    res = run_device(engine, doms)
    for b, d in enumerate(doms):
        compare(d.lp, device_row(res, b), d.host(), b)


@pytest.mark.parametrize("name", ["kwg_over", "toy_conv3"])
def test_lds_limit_refuses_wider_layers(name, engine):
    """Refused in gnnb_kw_bounds before any launch: GNNB_E_INVALID (-1), naming the LDS the dual pass would need."""
    net = Net(name)
    d = seeded_domain(net, 0)
    widest = max(int(np.prod(d.lp.shapes[i])) for i in d.lp.pre_relu_indices)
    need = 2 * widest * 8
    with pytest.raises(RuntimeError, match=rf"gnnb_kw_bounds failed \(-1\).*{widest} nodes needs {need} bytes of LDS"):
        run_device(engine, [d])
    lp = lp_producer.LayerGraphLP(d.lp.layers, d.x_lo, d.x_hi, bounds="kw_device", engine=engine)
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        lp.solve(d.mask)


def test_flat_box_on_a_conv_network_is_refused(engine):
    net = Net("cifar_base_kw")
    d = seeded_domain(net, 0)
    masks = torch.full((2, engine_relu_count(d)), -1, dtype=torch.int8)
    x = torch.stack([d.x_lo, d.x_hi]).reshape(2, -1)
    with pytest.raises(ValueError, match="Conv2d.*\\(B, C, H, W\\)"):
        engine.kw_bounds(net.fixed, [net.prop(3, 5)] * 2, x, x + 0.1, masks)
    # a Linear-first network takes the flat box (and the same bounds as the shaped one)
    mlp = Net("kwg_mlp")
    m = seeded_domain(mlp, 0)
    R = engine_relu_count(m)
    a = engine.kw_bounds(mlp.fixed, [mlp.prop(3, 5)], m.x_lo[None], m.x_hi[None], torch.full((1, R), -1, dtype=torch.int8))
    b = engine.kw_bounds(mlp.fixed, [mlp.prop(3, 5)], m.x_lo.reshape(1, -1), m.x_hi.reshape(1, -1), torch.full((1, R), -1, dtype=torch.int8))
    assert all(torch.equal(x, y) for x, y in zip(a.lb + a.ub, b.lb + b.ub))


def engine_relu_count(d):
    return sum(int(np.prod(d.lp.shapes[i])) for i in d.lp.pre_relu_indices)
