"""Tightened intermediate bounds on the MI355X (ScorerEngine.kw_bounds(tighten=n) -> gnnb_kw_tighten) against the
host fp64 twin LayerGraphLP.kw_bounds(tighten=n), on the geometries of tests/common.py KW_ARCHS: n_iter = 0 is gnnb_kw_bounds bit for bit;
five iterations agree with the twin within the bar the property row's ascent is held to; a domain's bounds depend neither on B nor on its
row; a child keeps its parent's layers; the counts are the twin's; the exact node extrema stay inside at n_iter = 20.

The boxes are small (BOX) so that every batch has few ambiguous nodes above layer 1: the twin walks them one by one."""
import numpy as np
import pytest
import torch

from tests import exact_minimum as E
from tests import margins
from tests.test_gpu_kw_geometry import Domain, Net, device_row, force_nodes, graph_index

pytestmark = pytest.mark.gpu

# eps of the root boxes per network: the smallest networks take the fixture's boxes, the conv stacks one that leaves tens of nodes ambiguous
BOX = {"kwg_mlp": 0.02, "kwg_gap": 0.01, "kwg_s1": 0.0015, "kwg_rect": 0.004, "kwg_deep8": 0.002, "kwg_single": 0.01, "kwg_cap": 0.003}
BAR = 1e-8
_shared = {}


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    from tests.common import register_kw_archs
    register_kw_archs()
    return ScorerEngine(None)


def batch_of(name):
    """B = 6 on one network: two roots, two domains with forced nodes in every ReLU layer, two children (split in the first and in the
    last ReLU layer) with their root's plain bounds as the parent's; every domain has its own centre and property."""
    if name not in _shared:
        from tests.common import register_kw_archs
        register_kw_archs()
        net, eps = Net(name), BOX[name]
        rng = np.random.RandomState(3)
        doms = [Domain(net, 11 + 97 * i, eps * (1.0 + 0.25 * (i % 2)), i % 10, (i + 3) % 10) for i in range(6)]
        for d in doms[2:4]:
            force_nodes(d, rng, 2)
        L = len(doms[0].mask)
        for j, d in enumerate(doms[4:]):
            d.parent = d.lp.kw_bounds(d.mask)
            d.split = j * (L - 1) if L > 1 else 0
            i = d.lp.pre_relu_indices[d.split]
            amb = torch.nonzero((d.parent[0][i].reshape(-1) < 0) & (d.parent[1][i].reshape(-1) > 0)).reshape(-1)
            if len(amb):
                d.mask[d.split][int(amb[len(amb) // 2])] = j % 2
        _shared[name] = doms
    return _shared[name]


def twin_of(name, b, n_iter):
    """(bounds, report) of domain b of the batch on the host, computed once."""
    key = (name, b, n_iter)
    if key not in _shared:
        d, report = batch_of(name)[b], {}
        _shared[key] = (d.lp.kw_bounds(d.mask, d.parent, d.split, tighten=n_iter, report=report), report)
    return _shared[key]


def run(engine, doms, tighten=0, want_fp32=False):
    net, lp = doms[0].net, doms[0].lp
    x_lo, x_hi = torch.stack([d.x_lo for d in doms]), torch.stack([d.x_hi for d in doms])
    masks = torch.stack([torch.cat([m.reshape(-1) for m in d.mask]) for d in doms]).to(torch.int8)
    parents = split = None
    gidx = graph_index(lp)
    if any(d.parent is not None for d in doms):
        sizes = [int(np.prod(lp.shapes[i])) for i in gidx]
        parents = tuple([torch.stack([d.parent[side][i].reshape(-1) if d.parent is not None else torch.zeros(n, dtype=torch.float64)
                                      for d in doms]) for i, n in zip(gidx, sizes)] for side in (0, 1))
        split = torch.tensor([d.split if d.parent is not None else -1 for d in doms], dtype=torch.int32)
    return engine.kw_bounds(net.fixed, [net.prop(d.gt, d.cls) for d in doms], x_lo, x_hi, masks, parents, split, want_fp32=want_fp32, tighten=tighten)


def device_of(engine, name, n_iter):
    key = ("device", name, n_iter)
    if key not in _shared:
        _shared[key] = run(engine, batch_of(name), n_iter, want_fp32=True)
    return _shared[key]


def all_equal(x, y, rows_x=slice(None), rows_y=slice(None)):
    return all(torch.equal(s[rows_x], t[rows_y]) for s, t in zip(x.lb + x.ub + x.lb32 + x.ub32 + [x.infeasible], y.lb + y.ub + y.lb32 + y.ub32 + [y.infeasible]))


NETWORKS = ["kwg_mlp", "kwg_gap", "kwg_s1", "kwg_rect", "kwg_deep8", "kwg_single", "kwg_cap"]


@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_s1", "kwg_single"])
def test_no_iterations_is_gnnb_kw_bounds_bit_for_bit(name, engine):
    """The entry point itself at n_iter = 0 (ScorerEngine.kw_bounds dispatches to it from tighten = 1 on), counts given: all zero."""
    import ctypes as C
    from gnn_branching_amd import _lib
    from gnn_branching_amd.engine import table
    doms = batch_of(name)
    plain = run(engine, doms, 0, want_fp32=True)
    one = run(engine, doms, 1, want_fp32=True)             # the same call at n_iter = 1 leaves the arguments to repeat at n_iter = 0
    B, dev = len(doms), engine.device
    net = doms[0].net
    Bq, xl, xu, mask, pw, pb = engine._domains(net.fixed, [net.prop(d.gt, d.cls) for d in doms], torch.stack([d.x_lo for d in doms]),
                                               torch.stack([d.x_hi for d in doms]),
                                               torch.stack([torch.cat([m.reshape(-1) for m in d.mask]) for d in doms]).to(torch.int8))
    gidx = graph_index(doms[0].lp)
    plb = [torch.stack([(d.parent[0][i] if d.parent is not None else torch.zeros(doms[0].lp.shapes[i], dtype=torch.float64)).reshape(-1)
                        for d in doms]).to(dev) for i in gidx]
    pub = [torch.stack([(d.parent[1][i] if d.parent is not None else torch.zeros(doms[0].lp.shapes[i], dtype=torch.float64)).reshape(-1)
                        for d in doms]).to(dev) for i in gidx]
    split = torch.tensor([d.split if d.parent is not None else -1 for d in doms], dtype=torch.int32, device=dev)
    lb, ub = [torch.empty_like(t) for t in plain.lb], [torch.empty_like(t) for t in plain.ub]
    lb32, ub32 = [torch.empty_like(t) for t in plain.lb32], [torch.empty_like(t) for t in plain.ub32]
    infeasible = torch.full((B,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    ws, tws = engine.kw_workspace(B), engine.kw_tighten_workspace(B)
    kb = _lib.KwBatch(xl.data_ptr(), xu.data_ptr(), pw.data_ptr(), pb.data_ptr(), mask.data_ptr(), table(plb), table(pub), split.data_ptr(), len(gidx) + 1)
    engine._call("gnnb_kw_tighten", C.byref(kb), B, 0, 0.1, table(lb), table(ub), table(lb32), table(ub32), infeasible.data_ptr(), counts.data_ptr(),
                 ws.data_ptr(), ws.numel(), tws.data_ptr(), tws.numel())
    from gnn_branching_amd.engine import KwBoundsResult
    assert all_equal(KwBoundsResult(lb, ub, lb32, ub32, infeasible), plain)
    assert counts.cpu().tolist() == [[0, 0]] * B
    assert one.counts is not None and plain.counts is None


def kinks_of(lp, report, want):
    """Objectives the bar does not bind: (graph layer entry, node, side) of every ascent that met 0 < |lambda| < 1e-12, and of every
    ascent above a layer one of whose bounds lies within the bar of 0 (its node changes state between the two sides)."""
    out = set()
    gidx = graph_index(lp)
    lowest = None
    for i in gidx[:-1]:
        wl, wu = want[0][i].reshape(-1), want[1][i].reshape(-1)
        tol = BAR * max(1.0, float(wl.abs().max()), float(wu.abs().max()))
        if bool((((wl != 0) & (wl.abs() <= tol)) | ((wu != 0) & (wu.abs() <= tol))).any()):
            lowest = i
            break
    for i, j, sign, tiny in report["objectives"]:
        if tiny < 1e-12 or (lowest is not None and i > lowest):
            out.add((i, j, 0 if sign > 0 else 1))
    return out


@pytest.mark.parametrize("name", NETWORKS)
def test_five_iterations_match_the_twin(name, engine):
    """Every bound within 1e-8 max(1, max |bound| of its layer) of the twin's; ambiguous and decided sets identical outside that bar
    (tests/test_gpu_kw_geometry.py compare, at this bar); the counts are the twin's.  Left out, counted and capped at 1 % of a domain's
    tightened bounds: the objectives of ``kinks_of``."""
    doms = batch_of(name)
    res = device_of(engine, name, 5)
    counts = res.counts.cpu().tolist()
    worst, n_kinks, n_obj = 0.0, 0, 0
    for b, d in enumerate(doms):
        want, report = twin_of(name, b, 5)
        got = device_row(res, b)
        gidx = graph_index(d.lp)
        kinks = kinks_of(d.lp, report, want)
        n_kinks += len(kinks)
        n_obj += len(report["objectives"])
        assert len(kinks) <= 0.01 * len(report["objectives"]), (name, b, len(kinks), len(report["objectives"]))
        for side in (0, 1):
            for g, i in enumerate(gidx):
                w = want[side][i].reshape(-1)
                tol = BAR * max(1.0, float(w.abs().max()))
                err = (got[side][g] - w).abs()
                for (ki, kj, ks) in kinks:
                    if ki == i and ks == side:
                        err[kj] = 0.0
                worst = max(worst, float(err.max()) / max(1.0, float(w.abs().max())))
                print(f"{name} row {b} side {side} layer {g}: max error {float(err.max()):.3e} (bar {tol:.3e})")
                assert float(err.max()) <= tol, (name, b, side, g, float(err.max()), tol)
        for g, i in enumerate(gidx[:-1]):
            gl, gu, wl, wu = got[0][g], got[1][g], want[0][i].reshape(-1), want[1][i].reshape(-1)
            tol = BAR * max(1.0, float(wl.abs().max()), float(wu.abs().max()))
            keep = ~(((wl != 0) & (wl.abs() <= tol)) | ((wu != 0) & (wu.abs() <= tol)))
            assert torch.equal(((gl < 0) & (gu > 0))[keep], ((wl < 0) & (wu > 0))[keep]), (name, b, g)
            assert torch.equal((gl >= 0)[keep], (wl >= 0)[keep]) and torch.equal((gu <= 0)[keep], (wu <= 0)[keep]), (name, b, g)
        if not kinks:
            assert counts[b] == report["counts"], (name, b, counts[b], report["counts"])
    ran = sum(c[0] for c in counts)
    print(f"{name}: {ran} nodes tightened, {sum(c[1] for c in counts)} decided, {n_kinks} of {n_obj} objectives at a kink, worst error / bar {worst / BAR:.3e}")
    margins.record("kw_tighten", name, n_rows=len(doms), n_nodes=ran, n_kinks=n_kinks, worst_over_bar=worst / BAR)
    if name != "kwg_single":
        assert ran > 0, "no node of the batch was ambiguous above layer 1: the case tests nothing"
    else:
        assert ran == 0
        plain = run(engine, doms, 0, want_fp32=True)
        assert all_equal(res, plain)


def test_a_layer_past_the_cap_is_refused(engine):
    net = Net("kwg_over")
    d = Domain(net, 5, 0.001, 3, 5)
    with pytest.raises(RuntimeError, match=r"gnnb_kw_tighten failed \(-1\).*4097 nodes needs"):
        run(engine, [d], 5)


@pytest.mark.parametrize("name", ["kwg_gap", "kwg_s1"])
def test_alone_and_permuted(name, engine):
    """A domain alone equals its row of the batch, a permuted batch equals the permutation, bit for bit (fp64, fp32, flags, counts)."""
    doms = batch_of(name)
    res = device_of(engine, name, 5)
    for b in (1, 3, 5):
        one = run(engine, [doms[b]], 5, want_fp32=True)
        assert all_equal(res, one, slice(b, b + 1), slice(0, 1)), (name, b)
        assert torch.equal(res.counts[b:b + 1], one.counts)
    perm = [4, 2, 5, 0, 3, 1]
    shuffled = run(engine, [doms[p] for p in perm], 5, want_fp32=True)
    idx = torch.tensor(perm, device=engine.device)
    assert all_equal(shuffled, res, slice(None), idx)
    assert torch.equal(shuffled.counts, res.counts[idx])


@pytest.mark.parametrize("name", ["kwg_s1", "kwg_deep8"])
def test_a_child_keeps_its_parents_layers(name, engine):
    """Up to the split layer the parent's bits (the split node clamped); above, inside the parent's; and nothing ran for a copied layer:
    the child split in the last ReLU layer copies every layer the ascent could run for, so its counts are zero."""
    doms = batch_of(name)
    res = device_of(engine, name, 5)
    plain = run(engine, doms, 0)
    for b in (4, 5):
        d = doms[b]
        got, base = device_row(res, b), device_row(plain, b)
        for g, i in enumerate(graph_index(d.lp)):
            plo, pup = d.parent[0][i].reshape(-1), d.parent[1][i].reshape(-1)
            if i <= d.lp.pre_relu_indices[d.split]:
                assert torch.equal(got[0][g], base[0][g]) and torch.equal(got[1][g], base[1][g]), (name, b, g)
            else:
                assert bool((got[0][g] >= plo).all()) and bool((got[1][g] <= pup).all()), (name, b, g)
                assert bool((got[0][g] >= base[0][g]).all()) and bool((got[1][g] <= base[1][g]).all()), (name, b, g)
    assert res.counts[5].cpu().tolist() == [0, 0]
    assert int(res.counts[4, 0]) > 0


@pytest.mark.parametrize("network", sorted({e["network"] for e in E.load().values()}))
def test_exact_node_extrema_stay_inside_at_twenty_iterations(network, engine):
    """The stored exact extrema of nodes of the last ReLU layer (tests/golden/exact_minima.npz) lie inside the device's tightened root
    bounds with the fixture's slack, and no bound is looser than gnnb_kw_bounds'."""
    fix = {c: e for c, e in E.load().items() if e["network"] == network}
    net = Net(network)
    for case, e in fix.items():
        lp = E.case_lp(case, e)
        d = Domain(net, 0, 0.0, *(int(v) for v in e["prop"]))
        d.x_lo, d.x_hi, d.lp = lp.input_lb, lp.input_ub, lp
        d.mask = E.root_mask(lp)
        res, plain = run(engine, [d], 20), run(engine, [d], 0)
        k = int(e["node_layer"])
        for node, (lo0, lo1, hi0, hi1) in zip(e["nodes"], e["node_extrema"]):
            lo, up = float(res.lb[k][0][node]), float(res.ub[k][0][node])
            assert lo <= lo1 + E.slack(lo1) and up >= hi0 - E.slack(hi0), (case, int(node), lo, up, lo1, hi0)
        for x, y in zip(res.lb, plain.lb):
            assert bool((x >= y).all()), case
        for x, y in zip(res.ub, plain.ub):
            assert bool((x <= y).all()), case
