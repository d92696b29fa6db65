"""CPU: the host twin of gnnb_dual_ascent (LayerGraphLP.dual_value / dual_ascent_host / dual_recover, torch fp64) against HiGHS on
the toy Wong-Kolter network of tests/test_lp_producer.py -- the root and the median ambiguous node of each ReLU layer split both
ways -- and the new entry points' argument checks that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, lp_producer, nets

KW_SPEC = [("conv", 3, 4, 4, 2, 1), ("relu",), ("conv", 4, 4, 4, 2, 1), ("relu",), ("flatten",), ("linear", 4 * 8 * 8, 24), ("relu",),
           ("linear", 24, 10)]


def toy_kw_domains():
    """(lp, [(name, mask, bounds)]): toy_kw (seed 77, property (2, 6), x from RandomState(9), eps 0.04), the root and six children."""
    nets.register_arch("toy_kw", KW_SPEC, seed=77)
    layers = nets.load_verified_net("toy_kw", 2, 6)
    x = torch.from_numpy(np.random.RandomState(9).standard_normal((3, 32, 32)).astype(np.float32))
    lp = lp_producer.LayerGraphLP(layers, x - 0.04, x + 0.04)
    root = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
    rb = lp.kw_bounds(root)
    doms = [("root", root, rb)]
    for r, i in enumerate(lp.pre_relu_indices):
        amb = torch.nonzero((rb[0][i].reshape(-1) < 0) & (rb[1][i].reshape(-1) > 0)).reshape(-1)
        node = int(amb[len(amb) // 2])
        for choice, what in ((0, "blocked"), (1, "passing")):
            m = [t.clone() for t in root]
            m[r][node] = choice
            doms.append((f"layer {r} node {node} {what}", m, lp.kw_bounds(m, rb, r)))
    return lp, doms


@pytest.fixture(scope="module")
def solved():
    """Per domain: (name, mask, bounds, LP optimum, the twin's 100 iterations at lr 0.1) -- computed once."""
    lp, doms = toy_kw_domains()
    out = []
    for name, mask, b in doms:
        sub = lp._solve_lp([t.clone() for t in mask], b[0], b[1])
        assert sub is not None, name
        out.append((name, mask, b, sub.lb, lp.dual_ascent_host(b, mask, 100, lr=0.1)))
    return lp, out


def test_the_domains_are_the_seven_of_the_design_note(solved):
    lp, out = solved
    assert [n for n, *_ in out] == ["root", "layer 0 node 484 blocked", "layer 0 node 484 passing", "layer 1 node 162 blocked",
                                    "layer 1 node 162 passing", "layer 2 node 11 blocked", "layer 2 node 11 passing"]


def test_every_iterate_is_a_lower_bound_of_the_lp(solved):
    """HiGHS' own tolerances are 1e-7; the twin's g never exceeds its optimum by more than 1e-6."""
    _, out = solved
    for name, _, _, opt, res in out:
        assert len(res.values) == 101
        assert max(res.values) <= opt + 1e-6, (name, max(res.values), opt)


def test_iteration_0_of_the_root_is_the_kw_property_bound(solved):
    lp, out = solved
    _, mask, b, _, res = out[0]
    kl, _ = lp._kw_layer(len(lp.layers) - 1, b[0], b[1])
    assert abs(res.values[0] - float(kl)) <= 1e-12, (res.values[0], float(kl))
    assert lp.dual_ascent_host(b, mask, 0).bound == res.values[0]


def test_best_value_does_not_decrease_and_closes_the_gap(solved):
    """After 100 iterations at lr 0.1 at least 99.9 % of (LP - iteration 0) is closed on every domain (measured: 99.990 % or more)."""
    lp, out = solved
    for name, mask, b, opt, res in out:
        best = np.maximum.accumulate(res.values)
        assert res.bound == best[-1]
        prev = -np.inf
        for n in (0, 5, 20, 100):
            r = lp.dual_ascent_host(b, mask, n, lr=0.1)
            assert r.bound == best[n] and r.bound >= prev, (name, n)      # the prefix of one run is the shorter run
            prev = r.bound
        closed = (res.bound - res.values[0]) / (opt - res.values[0])
        assert closed >= 0.999, (name, closed)
        assert float(lp.dual_value(b, mask, res.alpha, res.beta)) == res.bound


def test_supergradient_is_autograd_of_dual_value(solved):
    """At the default start and at a random point with every split multiplier active, on every domain."""
    lp, out = solved
    g = torch.Generator().manual_seed(5)
    for name, mask, b, _, _ in out:
        R = sum(len(m) for m in mask)
        for al, be in ((None, None), (torch.rand(R, generator=g, dtype=torch.float64), torch.rand(R, generator=g, dtype=torch.float64))):
            al, be = lp.dual_start(b, mask, al, be)
            res = lp.dual_ascent_host(b, mask, 0, alpha=al, beta=be)
            al, be = al.clone().requires_grad_(), be.clone().requires_grad_()
            lp.dual_value(b, mask, al, be).backward()
            for got, want in ((res.grad_alpha, al.grad), (res.grad_beta, be.grad)):
                assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
            assert float(res.grad_alpha.abs().max()) > 0
            assert (float(res.grad_beta.abs().max()) > 0) == (name != "root")
            split = torch.cat(mask) != -1
            assert not bool(res.grad_beta[~split].any()) and int(split.sum()) == (name != "root")


def test_recovered_point_is_a_point_of_the_relaxation(solved):
    """dual_recover: x_lp in the box, each pre-activation the affine image of the post-activation below, every post value inside its
    triangle, duals signed as _solve_lp's and zero on decided nodes."""
    lp, out = solved
    for name, mask, b, opt, res in out:
        rec = lp.dual_recover(b, mask, res.alpha, res.beta)
        assert rec["g"] == res.bound
        x = rec["x_lp"]
        assert bool((x >= lp.input_lb).all()) and bool((x <= lp.input_ub).all())
        q = x
        r = 0
        for i, l in enumerate(lp.layers):
            if type(l) is torch.nn.ReLU:
                lo, up = b[0][i].reshape(-1), b[1][i].reshape(-1)
                p, v, d, m = rec["pre"][r], rec["post"][r], rec["dual"][r], mask[r]
                assert torch.equal(p, q.reshape(-1))
                amb = (m == -1) & (lo < 0) & (up > 0)
                s = up / (up - lo)
                assert bool((v[amb] >= torch.clamp(p[amb], min=0) - 1e-6).all()) and bool((v[amb] <= (s * (p - lo))[amb] + 1e-6).all()), name
                assert not bool(d[~amb].any()) and not bool(d[:, 0].any())
                assert bool((d[:, 1] >= 0).all()) and bool((d[:, 2] <= 0).all()) and not bool(((d[:, 1] != 0) & (d[:, 2] != 0)).any())
                q = v.reshape(q.shape)
                r += 1
            elif type(l) in (torch.nn.Conv2d, torch.nn.Linear):
                q = lp._affine(l, q)
            else:
                q = q.reshape(-1)
        assert float(q.reshape(-1)[0]) == rec["out"]


def test_new_symbols_are_declared_bound_and_exported():
    _lib.build_library()
    lib = _lib.load()
    names = {s[0] for s in _lib.SYMBOLS}
    for n in ("gnnb_dual_workspace_bytes", "gnnb_dual_ascent"):
        assert n in names and hasattr(lib, n), n
    assert "gnnb_k_dual.h" in _lib.SOURCES
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    assert "k_dual_ascent" in classes


def test_null_handle_is_refused():
    _lib.build_library()
    lib = _lib.load()
    assert lib.gnnb_dual_workspace_bytes(None, 4) == 0
    db = _lib.DualBatch()
    assert lib.gnnb_dual_ascent(None, C.byref(db), 4, 5, 0.1, None, None, 0, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.gnnb_last_error()


def test_solve_many_and_the_threshold_loop_know_the_mode():
    lp, doms = toy_kw_domains()
    with pytest.raises(ValueError):
        lp.solve_many([], lp="simplex")
    with pytest.raises(ValueError):
        lp_producer.branch_and_bound_threshold(lp, None, None, lp.layers, child_lp="simplex")
    assert lp.solve_many([]) == [] and lp.engine is None
