"""LayerGraphLP.kw_bounds(tighten=n) on the host: intermediate bounds tightened by per-node slope-optimised dual
ascent, on the cases of tests/golden/exact_minima.npz -- tighten=0 is today's code path and bits, tighten=20 is never looser, contains the
stored exact node extrema and sampled points, decides nodes the plain bounds leave ambiguous, and raises the LP optimum and the ascent's
bound of the root.  Also the C-ABI of gnnb_kw_tighten as far as it can be checked without a device."""
import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib
from tests import exact_minimum as E
from tests.common import register_kw_archs
from tests.test_gpu_kw_geometry import Domain, Net, force_nodes

FIX = E.load()
CASES = list(FIX)
_shared = {}


def root(case):
    """(lp, mask, plain bounds, tightened bounds at 20 iterations, report) of the case's root, computed once."""
    if case not in _shared:
        lp = E.case_lp(case, FIX[case])
        mask, report = E.root_mask(lp), {}
        _shared[case] = (lp, mask, lp.kw_bounds(mask), lp.kw_bounds(mask, tighten=20, report=report), report)
    return _shared[case]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))


@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_gap", "kwg_s1", "kwg_deep8"])
def test_tighten_zero_is_the_plain_code_path(name):
    """Roots, a domain with forced nodes and a child with a parent: torch.equal, and nothing of the tightening runs."""
    register_kw_archs()
    net = Net(name)
    doms = [Domain(net, 11 + 97 * i, 0.003, i % 10, (i + 3) % 10) for i in range(3)]
    force_nodes(doms[1], np.random.RandomState(3), 2)
    d = doms[2]
    d.parent, d.split = d.lp.kw_bounds(d.mask), len(d.mask) - 2
    i = d.lp.pre_relu_indices[d.split]
    amb = torch.nonzero((d.parent[0][i].reshape(-1) < 0) & (d.parent[1][i].reshape(-1) > 0)).reshape(-1)
    assert len(amb)
    d.mask[d.split][int(amb[0])] = 1
    for d in doms:
        def never(*a, **k):
            raise AssertionError("tighten=0 reached the tightening")
        d.lp._tighten_layer = never
        report = {}
        assert same(d.lp.kw_bounds(d.mask, d.parent, d.split), d.lp.kw_bounds(d.mask, d.parent, d.split, tighten=0, report=report))
        assert report == {"counts": [0, 0], "objectives": []}


def test_bad_arguments_are_refused():
    lp, mask = root(CASES[0])[:2]
    for kw in ({"tighten": -1}, {"tighten": 3, "lr": 0.0}, {"tighten": 3, "lr": float("inf")}, {"tighten": 3, "lr": float("nan")}):
        with pytest.raises(ValueError):
            lp.kw_bounds(mask, **kw)


@pytest.mark.parametrize("case", CASES)
def test_never_looser_and_contains_the_extrema_and_sampled_points(case):
    lp, mask, plain, tight, _ = root(case)
    for side, better in ((0, torch.ge), (1, torch.le)):
        for i, (t, p) in enumerate(zip(tight[side], plain[side])):
            assert bool(better(t, p).all()), (case, side, i)
    e = FIX[case]
    i = lp.pre_relu_indices[int(e["node_layer"])]
    for node, (lo0, lo1, hi0, hi1) in zip(e["nodes"], e["node_extrema"]):
        lo, up = float(tight[0][i].reshape(-1)[node]), float(tight[1][i].reshape(-1)[node])
        assert lo <= lo1 + E.slack(lo1) and up >= hi0 - E.slack(hi0), (case, int(node), lo, up, lo1, hi0)
    g = torch.Generator().manual_seed(5)
    for _ in range(256):
        x = lp.input_lb + (lp.input_ub - lp.input_lb) * torch.rand(lp.input_lb.shape, generator=g, dtype=torch.float64)
        pre, out = E.pre_activations(lp, x)
        for r, p in zip(lp.pre_relu_indices, pre):
            assert bool((p >= tight[0][r].reshape(-1) - 1e-12).all()) and bool((p <= tight[1][r].reshape(-1) + 1e-12).all()), (case, r)
        assert float(tight[0][-1]) - 1e-12 <= out <= float(tight[1][-1]) + 1e-12


@pytest.mark.parametrize("case, least", [("kwg_mlp@0.02:8:3", 1), ("kwg_mlp@0.02:2:6", 1), ("kwg_gap@0.01:3:5", 1), ("kwg_gap@0.01:0:8", 1)])
def test_nodes_leave_the_ambiguous_set(case, least):
    lp, mask, plain, tight, report = root(case)
    ran, decided = report["counts"]
    assert ran >= decided >= least, (case, report["counts"])
    amb = [int((((lo < 0) & (up > 0)).sum())) for b in (plain, tight) for lo, up in [(torch.cat([b[0][i].reshape(-1) for i in lp.pre_relu_indices]),
                                                                                      torch.cat([b[1][i].reshape(-1) for i in lp.pre_relu_indices]))]]
    assert amb[0] - amb[1] >= decided, (case, amb)          # (at least: a decided node may decide others above it)
    assert len(report["objectives"]) == 2 * ran


@pytest.mark.parametrize("case", [c for c in CASES if FIX[c]["network"] == "kwg_single"])
def test_one_relu_layer_has_nothing_to_tighten(case):
    lp, mask, plain, tight, report = root(case)
    assert same(plain, tight) and report["counts"] == [0, 0]


@pytest.mark.parametrize("case", CASES)
def test_the_lp_optimum_and_the_ascent_bound_do_not_fall(case):
    """The LP's feasible set shrinks with the bounds; the 20-iteration ascent is a heuristic on it, held to the fixture's slack."""
    lp, mask, plain, tight, _ = root(case)
    a = lp._solve_lp([m.clone() for m in mask], *plain)
    b = lp._solve_lp([m.clone() for m in mask], *tight)
    assert b.lb >= a.lb - 1e-9, (case, a.lb, b.lb)
    da, db = lp.dual_ascent_host(plain, mask, 20).bound, lp.dual_ascent_host(tight, mask, 20).bound
    assert db >= da - E.slack(da), (case, da, db)
    m_up = float(FIX[case]["m_up"][0])
    assert b.lb <= m_up + E.slack(m_up) and db <= m_up + E.slack(m_up), (case, b.lb, db, m_up)


def test_the_first_evaluation_is_the_kw_bound():
    """One node of kwg_gap's Linear layer and one of its 1x1 conv: iteration 0 of both signs is _kw_layer's pair."""
    lp, mask, plain, _, _ = root("kwg_gap@0.01:3:5")
    for r in (1, 2):
        q = lp.pre_relu_indices[r] - 1
        while type(lp.layers[q]).__name__ not in ("Conv2d", "Linear"):
            q -= 1
        lbs, ubs = plain[0][:q + 1], plain[1][:q + 1]
        kl, ku = lp._kw_layer(q, lbs + [None], ubs + [None])
        j = int(torch.nonzero(((plain[0][q + 1] < 0) & (plain[1][q + 1] > 0)).reshape(-1))[0])
        only = [m.clone() for m in mask]
        only[r] = torch.where(torch.arange(only[r].numel()) == j, -1, 1)     # every other node of the layer is split: the ascent runs for j alone
        objectives = []
        nl, nu, ran, _ = lp._tighten_layer(q, r, lbs, ubs, torch.full_like(kl, -1e9), torch.full_like(ku, 1e9), only, 0, 0.1, objectives)
        assert ran == 1 and [o[:3] for o in objectives] == [(q + 1, j, 1.0), (q + 1, j, -1.0)]
        assert abs(float(nl.reshape(-1)[j]) - float(kl.reshape(-1)[j])) <= 1e-12 and abs(float(nu.reshape(-1)[j]) - float(ku.reshape(-1)[j])) <= 1e-12


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------------
NEW = ("gnnb_kw_tighten_workspace_bytes", "gnnb_kw_tighten")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_the_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert "gnnb_k_tighten.h" in _lib.SOURCES
    assert lib.gnnb_abi_version() == 2 and "GNNB_ABI_VERSION 2" in header.replace("  ", " ")
    from gnn_branching_amd.engine import ScorerEngine
    import inspect
    assert {"tighten", "lr"} <= set(inspect.signature(ScorerEngine.kw_bounds).parameters)


def test_a_null_handle_is_refused_before_anything_else(lib):
    assert lib.gnnb_kw_tighten_workspace_bytes(None, 4) == 0
    for n_iter, lr in ((5, 0.1), (-1, 0.1), (5, 0.0), (5, float("nan"))):
        assert lib.gnnb_kw_tighten(None, None, 1, n_iter, lr, None, None, None, None, None, None, None, 0, None, 0, None) == -1
        msg = lib.gnnb_last_error()
        assert b"gnnb_kw_tighten:" in msg and b"null handle" in msg, msg
