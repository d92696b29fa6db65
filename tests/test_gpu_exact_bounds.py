"""The bounding kernels on the MI355X against certified exact minima (tests/golden/exact_minima.npz; tests/exact_minimum.py states how
they were computed -- a MILP on the CPU, solved once; nothing is solved here).  Per network ONE gnnb_kw_bounds call and ONE
gnnb_dual_ascent call per setting over all stored domains of its cases, every domain with its own box, property and mask, the children
with their parent's device bounds and split layer:

1. bounds: the dual value is at most the exact minimum at n_iter 0, 5 and 25 and from a random warm start, and so is its fp32 copy;
2. containment: the fp64 and fp32 intermediate bounds contain the network at the exact minimiser, and the stored per-node extrema;
3. the infeasible flag is 1 on the stored infeasible domain and 0 on every domain whose MILP is feasible;
4. the upper side: gnnb_net_eval at the minimiser is the minimum, and no descent returns a value below it or a point outside the box;
5. strong branching: no row of the root's table claims more improvement than the exact minima of the children allow."""
import numpy as np
import pytest
import torch

from gnn_branching_amd import lp_producer
from gnn_branching_amd.frontier import branch_and_bound_frontier
from tests import exact_minimum as E
from tests.frontier_twin import CKPT
from tests.test_gpu_kw_geometry import Net

pytestmark = pytest.mark.gpu

FIX = E.load()
NETWORKS = sorted({e["network"] for e in FIX.values()})
ND = len(E.DOMAINS)
_shared = {}


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    from tests.common import register_kw_archs
    register_kw_archs()
    return ScorerEngine(None)


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


class Rows:
    """The stored domains of every case of one network as batch rows: row = case index * ND + domain index."""

    def __init__(self, name):
        self.net = Net(name)
        self.cases = [c for c, e in FIX.items() if e["network"] == name]
        self.lps = [E.case_lp(c, FIX[c]) for c in self.cases]
        self.entry = [FIX[c] for c in self.cases for _ in range(ND)]
        self.dom = [k for _ in self.cases for k in range(ND)]
        self.lp = [lp for lp in self.lps for _ in range(ND)]
        self.B = len(self.entry)
        self.props = [self.net.prop(*(int(v) for v in e["prop"])) for e in self.entry]
        self.x_lo = torch.stack([lp.input_lb for lp in self.lp])
        self.x_hi = torch.stack([lp.input_ub for lp in self.lp])
        self.masks = torch.from_numpy(np.stack([e["masks"][k] for e, k in zip(self.entry, self.dom)]))
        self.parent = [(-1 if int(e["parent"][k]) < 0 else (b - k) + int(e["parent"][k])) for b, (e, k) in enumerate(zip(self.entry, self.dom))]
        self.split = torch.tensor([int(e["split"][k]) for e, k in zip(self.entry, self.dom)], dtype=torch.int32)
        self.feasible = [int(e["status"][k]) == 0 for e, k in zip(self.entry, self.dom)]
        self.m_lo = [float(e["m_lo"][k]) for e, k in zip(self.entry, self.dom)]
        self.m_up = [float(e["m_up"][k]) for e, k in zip(self.entry, self.dom)]
        self.root_lo = [float(e["m_lo"][0]) for e in self.entry]
        # x_star in fp32 (every corner of the box is an fp32 value, so rounding to nearest stays inside); the infeasible rows get the centre
        xs = torch.stack([torch.from_numpy(e["x_star"][k]).reshape(lp.shapes[0]) if f else 0.5 * (lp.input_lb + lp.input_ub)
                          for e, k, lp, f in zip(self.entry, self.dom, self.lp, self.feasible)])
        self.x_star64, self.x_star32 = xs, xs.float()
        assert bool((self.x_star32.double() >= self.x_lo).all()) and bool((self.x_star32.double() <= self.x_hi).all())

    def what(self, b):
        return self.cases[b // ND], E.DOMAINS[self.dom[b]]


def rows_of(name):
    if ("rows", name) not in _shared:
        _shared[("rows", name)] = Rows(name)
    return _shared[("rows", name)]


def device_bounds(engine, name):
    """The intermediate bounds of every row: the parentless rows first (their own call would do; the whole batch is bounded twice so
    that the second call is the ONE call over all stored domains), then all rows, the children with their parent row's bounds."""
    if ("kw", name) not in _shared:
        R = rows_of(name)
        first = engine.kw_bounds(R.net.fixed, R.props, R.x_lo, R.x_hi, R.masks)
        src = torch.tensor([p if p >= 0 else b for b, p in enumerate(R.parent)], device=engine.device)
        parents = tuple([t[src].contiguous() for t in side] for side in (first.lb, first.ub))
        split = torch.where(torch.tensor(R.parent) >= 0, R.split, torch.full_like(R.split, -1))
        res = engine.kw_bounds(R.net.fixed, R.props, R.x_lo, R.x_hi, R.masks, parents, split, want_fp32=True)
        _shared[("kw", name)] = res
    return _shared[("kw", name)]


def ascent(engine, name, n_iter, alpha=None, beta=None, **kw):
    R, res = rows_of(name), device_bounds(engine, name)
    return engine.dual_ascent(R.net.fixed, R.props, R.x_lo, R.x_hi, R.masks, res.lb, res.ub, n_iter, 0.1, alpha, beta, **kw)


# ---- 3. the infeasible flag (first: everything below reads the feasible rows) ---------------------------------------------------------
@pytest.mark.parametrize("name", NETWORKS)
def test_infeasible_flag_is_the_milp_verdict(name, engine):
    """A flagged feasible domain would be a minimum thrown away."""
    R, res = rows_of(name), device_bounds(engine, name)
    flags = res.infeasible.cpu().tolist()
    for b, flag in enumerate(flags):
        assert flag == (0 if R.feasible[b] else 1), (R.what(b), flag)


# ---- 1. bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETWORKS)
def test_dual_bounds_never_exceed_the_exact_minimum(name, engine):
    R = rows_of(name)
    dev = engine.device
    g = torch.Generator().manual_seed(3)
    runs = [("n_iter 0", 0, None, None), ("n_iter 5", 5, None, None), ("n_iter 25", 25, None, None)]
    RR = R.masks.shape[1]
    alpha = torch.rand(R.B, RR, generator=g, dtype=torch.float64)
    beta = 2.0 * torch.rand(R.B, RR, generator=g, dtype=torch.float64)
    runs.append(("warm start, n_iter 5", 5, alpha, beta))
    for what, n_iter, al, be in runs:
        lb32 = torch.zeros(R.B, dtype=torch.float32, device=dev)
        da = ascent(engine, name, n_iter, al, be, lb32_prop=lb32)
        bound, b32 = da.bound.cpu().tolist(), lb32.cpu().tolist()
        worst = None
        for b in range(R.B):
            if not R.feasible[b]:
                continue
            sl = E.slack(R.m_up[b])
            gap = R.m_up[b] - bound[b]
            worst = gap if worst is None else min(worst, gap)
            assert bound[b] <= R.m_up[b] + sl, (R.what(b), what, bound[b], R.m_up[b])
            assert b32[b] <= R.m_up[b] + sl + ulp32(b32[b]), (R.what(b), what, b32[b], R.m_up[b])
            assert abs(b32[b] - bound[b]) <= ulp32(bound[b]), (R.what(b), what)
        print(f"{name} {what}: smallest exact minimum - bound = {worst:.3e}")


# ---- 2. containment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETWORKS)
def test_intermediate_bounds_contain_the_minimiser_and_the_node_extrema(name, engine):
    """At x_star (fp64, as stored) the pre-activations lie inside the device's bounds of the domain x_star minimises over: the fp64
    ones within the solver's feasibility tolerance of a split's sign constraint (1e-6 max(1, |p|)), the fp32 copies within that plus
    one fp32 ulp of the bound (they are the fp64 bounds rounded to nearest).  The stored exact extrema lie inside the root's bounds."""
    R, res = rows_of(name), device_bounds(engine, name)
    lb, ub = [t.cpu() for t in res.lb], [t.cpu() for t in res.ub]
    lb32, ub32 = [t.cpu().reshape(R.B, -1) for t in res.lb32], [t.cpu().reshape(R.B, -1) for t in res.ub32]
    for b in range(R.B):
        if not R.feasible[b]:
            continue
        pre, out = E.pre_activations(R.lp[b], R.x_star64[b])
        for k, p in enumerate(pre + [torch.tensor([out], dtype=torch.float64)]):
            tol = 1e-6 * torch.maximum(torch.ones_like(p), p.abs())
            assert bool((p >= lb[k][b] - tol).all()) and bool((p <= ub[k][b] + tol).all()), (R.what(b), k)
            lo32, up32 = lb32[k + 1][b].double(), ub32[k + 1][b].double()
            u_lo = torch.from_numpy(np.spacing(lo32.abs().float().numpy())).double()
            u_up = torch.from_numpy(np.spacing(up32.abs().float().numpy())).double()
            assert bool((p >= lo32 - tol - u_lo).all()) and bool((p <= up32 + tol + u_up).all()), (R.what(b), k, "fp32")
        x = R.x_star64[b].reshape(-1)
        assert bool((x >= lb32[0][b].double()).all()) and bool((x <= ub32[0][b].double()).all()), (R.what(b), "box")
    for c, case in enumerate(R.cases):
        e, b = FIX[case], c * ND
        k = int(e["node_layer"])
        for node, (lo0, lo1, hi0, hi1) in zip(e["nodes"], e["node_extrema"]):
            lo, up = float(lb[k][b][node]), float(ub[k][b][node])
            assert lo <= lo1 + E.slack(lo1) and up >= hi0 - E.slack(hi0), (case, int(node), lo, up, lo1, hi0)
            assert lo <= hi0 and up >= lo1


# ---- 4. the upper side ----------------------------------------------------------------------------------------------------------------
def fp64_values(R, x32):
    return [float(E.net_value(R.lp[b], x32[b].double())[0]) for b in range(R.B)]


@pytest.mark.parametrize("name", NETWORKS)
def test_net_eval_at_the_minimiser_is_the_minimum(name, engine):
    """gnnb_net_eval at x_star rounded to fp32: the fp64 network at that fp32 point by the device-against-host rule 1e-9 max(1, |v|), and
    within the rounding of the point of m_up -- both x_star and its fp32 image lie in the box [min, max] of the two, whose interval
    image's width bounds the difference of the two values."""
    R = rows_of(name)
    got = engine.net_eval(R.net.fixed, R.props, R.x_star32.to(engine.device)).cpu().tolist()
    want = fp64_values(R, R.x_star32)
    for b in range(R.B):
        if not R.feasible[b]:
            continue
        assert abs(got[b] - want[b]) <= 1e-9 * max(1.0, abs(want[b])), (R.what(b), got[b], want[b])
        a, c = R.x_star64[b], R.x_star32[b].double()
        tiny = lp_producer.LayerGraphLP(R.lp[b].layers, torch.minimum(a, c), torch.maximum(a, c))
        il, iu = tiny.interval_bounds(E.root_mask(tiny))
        width = float(iu[-1].reshape(-1)[0] - il[-1].reshape(-1)[0])
        assert abs(got[b] - R.m_up[b]) <= width + 1e-9 * max(1.0, abs(R.m_up[b])), (R.what(b), got[b], R.m_up[b], width)
        assert got[b] >= R.root_lo[b] - E.slack(R.root_lo[b]), (R.what(b), got[b], R.root_lo[b])


@pytest.mark.parametrize("name", NETWORKS)
def test_no_descent_returns_less_than_the_minimum_or_leaves_the_box(name, engine):
    """gnnb_net_descend from the LP point of a 5-step ascent and gnnb_net_descend_starts from that point and three random restarts: every
    returned value is the fp64 network at the returned point, the point lies in the row's box, and the value is no lower than the exact
    minimum over the box."""
    R = rows_of(name)
    dev = engine.device
    da = ascent(engine, name, 5, want_scorer_inputs=True)
    x_lo, x_hi = R.x_lo.reshape(R.B, -1).to(dev), R.x_hi.reshape(R.B, -1).to(dev)
    one = engine.net_descend(R.net.fixed, R.props, da.x_lp, x_lo, x_hi, 4)
    starts = engine.net_starts(R.net.fixed, da.x_lp, x_lo, x_hi, 3, seed=11)
    many = engine.net_descend_starts(R.net.fixed, R.props, starts, x_lo, x_hi, 4)
    lp_values = engine.net_eval(R.net.fixed, R.props, da.x_lp).cpu().tolist()
    for what, (x_best, value) in (("descend", one[:2]), ("descend_starts", many[:2])):
        x_best, value = x_best.cpu().reshape(R.x_star32.shape), value.cpu().tolist()
        want = fp64_values(R, x_best)
        for b in range(R.B):
            if not R.feasible[b]:
                continue
            assert abs(value[b] - want[b]) <= 1e-9 * max(1.0, abs(want[b])), (R.what(b), what, value[b], want[b])
            assert bool((x_best[b].double() >= R.x_lo[b]).all()) and bool((x_best[b].double() <= R.x_hi[b]).all()), (R.what(b), what)
            assert value[b] >= R.root_lo[b] - E.slack(R.root_lo[b]), (R.what(b), what, value[b], R.root_lo[b])
            assert value[b] <= lp_values[b], (R.what(b), what, value[b], lp_values[b])      # slot 0 is the LP point: never worse than it


# ---- 5. strong branching ---------------------------------------------------------------------------------------------------------------
def choice_of(lp):
    from gnn_branching_amd import bab_caller
    key = ("choice", tuple(int(m.numel()) for m in E.root_mask(lp)))
    if key not in _shared:
        c = bab_caller.BatchedGraphChoice(E.root_mask(lp), CKPT)
        c.verbose = False
        _shared[key] = c
    return _shared[key]


# the cases whose root has a negative bound (the improvement is defined against it) and does not close its own gap: global_ub is at least
# m_up and the device's root bound is the host twin's root20 to 1e-9, so with m_up - root20 below eps no round ever runs (kwg_deep8)
STRONG_CASES = [c for c, e in FIX.items() if float(e["root20"]) < 0 and float(e["m_up"][0] - e["root20"]) > 2e-4]


@pytest.mark.parametrize("case", STRONG_CASES)
def test_strong_table_of_the_root_against_the_children_s_exact_minima(case):
    """One audited round from the root, every undecided node a candidate.  With the root's bound P < 0 a candidate's improvement is
    (min(a, 0) + min(b, 0) - 2 P) / (-2 P) of its children's bounds a and b, so the audit dict gives min(a, 0) + min(b, 0) = 2 P (1 - imp):
    the table is read through that sum, the two bounds of a candidate are not in the audit separately.  The minimum m lies in one of the
    two children, so min(a, 0) + min(b, 0) <= min(min(a, b), 0) <= min(m, 0) for every candidate.  For the two stored splits, whose
    children's own minima m_a, m_b are known, the sharper min(m_a, 0) + min(m_b, 0) holds.  The committed decision's children are read
    through the trace and obey the same.

    Coverage: the five cases of STRONG_CASES -- the four with a negative minimum whose root leaves a gap, and kwg_mlp@0.01:8:6 (minimum
    0.017, root bound -0.0006), where min(m, 0) = 0 and the claim is only that no candidate improves by more than 1.  The two kwg_deep8
    cases have no table (their root closes the gap), the other positive cases no negative root bound."""
    assert len(STRONG_CASES) == 5
    e = FIX[case]
    lp = E.case_lp(case, e)
    audit, trace = [], []
    res = branch_and_bound_frontier(lp, choice_of(lp), lp.layers, K=1, n_iter=20, lr=0.1, eps=1e-4, max_rounds=1, log=lambda s: None, trace=trace,
                                    branching="babsr", strong_audit=audit)
    sl = E.slack(e["m_up"][0])
    m = min(float(e["m_up"][0]), 0.0)
    assert res[2] == 1, res
    assert len(audit) == 1 and len(trace) == 1
    row, t = audit[0], trace[0]
    P = t["parent_bounds"][0]
    assert P <= float(e["m_up"][0]) + sl and P < 0
    root = E.flat_mask(E.root_mask(lp))
    stored = {}
    for a, b in ((2, 3), (4, 5)):
        flat = int(np.nonzero(e["masks"][a] != root)[0][0])
        stored[int(flat)] = min(float(e["m_up"][a]), 0.0) + min(float(e["m_up"][b]), 0.0)
    seen = 0
    for cand, imp in zip(row["candidates"], row["improvements"]):
        if imp != imp:                                        # a dead pair: no claim
            continue
        total = 2 * P * (1 - imp)
        assert total <= m + 2 * sl, (case, cand, imp, total, m)
        if cand in stored:
            seen += 1
            assert total <= stored[cand] + 2 * sl, (case, cand, imp, total, stored[cand])
    assert seen == 2, (case, sorted(stored), len(row["candidates"]))
    live = [c for c in (0, 1) if t["live"][c] and not t["infeasible"][c]]
    assert live and min(t["child_bounds"][c] for c in live) <= float(e["m_up"][0]) + sl
    assert res[1] >= float(e["m_lo"][0]) - sl
