"""The witness of the upper bound on the MI355X:

1. gnnb_frontier_witness against a Python restatement of its rule, exact, on synthetic rows that take every branch;
2. gnnb_frontier_witness_jobs per entry against gnnb_frontier_witness on the entry's rows;
3. ``branch_and_bound_frontier(witness=..., pgd_steps=...)`` on toy_kw: the device's incumbent against the state record every round, the
   point against the network, the options off against the launches of a round as they were, soundness;
4. ``verify_properties`` / ``verify_properties_threshold``: every job's witness and result against its run alone."""
import math

import numpy as np
import pytest
import torch

from gnn_branching_amd.frontier import FrontierJob, FrontierJobs, RoundPlan, branch_and_bound_frontier, verify_properties, verify_properties_threshold
from tests.frontier_twin import EPS_BAB, LR, N_ITER, bind, engine, toy  # noqa: F401  (engine: the module fixture)
from tests.test_gpu_frontier import torch_fp64

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
NEW_CLASSES = ("k_net_descend", "k_frontier_witness", "k_frontier_witness_jobs")


# ---- 1. the kernel against its rule ---------------------------------------------------------------------------------------------------
class Rows:
    """2K child rows on the bound network: only live, infeasible and ubv are read, the rest has to exist."""

    def __init__(self, eng, K, live, infeasible, ubv):
        dev, R, n = eng.device, eng.R, 2 * K
        f64 = torch.float64
        self.mask = torch.zeros(n, R, dtype=torch.int8, device=dev)
        self.lb = [torch.zeros(n, s, dtype=f64, device=dev) for s in eng.sizes[1:]]
        self.ub = [torch.zeros(n, s, dtype=f64, device=dev) for s in eng.sizes[1:]]
        self.alpha, self.beta = torch.zeros(n, R, dtype=f64, device=dev), torch.zeros(n, R, dtype=f64, device=dev)
        self.bound = torch.zeros(n, dtype=f64, device=dev)
        self.live = torch.tensor(live, dtype=torch.int32).to(dev)
        self.infeasible = torch.tensor(infeasible, dtype=torch.int32).to(dev)
        self.ubv = torch.tensor(ubv, dtype=f64).to(dev)

    def view(self, a, b):
        """The child rows [a, b) as a set of their own."""
        out = object.__new__(Rows)
        for k, v in vars(self).items():
            setattr(out, k, [t[a:b] for t in v] if isinstance(v, list) else v[a:b])
        return out


def restate(live, infeasible, ubv, x_a, x_b, used, sel_rows, best_value, best_point):
    """The rule in Python: (value, point) after the step."""
    c, v = -1, INF
    for i in range(len(ubv)):
        if live[i] and not infeasible[i] and ubv[i] < v:            # strict: the first of equal values, never a NaN
            c, v = i, ubv[i]
    if c < 0 or not v < best_value:
        return best_value, best_point
    if used is not None and used[c >> 1]:
        return v, x_b[2 * sel_rows.index(c >> 1) + (c & 1)]
    return v, x_a[c]


def scenarios(K, rng):
    """(name, live, infeasible, ubv, used, sel_rows, incumbent) over 2K rows."""
    n = 2 * K
    base = rng.uniform(1.0, 2.0, n)
    lo, hi = 0, n - 1
    out = []
    v = base.copy(); v[lo] = v[hi] = 0.25                             # noqa: E702
    out.append(("two children of equal value: the lower index wins", [1] * n, [0] * n, v, None, [], INF))
    if K == 130:
        v = base.copy(); v[3] = v[259] = v[200] = 0.25                # noqa: E702  (3 and 259: one thread's two rows)
        out.append(("equal values of one thread and another", [1] * n, [0] * n, v, None, [], INF))
    v = base.copy(); v[hi] = 0.5                                      # noqa: E702
    out.append(("a value equal to the incumbent: the incumbent stays", [1] * n, [0] * n, v, None, [], 0.5))
    out.append(("a value below the incumbent", [1] * n, [0] * n, v, None, [], 0.75))
    if K >= 3:
        live, inf, v = [1] * n, [0] * n, base.copy()
        live[0], v[0] = 0, -5.0
        inf[1], v[1] = 1, -4.0
        v[2] = NAN
        v[n - 2] = 0.125
        out.append(("dead, infeasible and NaN rows do not win", live, inf, v, None, [], INF))
    out.append(("nothing live: nothing wins", [0] * n, [0] * n, base - 3.0, None, [], INF))
    out.append(("everything NaN: nothing wins", [1] * n, [0] * n, np.full(n, NAN), None, [], INF))
    for odd in (0, 1):                                                 # the winner is pair B's, through used_kw / sel_rows
        parent = K - 1
        sel = [parent] if K == 1 else [0, parent] if K == 3 else [5, 0, parent, 64]
        used = [0] * K
        used[parent] = 1
        if K > 1:
            used[0] = 0                                                # selected, but it kept its GNN pair
        v = base.copy(); v[2 * parent + odd] = 0.0625                  # noqa: E702
        out.append((f"a winner from pair B, child {odd}", [1] * n, [0] * n, v, used, sel, INF))
    used = [1] + [0] * (K - 1)
    v = base.copy(); v[n - 1] = 0.03125                                # noqa: E702
    out.append(("pair B in the round, the winner pair A's", [1] * n, [0] * n, v, used if K > 1 else None, [0] if K > 1 else [], INF))
    return out


@pytest.mark.parametrize("K", [1, 3, 130])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_witness_kernel_against_its_rule(name, K, engine):
    bind(engine, name)
    dev, N0 = engine.device, engine.sizes[0]
    rng = np.random.RandomState(5 + K)
    x_a = torch.from_numpy(rng.standard_normal((2 * K, N0)).astype(np.float32))
    x_b = torch.from_numpy(rng.standard_normal((2 * K, N0)).astype(np.float32)) + 100.0
    poison = torch.full((N0,), -777.0, dtype=torch.float32)
    for what, live, inf, ubv, used, sel, incumbent in scenarios(K, rng):
        rows = Rows(engine, K, live, inf, ubv)
        best_value = torch.tensor([incumbent], dtype=torch.float64).to(dev)
        best_point = poison.clone().to(dev)
        m = len(sel)
        pair_b = {} if used is None else {"x_b": x_b[:2 * m].to(dev), "used_kw": torch.tensor(used, dtype=torch.int32).to(dev),
                                          "sel_rows": torch.tensor(sel, dtype=torch.int32).to(dev), "m": m}
        engine.frontier_witness(K, rows, x_a.to(dev), best_value, best_point, **pair_b)          # m = 0 with x_b NULL when there is no pair B
        want_v, want_p = restate(live, inf, list(ubv), x_a, x_b, used, sel, incumbent, poison)
        got_v, got_p = float(best_value.cpu()[0]), best_point.cpu()
        assert got_v == want_v or (math.isnan(got_v) and math.isnan(want_v)), (name, K, what, got_v, want_v)
        assert torch.equal(got_p, want_p), (name, K, what)
        if "nothing wins" in what or "incumbent stays" in what:
            assert torch.equal(got_p, poison) and got_v == incumbent, (name, K, what)
        else:
            assert not torch.equal(got_p, poison), (name, K, what)


def test_witness_limits_with_a_handle(engine):
    bind(engine, "kwg_mlp")
    dev, N0 = engine.device, engine.sizes[0]
    rows = Rows(engine, 2, [1] * 4, [0] * 4, [1.0] * 4)
    bv, bp, x = torch.full((1,), INF, dtype=torch.float64, device=dev), torch.zeros(N0, device=dev), torch.zeros(8, N0, device=dev)
    used, sel = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="gnnb_frontier_witness.*m = 3"):
        engine.frontier_witness(2, rows, x, bv, bp, x_b=x, used_kw=used, sel_rows=sel, m=3)
    with pytest.raises(RuntimeError, match="gnnb_frontier_witness.*needs x_b"):
        engine.frontier_witness(2, rows, x, bv, bp, used_kw=used, m=1)
    with pytest.raises(ValueError):
        engine.frontier_witness(2, rows, x[:3], bv, bp)                 # fewer than 2K points


# ---- 2. the jobs form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_b", [False, True])
def test_witness_jobs_per_entry_equals_the_single_job_kernel(pair_b, engine):
    """Three entries in segments (3, 0, 2) of 5, k = (2, 1, 3): each segment's value and point are the single-job kernel's on the entry's
    rows, bit for bit; segments 1 and 4 have no entry and keep their poison.  With pair B, entries 0 and 2 win through used_kw / sel_rows."""
    bind(engine, "kwg_rect")
    dev, N0, S = engine.device, engine.sizes[0], 5
    entries, n = [(3, 0, 2), (0, 2, 1), (2, 3, 3)], 6
    rng = np.random.RandomState(17)
    ubv = rng.uniform(0.0, 1.0, 2 * n)
    live, inf = [1] * (2 * n), [0] * (2 * n)
    live[1], inf[7] = 0, 1
    ubv[1], ubv[7], ubv[8] = -1.0, -1.0, NAN
    x_a = torch.from_numpy(rng.standard_normal((2 * n, N0)).astype(np.float32)).to(dev)
    x_b = (torch.from_numpy(rng.standard_normal((2 * n, N0)).astype(np.float32)) + 100.0).to(dev)
    m_e, sel = [1, 0, 2], [1, 3, 5]                                     # global rows, dense, in plan order
    used = [0, 1, 0, 0, 0, 1]
    ubv[2 * 1 + 1], ubv[2 * 5] = -0.5, -0.25                            # the winners of entries 0 and 2 are pair B's (an odd and an even child)
    rows = Rows(engine, n, live, inf, ubv)
    incumbent = [0.1, 7.0, 0.0, INF, 9.0]
    best_value = torch.tensor(incumbent, dtype=torch.float64).to(dev)
    best_point = torch.full((S, N0), -777.0, dtype=torch.float32, device=dev)
    plan = RoundPlan(dev, S, S, 8)
    plan.send(entries)
    kw = {}
    if pair_b:
        kw = {"M": 3, "m_entry": torch.tensor(m_e + [3], dtype=torch.int32).to(dev), "x_b": x_b, "used_kw": torch.tensor(used, dtype=torch.int32).to(dev),
              "sel_rows": torch.tensor(sel, dtype=torch.int32).to(dev)}
    engine.frontier_witness_jobs(plan, rows, x_a, best_value, best_point, **kw)
    got_v, got_p = best_value.cpu(), best_point.cpu()
    sel0 = 0
    for e, (seg, row0, k) in enumerate(entries):
        bv = torch.tensor([incumbent[seg]], dtype=torch.float64).to(dev)
        bp = torch.full((N0,), -777.0, dtype=torch.float32, device=dev)
        one = {}
        if pair_b and m_e[e]:
            one = {"x_b": x_b[2 * sel0:2 * (sel0 + m_e[e])], "used_kw": torch.tensor(used[row0:row0 + k], dtype=torch.int32).to(dev),
                   "sel_rows": torch.tensor([r - row0 for r in sel[sel0:sel0 + m_e[e]]], dtype=torch.int32).to(dev), "m": m_e[e]}
        engine.frontier_witness(k, rows.view(2 * row0, 2 * row0 + 2 * k), x_a[2 * row0:2 * row0 + 2 * k], bv, bp, **one)
        assert float(bv.cpu()[0]) == float(got_v[seg]) and torch.equal(bp.cpu(), got_p[seg]), (e, seg)
        sel0 += m_e[e]
    assert float(got_v[3]) == (-0.5 if pair_b else float(min(ubv[0], ubv[2], ubv[3])))
    if pair_b:
        assert torch.equal(got_p[3], x_b[1].cpu())                       # entry 0, dense entry 0, its odd child
    assert float(got_v[2]) == -0.25 and torch.equal(got_p[2], (x_b[4] if pair_b else x_a[10]).cpu())      # dense entry 2, its even child
    for seg in (1, 4):
        assert float(got_v[seg]) == incumbent[seg] and bool((got_p[seg] == -777.0).all()), seg


# ---- 3. runs on toy_kw -----------------------------------------------------------------------------------------------------------------
_runs = {}


def toy_run(K, rounds, threshold=None, pgd=None, witness=True):
    key = (K, rounds, threshold, pgd, witness)
    if key not in _runs:
        lp, choice, _ = toy()
        trace, point = [], [] if witness else None
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace,
                                        branching_threshold=threshold, witness=point, pgd_steps=pgd)
        _runs[key] = (res, trace, point)
    return _runs[key]


def value64(lp, x):
    return float(torch_fp64(lp.layers, x[None]).reshape(()))


@pytest.mark.parametrize("pgd", [None, 4])
@pytest.mark.parametrize("threshold", [None, 1.0])
@pytest.mark.parametrize("K,rounds", [(1, 4), (4, 5)])
def test_the_witness_is_the_point_of_global_ub(K, rounds, threshold, pgd):
    lp, choice, _ = toy()
    res, trace, point = toy_run(K, rounds, threshold, pgd)
    global_lb, global_ub = res[0], res[1]
    assert len(trace) >= 1 and len(point) == 1 and point[0] is not None
    for r, row in enumerate(trace):                                     # the invariant, every round: the same bits
        assert row["witness_value"] == row["global_ub"], (r, row["witness_value"], row["global_ub"])
    assert trace[-1]["global_ub"] == global_ub
    if threshold is not None:
        print("KW pairs taken per round", [sum(row["used_kw"]) for row in trace])
    x = point[0]
    assert x.dtype == torch.float32 and x.device.type == "cpu" and tuple(x.shape) == tuple(lp.input_lb.shape)
    eng = choice.model.engine()
    on_device = float(eng.net_eval(lp.layers[:-1], [lp.layers[-1]], x[None].to(eng.device)).cpu()[0])
    assert on_device == global_ub, (on_device, global_ub)               # gnnb_net_eval(witness), bit for bit
    f64 = value64(lp, x)
    assert abs(f64 - global_ub) <= 1e-9, (f64, global_ub)
    assert bool((x >= lp.input_lb.float().cpu()).all()) and bool((x <= lp.input_ub.float().cpu()).all())
    # soundness: global_lb below the network everywhere we look
    rng = np.random.RandomState(3)
    lo, hi = lp.input_lb.double().cpu(), lp.input_ub.double().cpu()
    for _ in range(16):
        s = (lo + (hi - lo) * torch.from_numpy(rng.uniform(0, 1, tuple(lo.shape)))).float()
        assert global_lb <= value64(lp, s) + 1e-9
    assert global_lb <= f64 + 1e-9


def test_the_kw_pair_is_taken_in_the_threshold_runs():
    """branching_threshold = 1.0 asks BaBSR for every parent: at least one round of the runs above commits a pair B, so the witness step's
    used_kw / sel_rows path ran on live rows."""
    assert sum(sum(row["used_kw"]) for row in toy_run(4, 5, 1.0, None)[1]) >= 1


@pytest.mark.parametrize("threshold", [None, 1.0])
def test_zero_steps_and_the_witness_change_nothing(threshold):
    """pgd_steps = 0 without a witness: the five-tuple and every key of every round's trace are the plain run's, bit for bit; a witness alone
    changes neither."""
    plain = toy_run(4, 5, threshold, None, witness=False)
    zero = toy_run(4, 5, threshold, 0, witness=False)
    assert zero[0] == plain[0] and zero[1] == plain[1] and len(plain[1]) >= 2
    seen = toy_run(4, 5, threshold, None)
    assert seen[0] == plain[0]
    assert [{k: v for k, v in row.items() if k not in ("witness_value", "global_ub")} for row in seen[1]] == plain[1]
    both = toy_run(4, 5, threshold, 0)
    assert both[0] == plain[0] and torch.equal(both[2][0], seen[2][0])


def test_descent_lowers_the_root_s_upper_bound():
    plain, pgd = toy_run(4, 0, None, None), toy_run(4, 0, None, 4)
    print("root global_ub plain", plain[0][1], "pgd_steps 4", pgd[0][1])
    assert pgd[0][1] <= plain[0][1] and pgd[0][2] == 0
    assert pgd[2][0] is not None and plain[2][0] is not None           # the root goes through the witness step too


def launches(threshold, **options):
    lp, choice, _ = toy()
    eng = choice.model.engine()
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.profile_trace()
        branch_and_bound_frontier(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=lambda s: None,
                                  branching_threshold=threshold, **options)
        eng.profile_read()
        return [name for name, _ in eng.profile_trace(1 << 16)]
    finally:
        eng.profile_enable(False)


@pytest.mark.parametrize("threshold", [None, 1.0])
def test_options_off_launch_none_of_the_new_kernels(threshold):
    off = launches(threshold)
    assert "k_net_eval" in off and not set(off) & set(NEW_CLASSES), set(off) & set(NEW_CLASSES)
    on = launches(threshold, witness=[], pgd_steps=0)                  # (0 steps: the same values, so the same rounds)
    assert "k_net_descend" in on and "k_frontier_witness" in on and "k_net_eval" not in on
    assert [k for k in on if k not in NEW_CLASSES] == [k for k in off if k != "k_net_eval"]       # nothing else moved
    assert on.count("k_net_descend") == off.count("k_net_eval")


# ---- 4. many jobs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pgd", [None, 4])
@pytest.mark.parametrize("threshold", [None, 1.0])
def test_every_job_s_witness_is_what_it_gets_alone(threshold, pgd):
    """Three jobs in two segments (the third is admitted late, into a reused segment): results and witnesses bit-equal to the runs alone."""
    from tests.test_gpu_frontier_jobs import JOBS, toy_jobs
    choice, lps = toy_jobs()
    K, cap, rounds = 2, 9, 3
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], db) for lp, (_, _, _, db) in zip(lps[:3], JOBS)]
    alone, alone_points = [], []
    for lp, job in zip(lps, jobs):
        kw = {} if threshold is None else {"branching_threshold": threshold}
        alone.append(branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=cap,
                                               decision_bound=job.decision_bound, log=lambda s: None, witness=alone_points, pgd_steps=pgd, **kw))
    points, trace = [], []
    jobs = FrontierJobs(jobs, witness=points, pgd_steps=pgd)
    common = dict(K=K, segments=2, capacity=cap, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace)
    if threshold is None:
        got = verify_properties(choice, lps[0].layers[:-1], jobs, **common)
    else:
        got = verify_properties_threshold(choice, lps[0].layers[:-1], jobs, threshold, **common)
    assert len(points) == len(alone_points) == 3
    assert {row["segment"] for row in trace if row["job"] == 2} <= {0, 1} and any(row["job"] == 2 for row in trace)
    for row in trace:
        assert row["witness_value"] == row["global_ub"], row["job"]
    for j in range(3):
        print("job", j, "alone", alone[j], "together", got[j])
        assert got[j] == alone[j], j
        assert (points[j] is None) == (alone_points[j] is None), j
        if points[j] is not None:
            assert torch.equal(points[j], alone_points[j]), j
    assert any(p is not None for p in points)
