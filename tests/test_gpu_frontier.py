"""The device-resident BaB frontier on the MI355X (gnn_branching_amd/frontier.py; csrc/gnnb_k_frontier.h):

1. gnnb_net_eval against torch fp64 on the geometries of tests/common.py KW_ARCHS;
2. gnnb_frontier_gather / _expand against torch indexing, exact;
3. gnnb_frontier_commit against a Python restatement written here, exact;
4. / 5. branch_and_bound_frontier at K = 1 and K = 4 on toy_kw against a host loop made of the existing public pieces
   (tests/frontier_twin.py: lp.solve_many(lp="dual_device"), GraphChoice.decision / BatchedGraphChoice.decision_many, the keep-or-close rule);
6. soundness of the returned bounds; 7. nothing but the state record crosses to the host in a round; 8. the limits."""
import copy
import math

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, lp_producer
from gnn_branching_amd.frontier import DomainPool, FrontierRun, branch_and_bound_frontier
from tests import margins
from tests.frontier_twin import CKPT, EPS_BAB, INF, LR, N_ITER, engine, masked, toy, twin   # noqa: F401  (engine: the module's fixture)
from tests.test_dual_ascent_cpu import toy_kw_domains
from tests.test_gpu_kw_geometry import Net, seeded_domain

pytestmark = pytest.mark.gpu

NETS = ["kwg_mlp", "kwg_rect", "kwg_gap", "kwg_single", "kwg_s1", "kwg_deep8"]
S = _lib


def torch_fp64(layers, x):
    """The layers in fp64 at the fp32 points x cast up."""
    with torch.no_grad():
        act = x.double()
        for l in layers:
            act = copy.deepcopy(l).double()(act)
    return act


# ---- 1. net_eval ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_net_eval_against_torch_fp64(name, engine):
    """B = 5 points of [-1, 1]^N_0 with five different property rows: within the fp64 device-against-host rule 1e-9 max(1, |value|)
    (tests/test_gpu_kw_geometry.py), and row b of the batch is the same point evaluated alone, bit for bit."""
    net = Net(name)
    B = 5
    x = torch.from_numpy(np.random.RandomState(11).uniform(-1, 1, (B,) + tuple(net.shape)).astype(np.float32))
    props = [net.prop(i, (i + 3) % 10) for i in range(B)]
    got = engine.net_eval(net.fixed, props, x.to(engine.device)).cpu()
    hidden = torch_fp64(net.fixed, x)
    want = torch.stack([torch_fp64([props[b]], hidden[b:b + 1]).reshape(()) for b in range(B)])
    worst = 0.0
    for b in range(B):
        dev = abs(float(got[b]) - float(want[b])) / max(1.0, abs(float(want[b])))
        worst = max(worst, dev)
        print(f"net_eval {name} point {b}: device {float(got[b]):.15g} torch fp64 {float(want[b]):.15g} relative deviation {dev:.3e}")
    margins.record("frontier_net_eval", name, worst_relative_deviation=worst, tolerance=1e-9)
    assert worst <= 1e-9, (name, worst)
    for b in range(B):
        alone = engine.net_eval(net.fixed, [props[b]], x[b:b + 1].to(engine.device)).cpu()
        assert torch.equal(alone, got[b:b + 1]), (name, b)


# ---- 2. gather and expand ---------------------------------------------------------------------------------------------
def random_pool(engine, net, cap, seed):
    """A pool whose every entry is a distinct random value (masks in {-1, 0, 1})."""
    engine.bind(net.fixed, tuple(net.shape))
    pool = DomainPool(engine, cap)
    g = torch.Generator().manual_seed(seed)
    for t in pool.lb + pool.ub + [pool.alpha, pool.beta, pool.bound]:
        t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64))
    pool.mask.copy_(torch.randint(-1, 2, pool.mask.shape, generator=g).to(torch.int8))
    pool.open.fill_(1)
    return pool


def snapshot(pool):
    return [t.clone() for t in pool.arrays()]


def poisoned(n, cols, dtype, dev):
    if dtype in (torch.float64, torch.float32):
        return torch.full((n, cols), float("nan"), dtype=dtype, device=dev)
    return torch.full((n, cols), 77, dtype=dtype, device=dev)


def decisions_for(engine, kinds):
    L = len(engine.sizes) - 2
    table = {"first": [0, 0], "last": [L - 1, engine.sizes[L] - 1], "none": [-1, -1]}
    return [table[k] for k in kinds]


CASES = [([4], ["last"]), ([2], ["none"]), ([5, 0, 3], ["first", "last", "none"])]


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
@pytest.mark.parametrize("slots,kinds", CASES)
def test_gather_against_torch_indexing(name, slots, kinds, engine):
    net = Net(name)
    pool = random_pool(engine, net, 7, 5)
    before = snapshot(pool)
    dev, R, sizes, K = engine.device, engine.R, engine.sizes, len(slots)
    n = K + 1                                             # one row more than asked for: it must stay as it was
    g = torch.Generator().manual_seed(6)
    x_lo = torch.randn(n, sizes[0], generator=g, dtype=torch.float64).to(dev)
    x_hi = x_lo + 0.1
    mask = poisoned(n, R, torch.int8, dev)
    lb, ub = ([poisoned(n, s, torch.float64, dev) for s in sizes[1:]] for _ in range(2))
    lb32, ub32 = ([poisoned(n, s, torch.float32, dev) for s in sizes] for _ in range(2))
    alpha, beta, amb = poisoned(n, R, torch.float64, dev), poisoned(n, R, torch.float64, dev), poisoned(n, R, torch.float32, dev)
    sl = torch.tensor(slots, dtype=torch.int32, device=dev)
    engine.frontier_gather(pool, sl, x_lo, x_hi, mask, lb, ub, lb32, ub32, alpha, beta, amb)
    idx = torch.tensor(slots, device=dev)
    assert torch.equal(mask[:K], pool.mask[idx]) and torch.equal(alpha[:K], pool.alpha[idx]) and torch.equal(beta[:K], pool.beta[idx])
    assert torch.equal(amb[:K], (pool.mask[idx] == -1).float())
    assert torch.equal(lb32[0][:K], x_lo[:K].float()) and torch.equal(ub32[0][:K], x_hi[:K].float())
    for k in range(len(sizes) - 1):
        assert torch.equal(lb[k][:K], pool.lb[k][idx]) and torch.equal(ub[k][:K], pool.ub[k][idx]), k
        assert torch.equal(lb32[k + 1][:K], pool.lb[k][idx].float()) and torch.equal(ub32[k + 1][:K], pool.ub[k][idx].float()), k
    assert bool((mask[K] == 77).all())
    for t in lb + ub + lb32 + ub32 + [alpha, beta, amb]:
        assert bool(torch.isnan(t[K]).all()) and not bool(torch.isnan(t[:K]).any())
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
@pytest.mark.parametrize("slots,kinds", CASES)
def test_expand_against_torch_indexing(name, slots, kinds, engine):
    net = Net(name)
    pool = random_pool(engine, net, 7, 5)
    before = snapshot(pool)
    dev, R, sizes, K = engine.device, engine.R, engine.sizes, len(slots)
    L, n = len(sizes) - 2, 2 * K + 1
    off = np.concatenate([[0], np.cumsum(sizes[1:-1])])
    dec = decisions_for(engine, kinds)
    mask = poisoned(n, R, torch.int8, dev)
    plb, pub = ([poisoned(n, s, torch.float64, dev) for s in sizes[1:]] for _ in range(2))
    alpha, beta = poisoned(n, R, torch.float64, dev), poisoned(n, R, torch.float64, dev)
    split, live = poisoned(n, 1, torch.int32, dev).reshape(-1), poisoned(n, 1, torch.int32, dev).reshape(-1)
    sl = torch.tensor(slots, dtype=torch.int32, device=dev)
    engine.frontier_expand(pool, sl, torch.tensor(dec, dtype=torch.int32, device=dev), mask, plb, pub, split, alpha, beta, live)
    for i, (s, (lay, idx)) in enumerate(zip(slots, dec)):
        for choice in (0, 1):                             # row 2i blocked, 2i + 1 passing: the order of lp_producer._bound_children
            c = 2 * i + choice
            want = pool.mask[s].clone()
            if lay >= 0:
                want[int(off[lay]) + idx] = choice
            assert torch.equal(mask[c], want), (i, choice)
            assert int(live[c]) == (1 if lay >= 0 else 0) and int(split[c]) == (lay if lay >= 0 else L - 1)
            assert torch.equal(alpha[c], pool.alpha[s]) and torch.equal(beta[c], pool.beta[s])
            for k in range(L + 1):
                assert torch.equal(plb[k][c], pool.lb[k][s]) and torch.equal(pub[k][c], pool.ub[k][s])
    assert bool((mask[2 * K] == 77).all()) and int(split[2 * K]) == 77 and int(live[2 * K]) == 77
    for t in plb + pub + [alpha, beta]:
        assert bool(torch.isnan(t[2 * K]).all()) and not bool(torch.isnan(t[:2 * K]).any())
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a, b)


# ---- 3. commit ----------------------------------------------------------------------------------------------------------
def commit_reference(pool, state, slots, ch, eps, decision_bound, sizes):
    """gnnb_frontier_commit restated on host tensors.  pool: dict of CPU tensors (changed in place); state: list of 9 floats; ch: dict of
    the 2K children's CPU tensors.  Returns the new state."""
    K, n, L = len(slots), 2 * len(slots), len(sizes) - 2
    off = np.concatenate([[0], np.cumsum(sizes[1:-1])])
    rmask, undecided = ch["mask"].clone(), [False] * n
    for c in range(n):
        if not ch["live"][c]:
            continue
        for k in range(L):
            m = rmask[c, off[k]:off[k + 1]]
            lo, up = ch["lb"][k][c], ch["ub"][k][c]
            m = torch.where((m == -1) & (lo >= 0), torch.ones_like(m), m)
            m = torch.where((m == -1) & (up <= 0), torch.zeros_like(m), m)
            rmask[c, off[k]:off[k + 1]] = m
        undecided[c] = bool((rmask[c] == -1).any())
    feasible = [bool(ch["live"][c]) and not bool(ch["infeasible"][c]) for c in range(n)]
    gub = min([state[S.FS_GLOBAL_UB]] + [float(ch["ub_value"][c]) for c in range(n) if feasible[c]])
    closed_lb, in_use = state[S.FS_CLOSED_LB], int(state[S.FS_IN_USE])
    kept, n_closed = [], 0
    for c in range(n):
        if not feasible[c]:
            continue
        lb = float(ch["bound"][c])
        if undecided[c] and lb < gub - eps and (decision_bound is None or lb < decision_bound):
            kept.append(c)
        else:
            closed_lb, n_closed = min(closed_lb, lb), n_closed + 1
    for i, s in enumerate(slots):
        if not ch["live"][2 * i] and not ch["live"][2 * i + 1]:
            closed_lb, n_closed = min(closed_lb, float(pool["bound"][s])), n_closed + 1
    for s in slots:
        pool["open"][s] = 0
    for r, c in enumerate(kept):
        d = slots[r] if r < K else in_use + (r - K)
        pool["mask"][d], pool["alpha"][d], pool["beta"][d], pool["bound"][d], pool["open"][d] = rmask[c], ch["alpha"][c], ch["beta"][c], ch["bound"][c], 1
        for k in range(L + 1):
            pool["lb"][k][d], pool["ub"][k][d] = ch["lb"][k][c], ch["ub"][k][c]
        in_use = max(in_use, d + 1)
    open_bounds = [float(pool["bound"][s]) for s in range(in_use) if pool["open"][s]]
    return [gub, closed_lb, min(open_bounds + [INF]), float(len(open_bounds)), float(in_use), float(len(kept)), float(n_closed),
            float(sum(bool(ch["live"][c]) and bool(ch["infeasible"][c]) for c in range(n))), 0.0]


def six_children(sizes, R, seed, eps):
    """2K = 6 children, one of each kind: 0 infeasible, 1 dead, 2 at global_ub - eps / 2, 3 at or above the decision bound 0.1 only,
    4 fully decided once its bounds resolve its last two undecided nodes, 5 kept, with one node resolved each way.  global_ub becomes
    0.5 (child 5's value; the infeasible child's 0.1 and the dead child's NaN do not count)."""
    g = torch.Generator().manual_seed(seed)
    n = 6
    mask = torch.full((n, R), -1, dtype=torch.int8)
    lb = [-torch.rand(n, s, generator=g, dtype=torch.float64) - 0.1 for s in sizes[1:]]
    ub = [torch.rand(n, s, generator=g, dtype=torch.float64) + 0.1 for s in sizes[1:]]
    mask[:, 3], mask[:, 7] = 0, 1                          # split nodes everywhere
    mask[4] = torch.randint(0, 2, (R,), generator=g).to(torch.int8)
    mask[4, 0] = mask[4, R - 1] = -1                       # ... which its bounds decide
    lb[0][4, 0], ub[-2][4, sizes[-2] - 1] = 0.0, 0.0       # (first node of the first ReLU layer passing, last of the last blocked)
    lb[0][5, 1], ub[0][5, 2] = 0.25, -0.0                  # child 5: node 1 -> 1, node 2 -> 0 (up = -0.0 <= 0)
    return {"mask": mask, "lb": lb, "ub": ub, "infeasible": torch.tensor([1, 0, 0, 0, 0, 0], dtype=torch.int32),
            "live": torch.tensor([1, 0, 1, 1, 1, 1], dtype=torch.int32),
            "bound": torch.tensor([-3.0, float("nan"), 0.5 - eps / 2, 0.2, -0.5, -1.0], dtype=torch.float64),
            "ub_value": torch.tensor([0.1, float("nan"), 0.9, 0.8, 0.7, 0.5], dtype=torch.float64),
            "alpha": torch.rand(n, R, generator=g, dtype=torch.float64), "beta": torch.rand(n, R, generator=g, dtype=torch.float64)}


def run_commit(engine, net, cap, slots, other_open, in_use, ch, eps, decision_bound, seed):
    """One commit on the device and in the restatement, from the same pool; returns (device pool arrays, device state, reference pool,
    reference state)."""
    pool = random_pool(engine, net, cap, seed)
    pool.open.zero_()
    for s in list(slots) + list(other_open):
        pool.open[s] = 1
    state0 = [1.0, INF, INF, float(len(slots) + len(other_open)), float(in_use), 0.0, 0.0, 0.0, 0.0]
    pool.state.copy_(torch.tensor(state0, dtype=torch.float64))
    ref = {"mask": pool.mask.cpu(), "lb": [t.cpu() for t in pool.lb], "ub": [t.cpu() for t in pool.ub], "alpha": pool.alpha.cpu(),
           "beta": pool.beta.cpu(), "bound": pool.bound.cpu(), "open": pool.open.cpu()}
    dev = engine.device
    d = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in ch.items()}
    engine.frontier_commit(pool, torch.tensor(slots, dtype=torch.int32, device=dev), d["mask"], d["lb"], d["ub"], d["infeasible"], d["bound"], d["alpha"],
                           d["beta"], d["ub_value"], d["live"], pool.state, eps=eps, decision_bound=decision_bound)
    want_state = commit_reference(ref, state0, slots, ch, eps, decision_bound, engine.sizes)
    return pool, pool.state.cpu().tolist(), ref, want_state


def assert_pool_equals(pool, ref):
    assert torch.equal(pool.open.cpu(), ref["open"])
    assert torch.equal(pool.mask.cpu(), ref["mask"]) and torch.equal(pool.alpha.cpu(), ref["alpha"]) and torch.equal(pool.beta.cpu(), ref["beta"])
    assert torch.equal(pool.bound.cpu(), ref["bound"])
    for a, b in zip(pool.lb + pool.ub, ref["lb"] + ref["ub"]):
        assert torch.equal(a.cpu(), b)


@pytest.mark.parametrize("decision_bound", [None, 0.1])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_commit_against_the_restatement(name, decision_bound, engine):
    net = Net(name)
    engine.bind(net.fixed, tuple(net.shape))
    eps = 1e-4
    ch = six_children(engine.sizes, engine.R, 21, eps)
    pool, got, ref, want = run_commit(engine, net, 8, [5, 0, 3], [1], 6, ch, eps, decision_bound, 31)
    print("state", got, "restated", want)
    assert got == want
    assert_pool_equals(pool, ref)
    kept = [5] if decision_bound is not None else [3, 5]   # (in child order)
    assert want[S.FS_GLOBAL_UB] == 0.5 and want[S.FS_KEPT] == len(kept) and want[S.FS_INFEASIBLE] == 1 and want[S.FS_CLOSED] == 4 - len(kept)
    assert want[S.FS_CLOSED_LB] == -0.5 and want[S.FS_N_OPEN] == 1 + len(kept)
    stored = ref["mask"][5 if decision_bound is not None else 0]      # child 5's resolved mask sits in the parents' slot of its rank
    assert int(stored[1]) == 1 and int(stored[2]) == 0 and bool((stored == -1).any())
    # the same children in another pool, other slot numbers, the same order: the same record and the same rows by rank
    pool2, got2, ref2, want2 = run_commit(engine, net, 9, [6, 2, 4], [7], 8, ch, eps, decision_bound, 32)
    assert got2 == want2
    assert_pool_equals(pool2, ref2)
    assert got2[:S.FS_LOWEST_OPEN] == got[:S.FS_LOWEST_OPEN] and got2[S.FS_KEPT:] == got[S.FS_KEPT:]
    for r in range(len(kept)):
        a, b = [5, 0, 3][r], [6, 2, 4][r]
        assert torch.equal(pool.mask[a], pool2.mask[b]) and torch.equal(pool.alpha[a], pool2.alpha[b]) and float(pool.bound[a]) == float(pool2.bound[b])
        for x, y in zip(pool.lb + pool.ub, pool2.lb + pool2.ub):
            assert torch.equal(x[a], y[b])


def test_commit_more_kept_children_than_parents_and_a_parent_without_children(engine):
    """K = 2: parent 0 has no decision (both rows dead: closed at its own bound), both children of parent 1 are kept -- the second kept
    child is of rank 1 < K and takes the dead parent's slot; with K = 1 and two kept children the second goes to slot in_use."""
    net = Net("kwg_mlp")
    engine.bind(net.fixed, tuple(net.shape))
    ch = six_children(engine.sizes, engine.R, 22, 1e-4)
    two = {k: ([t[[1, 1, 3, 5]] for t in v] if isinstance(v, list) else v[[1, 1, 3, 5]]) for k, v in ch.items()}
    pool, got, ref, want = run_commit(engine, net, 8, [2, 6], [0], 7, two, 1e-4, None, 33)
    assert got == want and want[S.FS_KEPT] == 2 and want[S.FS_CLOSED] == 1 and math.isfinite(want[S.FS_CLOSED_LB])
    assert int(ref["open"][2]) == 1 and int(ref["open"][6]) == 1 and want[S.FS_N_OPEN] == 3 and want[S.FS_IN_USE] == 7
    assert_pool_equals(pool, ref)
    one = {k: ([t[[3, 5]] for t in v] if isinstance(v, list) else v[[3, 5]]) for k, v in ch.items()}
    pool, got, ref, want = run_commit(engine, net, 8, [2], [0, 4], 5, one, 1e-4, None, 34)
    assert got == want and want[S.FS_KEPT] == 2 and want[S.FS_IN_USE] == 6 and int(ref["open"][5]) == 1 and int(ref["open"][2]) == 1
    assert_pool_equals(pool, ref)


def test_compaction_moves_the_open_slots_to_the_front_in_slot_order(engine):
    """DomainPool.compact (what the loop does when the slots above the ones in use run out) against torch indexing."""
    pool = random_pool(engine, Net("kwg_mlp"), 7, 41)
    pool.open.copy_(torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.int32))
    before = snapshot(pool)
    pool.compact(4)
    keep = torch.tensor([0, 2, 3, 6], device=engine.device)
    assert pool.open.cpu().tolist() == [1, 1, 1, 1, 0, 0, 0] and float(pool.state[S.FS_IN_USE]) == 4.0
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a[keep], b[:4]) and b.is_contiguous()


# ---- 4. - 6. the loop on toy_kw against a host loop of the existing pieces --------------------------------------------
_shared = {}


def runs(K, rounds):
    if (K, rounds) not in _shared:
        lp, choice, _ = toy()
        trace = []
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace)
        _shared[(K, rounds)] = (twin(K, rounds), res, trace)
    return _shared[(K, rounds)]


def assert_same_run(twin, res, trace):
    glb, gub, rounds, bounded, reason = res
    print("twin", twin, "frontier", res)
    assert [t["decisions"] for t in trace] == twin["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]   # bit for bit: Python floats of the same fp64 values
    assert glb == twin["global_lb"]
    assert abs(gub - twin["global_ub"]) <= 1e-9 * max(1.0, abs(twin["global_ub"]))
    assert bounded == 1 + sum(len(t["live"]) for t in trace)


def test_k1_equals_the_host_loop_of_the_existing_pieces():
    twin, res, trace = runs(1, 4)
    assert twin["branches"] >= 3
    assert_same_run(twin, res, trace)


def test_k4_equals_the_host_loop_of_the_existing_pieces():
    twin, res, trace = runs(4, 3)
    assert twin["branches"] >= 3
    assert_same_run(twin, res, trace)


def test_k4_in_a_pool_just_above_the_smallest():
    """capacity = 2K + 2: the rounds it runs give the roomy run's bounds; it may stop early ("capacity"), then with a global_lb no higher."""
    _, roomy, rtrace = runs(4, 3)
    lp, choice, _ = toy()
    trace = []
    tight = branch_and_bound_frontier(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=3, capacity=10, log=lambda s: None, trace=trace)
    print("roomy", roomy, "tight", tight)
    assert len(trace) >= 1
    for a, b in zip(trace, rtrace):
        assert a["decisions"] == b["decisions"] and a["live"] == b["live"] and a["infeasible"] == b["infeasible"]
        assert [x for x, l in zip(a["child_bounds"], a["live"]) if l] == [x for x, l in zip(b["child_bounds"], b["live"]) if l]
    assert tight[0] <= roomy[0]
    assert tight[0] == roomy[0] if len(trace) == len(rtrace) else tight[4] == "capacity"


@pytest.mark.parametrize("K,rounds", [(1, 4), (4, 3)])
def test_soundness(K, rounds, engine):
    """As tests/test_gpu_dual_ascent.py test_threshold_loop_with_dual_device_children: global_lb <= global_ub, global_lb at most the
    network's minimum over 256 sampled points of the box + 1e-5, and no higher than the global_ub of the HiGHS threshold loop."""
    from gnn_branching_amd.graphnet.graph_score import GraphChoice
    from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
    _, (glb, gub, *_), _ = runs(K, rounds)
    lp0, _ = toy_kw_domains()
    assert glb <= gub
    with torch.no_grad():
        x = lp0.input_lb.float() + (lp0.input_ub - lp0.input_lb).float() * torch.rand((256,) + lp0.shapes[0], generator=torch.Generator().manual_seed(0))
        for l in lp0.layers:
            x = l(x)
    assert glb <= float(x.min()) + 1e-5
    if "highs" not in _shared:
        lp = lp_producer.LayerGraphLP(lp0.layers, lp0.input_lb.float(), lp0.input_ub.float(), bounds="kw_device", engine=engine)
        root_mask = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
        choice = GraphChoice(root_mask, CKPT)
        choice.verbose = False

        def kw(sub, icp, order, sparsest):
            return choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, order, sparsest)
        _shared["highs"] = lp_producer.branch_and_bound_threshold(lp, lp_producer.gnn_scorer(choice, lp), kw, lp.layers, max_branches=3,
                                                                  log=lambda s: None, child_lp="highs")
    assert glb <= _shared["highs"][1] + 1e-6


# ---- 7. device residency ----------------------------------------------------------------------------------------------
def test_a_round_copies_nothing_but_the_state_record():
    """With the sync debug mode at "error" every synchronising call of torch raises: the body of a round runs under it, the read of the
    state record is the one exemption."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy()
    run = FrontierRun(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB)
    st = run.root()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            run.pool.state.cpu()
            live = False
        except RuntimeError:
            live = True
        finally:
            torch.cuda.set_sync_debug_mode(before)
        if not live:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
        for _ in range(2):
            n_open, in_use = int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
            assert n_open >= 1
            torch.cuda.set_sync_debug_mode("error")
            run.launch_round(min(4, n_open), in_use)
            with pytest.raises(RuntimeError):             # the mode is live: the state read is a synchronising copy
                run.read_state()
            torch.cuda.set_sync_debug_mode(before)        # the explicit exemption
            st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert st[S.FS_KEPT] + st[S.FS_CLOSED] + st[S.FS_INFEASIBLE] >= 2
    run.check_status()


# ---- 8. limits ---------------------------------------------------------------------------------------------------------
def test_limits(engine):
    """kwg_over (a 4097-node layer) is refused by every step before a launch and the handle stays usable; an unbound handle is
    GNNB_E_STATE; K < 1 GNNB_E_INVALID; a workspace one byte short GNNB_E_NOMEM."""
    from gnn_branching_amd.engine import ScorerEngine
    dev = engine.device
    fresh = ScorerEngine(None)
    x1 = torch.zeros(1, 4, dtype=torch.float32, device=dev)
    o1 = torch.zeros(1, dtype=torch.float64, device=dev)
    assert fresh.lib.gnnb_net_eval(fresh.h, x1.data_ptr(), x1.data_ptr(), x1.data_ptr(), 1, o1.data_ptr(), o1.data_ptr(), 8, None) == -3
    assert b"gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    pool_s, ch_s = _lib.Pool(), _lib.Children()
    import ctypes as C
    assert fresh.lib.gnnb_frontier_commit(fresh.h, C.byref(pool_s), None, 1, C.byref(ch_s), 1e-4, 0.0, None, None, 0, None) == -3
    assert fresh.lib.gnnb_frontier_gather(fresh.h, C.byref(pool_s), None, 1, None, None, None, None, None, None, None, None, None, None, None) == -3
    assert fresh.lib.gnnb_frontier_expand(fresh.h, C.byref(pool_s), None, None, 1, None, None, None, None, None, None, None, None) == -3
    assert fresh.lib.gnnb_net_eval_workspace_bytes(fresh.h, 1) == 0 and fresh.lib.gnnb_frontier_commit_workspace_bytes(fresh.h, 1) == 0

    over = Net("kwg_over")
    d = seeded_domain(over, 0)
    x = d.x_lo[None].float().to(dev)
    with pytest.raises(RuntimeError, match=r"gnnb_net_eval failed \(-1\).*4097 nodes"):
        engine.net_eval(over.fixed, [over.prop(d.gt, d.cls)], x)
    pool = DomainPool(engine, 3)
    sl = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = lambda n, dt: [torch.zeros(n, s, dtype=dt, device=dev) for s in engine.sizes[1:]]     # noqa: E731
    R = engine.R
    m2, a2, b2 = torch.zeros(2, R, dtype=torch.int8, device=dev), torch.zeros(2, R, dtype=torch.float64, device=dev), torch.zeros(2, R, dtype=torch.float64, device=dev)
    i2, f2 = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_expand failed \(-1\).*4097 nodes"):
        engine.frontier_expand(pool, sl, torch.zeros(1, 2, dtype=torch.int32, device=dev), m2, rows(2, torch.float64), rows(2, torch.float64), i2, a2, b2, i2.clone())
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit failed \(-1\).*4097 nodes"):
        engine.frontier_commit(pool, sl, m2, rows(2, torch.float64), rows(2, torch.float64), i2, f2, a2, b2, f2, i2, pool.state)
    f32rows = [torch.zeros(1, s, dtype=torch.float32, device=dev) for s in engine.sizes]
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_gather failed \(-1\).*4097 nodes"):
        engine.frontier_gather(pool, sl, torch.zeros(1, engine.sizes[0], dtype=torch.float64, device=dev), torch.zeros(1, engine.sizes[0], dtype=torch.float64, device=dev),
                               m2, rows(1, torch.float64), rows(1, torch.float64), f32rows, [t.clone() for t in f32rows], a2, b2, torch.zeros(1, R, dtype=torch.float32, device=dev))

    # the handle stays usable: a network within the cap, then K < 1 and the short workspaces
    net = Net("kwg_mlp")
    xs = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (2,) + tuple(net.shape)).astype(np.float32)).to(dev)
    props = [net.prop(0, 1), net.prop(2, 3)]
    first = engine.net_eval(net.fixed, props, xs)
    assert bool(torch.isfinite(first).all())
    need = engine.lib.gnnb_net_eval_workspace_bytes(engine.h, 2)
    assert need > 0
    with pytest.raises(RuntimeError, match=r"gnnb_net_eval failed \(-4\)"):
        engine.net_eval(net.fixed, props, xs, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert torch.equal(engine.net_eval(net.fixed, props, xs, workspace=torch.empty(need, dtype=torch.uint8, device=dev)), first)
    pw, pb = engine._prop(props)
    assert engine.lib.gnnb_net_eval(engine.h, xs.data_ptr(), pw.data_ptr(), pb.data_ptr(), 0, first.data_ptr(), xs.data_ptr(), 1 << 20, None) == -1
    ch = six_children(engine.sizes, engine.R, 21, 1e-4)
    pool = random_pool(engine, net, 8, 31)
    pool.state.copy_(torch.tensor([1.0, INF, INF, 8.0, 8.0, 0, 0, 0, 0], dtype=torch.float64))
    d = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in ch.items()}
    need = engine.lib.gnnb_frontier_commit_workspace_bytes(engine.h, 3)
    slots = torch.tensor([5, 0, 3], dtype=torch.int32, device=dev)
    before = snapshot(pool)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit failed \(-4\)"):
        engine.frontier_commit(pool, slots, d["mask"], d["lb"], d["ub"], d["infeasible"], d["bound"], d["alpha"], d["beta"], d["ub_value"], d["live"], pool.state,
                               workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a, b)
    assert math.isinf(float(pool.state[S.FS_CLOSED_LB]))
