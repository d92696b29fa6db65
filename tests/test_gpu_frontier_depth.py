"""A frontier round that splits each parent on several ReLUs (``LayerGraphLP(..., split_depth=D)``) on the MI355X:

1. gnnb_frontier_expand_depth against the twin of tests/frontier_depth_twin.py, exact; 2. at depth 1 both entry points against
gnnb_frontier_expand / gnnb_frontier_commit, bit for bit; 3. gnnb_frontier_commit_depth against the twin, exact, up to the pool's last
slot and one past it; 4. the children's bounds against the same rows assembled by torch indexing in another batch order; 5. whole runs on
toy_kw: split_depth=1 against None, split_depth=3 against a host loop of the twins and the existing batch entry points, the traced depths,
a full first round; 6. soundness against certified exact minima; 7. nothing but the state record crosses to the host; 8. the limits."""
import contextlib
import ctypes as C
import math

import pytest
import torch

from gnn_branching_amd import _lib, frontier
from gnn_branching_amd.frontier import DomainPool, FrontierRun, branch_and_bound_frontier
from tests import frontier_depth_twin as T
from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, engine, masked, toy   # noqa: F401  (engine: the module's fixture)
from tests.test_gpu_exact_frontier import BRANCHES, CASES, MODES, case_lp, recorded, run_case
from tests.test_gpu_frontier import poisoned, random_pool, six_children, snapshot
from tests.test_gpu_kw_geometry import Net

pytestmark = pytest.mark.gpu
S = _lib


@contextlib.contextmanager
def split_depth(lp, D):
    """``lp.split_depth = D`` inside the block: the problems of the twins are shared between tests (``LayerGraphLP(..., split_depth=D)``
    sets the same attribute)."""
    before = getattr(lp, "split_depth", None)
    lp.split_depth = D
    try:
        yield lp
    finally:
        lp.split_depth = before


def depth_frontier_run(lp, choice, D, **kw):
    with split_depth(lp, D):
        return FrontierRun(lp, choice, lp.layers, n_iter=N_ITER, lr=LR, eps=EPS_BAB, **kw)


def bits(t):
    """t on the host with floats as their bit patterns: NaNs compare like any other value."""
    t = t.cpu()
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def pool_to_host(pool):
    return {"mask": pool.mask.cpu(), "lb": [t.cpu() for t in pool.lb], "ub": [t.cpu() for t in pool.ub], "alpha": pool.alpha.cpu(),
            "beta": pool.beta.cpu(), "bound": pool.bound.cpu(), "open": pool.open.cpu()}


def assert_pool_is(pool, ref):
    for a, b in zip([pool.mask, pool.alpha, pool.beta, pool.bound, pool.open] + pool.lb + pool.ub,
                    [ref["mask"], ref["alpha"], ref["beta"], ref["bound"], ref["open"]] + ref["lb"] + ref["ub"]):
        assert same(a, b)


def child_rows(n, engine):
    """Poisoned outputs of an expand of n rows: (mask, plb, pub, split, alpha, beta, live)."""
    dev, R, sizes = engine.device, engine.R, engine.sizes
    plb, pub = ([poisoned(n, s, torch.float64, dev) for s in sizes[1:]] for _ in range(2))
    return (poisoned(n, R, torch.int8, dev), plb, pub, poisoned(n, 1, torch.int32, dev).reshape(-1), poisoned(n, R, torch.float64, dev),
            poisoned(n, R, torch.float64, dev), poisoned(n, 1, torch.int32, dev).reshape(-1))


def rows_to_host(rows):
    mask, plb, pub, split, alpha, beta, live = rows
    return {"mask": mask.cpu(), "plb": [t.cpu() for t in plb], "pub": [t.cpu() for t in pub], "split": split.cpu(), "alpha": alpha.cpu(),
            "beta": beta.cpu(), "live": live.cpu()}


def assert_rows_are(rows, want):
    mask, plb, pub, split, alpha, beta, live = rows
    assert same(mask, want["mask"]) and same(split, want["split"]) and same(live, want["live"])
    assert same(alpha, want["alpha"]) and same(beta, want["beta"])
    for a, b in zip(plb + pub, want["plb"] + want["pub"]):
        assert same(a, b)


# ---- 1. expand against the twin -----------------------------------------------------------------------------------------------------------
KINDS = [["full"], ["full", "outside", "none"], ["one", "over", "bad"], ["over", "full", "one"]]
IN_POOL = [5, 0, 3]


def lists_for(sizes, kinds, depth):
    """(slots, cand0, cand_dec) in a pool of 7 slots.  full: ``depth`` nodes, the first node of the first ReLU layer and (from depth 2 on)
    the last of the last among them; one: the last node of the last layer alone; none: no node; over: depth + 1 nodes (dead rows);
    bad: a list whose last entry names no node; outside: slot 9 with a node listed."""
    off, L = T.offsets(sizes), len(sizes) - 2
    R = off[-1]

    def pair(r):
        lay = max(l for l in range(L) if off[l] <= r)
        return [lay, r - off[lay]]
    slots, cand0, cand_dec = [], [0], []
    for i, kind in enumerate(kinds):
        slots.append(9 if kind == "outside" else IN_POOL[i])
        nodes = {"full": [pair(r) for r in sorted([0, R - 1, 17, 23, 29, 31, 37, 41][:depth])], "one": [pair(R - 1)], "none": [],
                 "over": [pair(r) for r in [1, 3, 5, 7, 11, 13, 19, 27, 33][:depth + 1]],
                 "bad": ([[0, 2]] if depth > 1 else []) + [[L - 1, sizes[L]]], "outside": [[0, 0]]}[kind]
        cand_dec += nodes
        cand0.append(len(cand_dec))
    return slots, cand0, cand_dec


@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("kinds", KINDS, ids=["-".join(k) for k in KINDS])
def test_expand_against_the_twin(name, depth, kinds, engine):
    net = Net(name)
    pool = random_pool(engine, net, 7, 5)
    before = snapshot(pool)
    dev, sizes, K, Cn = engine.device, engine.sizes, len(kinds), 2 ** depth
    slots, cand0, cand_dec = lists_for(sizes, kinds, depth)
    rows = child_rows(K * Cn + 1, engine)                 # one row more than asked for: it must stay as it was
    want = rows_to_host(rows)
    engine.frontier_expand_depth(pool, torch.tensor(slots, dtype=torch.int32, device=dev), depth, torch.tensor(cand0, dtype=torch.int32, device=dev),
                                 torch.tensor(cand_dec, dtype=torch.int32, device=dev).reshape(-1, 2), *rows)
    T.expand(pool_to_host(pool), slots, depth, cand0, cand_dec, sizes, want)
    assert_rows_are(rows, want)
    live = want["live"].tolist()
    for i, kind in enumerate(kinds):                      # the twin's rows are what this test means them to be
        m = {"full": depth, "one": 1}.get(kind, 0)
        assert live[Cn * i:Cn * i + Cn] == [1] * (2 ** m if m else 0) + [0] * (Cn - (2 ** m if m else 0)), (kind, live)
        if kind == "full":
            assert int(want["split"][Cn * i]) == 0
        if kind == "one":
            assert int(want["split"][Cn * i]) == len(sizes) - 3 and int(want["mask"][Cn * i + 1, engine.R - 1]) == 1
    assert live[K * Cn] == 77 and bool((want["mask"][K * Cn] == 77).all())
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a, b)


# ---- 2. depth 1 is the existing entry points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
@pytest.mark.parametrize("slots", [[5, 0, 3], [5, 9, 3], [4]])
def test_expand_at_depth_1_is_gnnb_frontier_expand(name, slots, engine):
    net = Net(name)
    pool = random_pool(engine, net, 7, 5)
    dev, sizes, K = engine.device, engine.sizes, len(slots)
    L = len(sizes) - 2
    dec = [[0, 0], [L - 1, sizes[L] - 1], [-1, -1]][:K]
    sl, dec_t = torch.tensor(slots, dtype=torch.int32, device=dev), torch.tensor(dec, dtype=torch.int32, device=dev)
    old, new = child_rows(2 * K + 1, engine), child_rows(2 * K + 1, engine)
    engine.frontier_expand(pool, sl, dec_t, *old)
    engine.frontier_expand_depth(pool, sl, 1, torch.arange(K + 1, dtype=torch.int32, device=dev), dec_t, *new)
    assert_rows_are(new, rows_to_host(old))
    assert old[6][:2 * K].cpu().tolist() == [v for s, d in zip(slots, dec) for v in [int(s < 7 and d[0] >= 0)] * 2]


def to_dev(ch, dev):
    return {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in ch.items()}


def commit_on_device(engine, net, cap, slots, other_open, in_use, ch, eps, decision_bound, seed, depth):
    """One commit from a seeded random pool: depth None -> gnnb_frontier_commit, else gnnb_frontier_commit_depth.  Returns (pool, the pool
    as it was on the host, the record before)."""
    pool = random_pool(engine, net, cap, seed)
    pool.open.zero_()
    for s in list(slots) + list(other_open):
        if s < cap:
            pool.open[s] = 1
    state0 = [1.0, INF, INF, float(len(slots) + len(other_open)), float(in_use), 0.0, 0.0, 0.0, 0.0]
    pool.state.copy_(torch.tensor(state0, dtype=torch.float64))
    ref = pool_to_host(pool)
    d = to_dev(ch, engine.device)
    args = (d["mask"], d["lb"], d["ub"], d["infeasible"], d["bound"], d["alpha"], d["beta"], d["ub_value"], d["live"], pool.state)
    sl = torch.tensor(slots, dtype=torch.int32, device=engine.device)
    if depth is None:
        engine.frontier_commit(pool, sl, *args, eps=eps, decision_bound=decision_bound)
    else:
        engine.frontier_commit_depth(pool, sl, depth, *args, eps=eps, decision_bound=decision_bound)
    return pool, ref, state0


@pytest.mark.parametrize("decision_bound", [None, 0.1])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_commit_at_depth_1_is_gnnb_frontier_commit(name, decision_bound, engine):
    net = Net(name)
    engine.bind(net.fixed, tuple(net.shape))
    ch = six_children(engine.sizes, engine.R, 21, 1e-4)
    old, _, _ = commit_on_device(engine, net, 8, [5, 0, 3], [1], 6, ch, 1e-4, decision_bound, 31, None)
    new, _, _ = commit_on_device(engine, net, 8, [5, 0, 3], [1], 6, ch, 1e-4, decision_bound, 31, 1)
    assert same(old.state, new.state) and float(new.state[S.FS_KEPT]) >= 1
    for a, b in zip(snapshot(old), snapshot(new)):
        assert same(a, b)
    # K = 1 with two kept children: the second lands above in_use, the same way
    one = {k: ([t[[3, 5]] for t in v] if isinstance(v, list) else v[[3, 5]]) for k, v in ch.items()}
    old, _, _ = commit_on_device(engine, net, 8, [2], [0, 4], 5, one, 1e-4, None, 34, None)
    new, _, _ = commit_on_device(engine, net, 8, [2], [0, 4], 5, one, 1e-4, None, 34, 1)
    assert same(old.state, new.state) and float(new.state[S.FS_IN_USE]) == 6.0
    for a, b in zip(snapshot(old), snapshot(new)):
        assert same(a, b)


# ---- 3. commit against the twin ------------------------------------------------------------------------------------------------------------
def composed(ch6, idx):
    """Child rows picked from ``six_children``'s six kinds (0 infeasible, 1 dead, 2 closed by global_ub - eps, 3 closed by the decision
    bound only, 4 decided by its bounds, 5 kept), each row told apart: alpha shifted by its row number, a kept row's bound lowered by it."""
    ch = {k: ([t[idx].clone() for t in v] if isinstance(v, list) else v[idx].clone()) for k, v in ch6.items()}
    n = len(idx)
    ch["alpha"] += torch.arange(n, dtype=torch.float64)[:, None]
    for c, kind in enumerate(idx):
        if kind == 5:
            ch["bound"][c] -= 0.01 * c
    return ch


def commit_both(engine, name, cap, slots, other_open, in_use, idx, depth, decision_bound, seed):
    net = Net(name)
    engine.bind(net.fixed, tuple(net.shape))
    ch = composed(six_children(engine.sizes, engine.R, 21, 1e-4), idx)
    assert len(idx) == len(slots) << depth
    pool, ref, state0 = commit_on_device(engine, net, cap, slots, other_open, in_use, ch, 1e-4, decision_bound, seed, depth)
    want = T.commit(ref, state0, slots, 2 ** depth, ch, 1e-4, decision_bound, engine.sizes)
    got = pool.state.cpu().tolist()
    print("state", got, "twin", want)
    assert got == want
    assert_pool_is(pool, ref)
    return want, ref, ch


@pytest.mark.parametrize("decision_bound", [None, 0.1])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_commit_against_the_twin(name, decision_bound, engine):
    """Depth 2 with K = 3 and depth 3 with K = 2: every kind of child, more kept children than parents, a parent without a live child."""
    kept3 = 0 if decision_bound is not None else 1               # kind 3 is below global_ub - eps and above the decision bound
    want, ref, ch = commit_both(engine, name, 16, [5, 0, 3], [1], 6, [5, 0, 5, 5, 1, 1, 1, 1, 4, 2, 3, 5], 2, decision_bound, 41)
    assert want[S.FS_KEPT] == 4 + kept3 > 3 and want[S.FS_INFEASIBLE] == 1 and want[S.FS_CLOSED] == 3 - kept3 + 1 and want[S.FS_OVERFLOW] == 0
    assert want[S.FS_GLOBAL_UB] == 0.5 and want[S.FS_N_OPEN] == 1 + want[S.FS_KEPT] and want[S.FS_IN_USE] == 6 + want[S.FS_KEPT] - 3
    assert [float(ref["bound"][s]) for s in (5, 0, 3)] == [float(ch["bound"][c]) for c in (0, 2, 3)]      # ranks 0..2: the parents' slots, in their order
    assert float(ref["bound"][6]) == float(ch["bound"][10 if kept3 else 11])                               # rank 3 = K: slot in_use
    assert want[S.FS_CLOSED_LB] <= float(pool_bound_of_dead_parent(engine, name, 16, 41, 0))
    want, ref, ch = commit_both(engine, name, 21, [2, 6], [0], 7, [5, 0, 5, 5, 4, 2, 3, 5] + [1] * 8, 3, decision_bound, 42)
    assert want[S.FS_KEPT] == 4 + kept3 > 2 and want[S.FS_CLOSED] == 3 - kept3 + 1 and want[S.FS_IN_USE] == 7 + want[S.FS_KEPT] - 2


def pool_bound_of_dead_parent(engine, name, cap, seed, slot):
    """The bound the seeded pool holds for ``slot`` (the parent whose rows are all dead is closed at it)."""
    return random_pool(engine, Net(name), cap, seed).bound[slot].cpu()


@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_commit_up_to_the_pool_s_last_slot_and_one_past_it(name, engine):
    """Depth 2, K = 2, all 8 children kept, 4 slots in use: a pool of 4 + (C - 1) K = 10 slots holds them all; in one of 9 the child of the
    last rank finds no slot, record [8] counts it and closed_lb takes its bound."""
    want, ref, ch = commit_both(engine, name, 10, [1, 3], [0], 4, [5] * 8, 2, None, 43)
    assert want[S.FS_KEPT] == 8 and want[S.FS_OVERFLOW] == 0 and want[S.FS_IN_USE] == 10 and math.isinf(want[S.FS_CLOSED_LB])
    assert [float(ref["bound"][s]) for s in (1, 3, 4, 5, 6, 7, 8, 9)] == ch["bound"].tolist()
    want, ref, ch = commit_both(engine, name, 9, [1, 3], [0], 4, [5] * 8, 2, None, 43)
    assert want[S.FS_KEPT] == 7 and want[S.FS_OVERFLOW] == 1 and want[S.FS_CLOSED] == 1 and want[S.FS_IN_USE] == 9
    assert want[S.FS_CLOSED_LB] == float(ch["bound"][7]) and want[S.FS_N_OPEN] == 8


# ---- 4. the children's bounds ---------------------------------------------------------------------------------------------------------------
def test_children_s_bounds_are_those_of_the_same_rows_in_another_batch_order():
    """Round 2 of a depth run on toy_kw, by hand: the rows gnnb_frontier_expand_depth writes, bounded, against the same rows assembled from
    the pool by torch indexing and bounded in reverse order.  The batch kernels treat rows independently, so any difference is expand's."""
    lp, choice, _ = toy()
    run = depth_frontier_run(lp, choice, 3, K=4)
    st = run.root()
    run.launch_round(1, int(st[S.FS_IN_USE]), 3)
    st = run.read_state()
    n_open, in_use = int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
    assert n_open >= 2
    k, d, Cn = 2, 2, 4
    P, Ch, eng, pool = run.P, run.Ch, run.eng, run.pool
    slots = run.pick(k, in_use)
    eng.frontier_gather(pool, slots, P.box[0], P.box[1], P.mask, P.lb, P.ub, P.lb32, P.ub32, P.alpha, P.beta, P.amb)
    run._score_parents(k)
    eng.strong_list(pool, slots, P.amb, P.scores, d, run.cand0, run.cand_row, run.cand_slot, run.cand_dec, workspace=run.ws_strong)
    eng.frontier_expand_depth(pool, slots, d, run.cand0, run.cand_dec, Ch.mask, Ch.plb, Ch.pub, Ch.split, Ch.alpha, Ch.beta, Ch.live)
    run._bound_children(Ch, k * Cn, warm=True)
    outs = lambda: [Ch.bound, Ch.infeasible, Ch.alpha, Ch.beta, Ch.ubv, Ch.x_lp] + Ch.lb + Ch.ub      # noqa: E731
    got = [t[:k * Cn].clone() for t in outs()]
    live = Ch.live[:k * Cn].cpu().tolist()
    c0 = run.cand0[:k + 1].cpu().tolist()
    dec, off = run.cand_dec[:c0[-1]].cpu().tolist(), T.offsets(eng.sizes)
    rows = []
    for i in range(k):
        nodes = dec[c0[i]:c0[i + 1]]
        assert 1 <= len(nodes) <= d
        for j in range(2 ** len(nodes)):
            rows.append((Cn * i + j, int(slots[i]), [(off[lay] + idx, (j >> b) & 1) for b, (lay, idx) in enumerate(nodes)], min(lay for lay, _ in nodes)))
    assert [c for c, *_ in rows] == [c for c in range(k * Cn) if live[c]] and len(rows) >= 6
    order = list(reversed(rows))
    for r, (c, s, sets, lay) in enumerate(order):
        Ch.mask[r] = pool.mask[s]
        for node, bit in sets:
            Ch.mask[r, node] = bit
        Ch.alpha[r], Ch.beta[r], Ch.split[r] = pool.alpha[s], pool.beta[s], lay
        for a, b in zip(Ch.plb + Ch.pub, pool.lb + pool.ub):
            a[r] = b[s]
    run._bound_children(Ch, len(order), warm=True)
    for r, (c, *_) in enumerate(order):
        for a, b in zip(outs(), got):
            assert same(a[r], b[c]), (r, c)
    run.check_status()


# ---- 5. whole runs on toy_kw -------------------------------------------------------------------------------------------------------------------
_shared = {}


def depth_run(D, K, rounds, capacity=None):
    """``branch_and_bound_frontier`` on toy_kw at ``lp.split_depth`` = D with its trace and every record its own loop reads (the root's first)."""
    key = (D, K, rounds, capacity)
    if key not in _shared:
        lp, choice, _ = toy()
        trace = []
        with recorded() as records, split_depth(lp, D):
            res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=capacity,
                                            log=lambda s: None, trace=trace)
        _shared[key] = (res, records, trace)
    return _shared[key]


def test_split_depth_1_is_the_run_without_it():
    res0, records0, trace0 = depth_run(None, 4, 3)
    res1, records1, trace1 = depth_run(1, 4, 3)
    assert res1 == res0 and records1 == records0 and len(trace1) == len(trace0) >= 2
    for a, b in zip(trace0, trace1):
        assert "depth" not in a and b["depth"] == 1
        assert {k: v for k, v in b.items() if k not in ("depth", "nodes")} == a      # decisions, bounds, upper values, flags: Python floats of the same values
        assert b["nodes"] == [[dec] if dec[0] >= 0 else [] for dec in a["decisions"]]      # the list's first-ranked node is gnnb_forward's own decision


def host_loop(K, D, rounds, cap):
    """The depth run as a host loop: the twins (depth, nodes, expand, commit) around the EXISTING batch entry points, which a run without
    split_depth supplies -- its gather, its gnnb_dual_ascent at n_iter 0 and gnnb_forward, its gnnb_kw_bounds / gnnb_dual_ascent /
    gnnb_net_eval on child rows.  The pool crosses the link every round."""
    lp, choice, _ = toy()
    ref = FrontierRun(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, capacity=cap)
    st = ref.root()
    eng, P, Ch, sizes = ref.eng, ref.P, ref.Ch, ref.eng.sizes
    out = {"decisions": [], "nodes": [], "child_bounds": [], "depth": [], "records": [st]}
    for r in range(rounds):
        glb = min(st[S.FS_LOWEST_OPEN], st[S.FS_CLOSED_LB], st[S.FS_GLOBAL_UB])
        n_open, in_use = int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
        if n_open == 0 or not st[S.FS_GLOBAL_UB] - glb > EPS_BAB:
            break
        k = min(K, n_open)
        d = T.depth_of_round(k, K, D, n_open, cap)
        assert d >= 1
        Cn, pool = 2 ** d, ref.pool
        if in_use + (Cn - 1) * k > cap:
            pool.compact(n_open)
            st[S.FS_IN_USE], in_use = float(n_open), n_open
        slots = ref.pick(k, in_use)
        eng.frontier_gather(pool, slots, P.box[0], P.box[1], P.mask, P.lb, P.ub, P.lb32, P.ub32, P.alpha, P.beta, P.amb)
        ref._score_parents(k)
        scores, amb, sl = P.scores[:k].cpu(), P.amb[:k].cpu(), slots.cpu().tolist()
        nodes = [T.top_nodes(scores[i], amb[i] != 0, d, sizes) for i in range(k)]
        cand0, cand_dec = [0], []
        for ns in nodes:
            cand_dec += ns
            cand0.append(len(cand_dec))
        hp, n = pool_to_host(pool), Cn * k
        rows = {"mask": Ch.mask[:n].cpu(), "plb": [t[:n].cpu() for t in Ch.plb], "pub": [t[:n].cpu() for t in Ch.pub], "split": Ch.split[:n].cpu(),
                "alpha": Ch.alpha[:n].cpu(), "beta": Ch.beta[:n].cpu(), "live": Ch.live[:n].cpu()}
        T.expand(hp, sl, d, cand0, cand_dec, sizes, rows)
        for dst, src in zip([Ch.mask, Ch.split, Ch.alpha, Ch.beta, Ch.live] + Ch.plb + Ch.pub,
                            [rows["mask"], rows["split"], rows["alpha"], rows["beta"], rows["live"]] + rows["plb"] + rows["pub"]):
            dst[:n] = src.to(eng.device)
        ref._bound_children(Ch, n, warm=True)
        parent = hp["bound"][torch.tensor(sl)].repeat_interleave(Cn)
        ch = {"mask": Ch.mask[:n].cpu(), "lb": [t[:n].cpu() for t in Ch.lb], "ub": [t[:n].cpu() for t in Ch.ub], "infeasible": Ch.infeasible[:n].cpu(),
              "bound": torch.maximum(Ch.bound[:n].cpu(), parent), "alpha": Ch.alpha[:n].cpu(), "beta": Ch.beta[:n].cpu(), "ub_value": Ch.ubv[:n].cpu(),
              "live": rows["live"]}
        st = T.commit(hp, st, sl, Cn, ch, EPS_BAB, None, sizes)
        for dst, src in zip([pool.mask, pool.alpha, pool.beta, pool.bound, pool.open] + pool.lb + pool.ub,
                            [hp["mask"], hp["alpha"], hp["beta"], hp["bound"], hp["open"]] + hp["lb"] + hp["ub"]):
            dst.copy_(src)
        pool.state.copy_(torch.tensor(st, dtype=torch.float64))
        out["decisions"].append(P.dec[:k].cpu().tolist())
        out["nodes"].append(nodes)
        out["depth"].append(d)
        out["child_bounds"].append(masked(ch["bound"].tolist(), ch["infeasible"].tolist(), ch["live"].tolist()))
        out["records"].append(st)
    ref.check_status()
    return out


def test_split_depth_3_equals_the_host_loop_of_the_twins():
    (glb, gub, rounds, bounded, reason), records, trace = depth_run(3, 4, 3, 64)
    want = host_loop(4, 3, 3, 64)
    print("twin", {k: want[k] for k in ("depth", "decisions", "nodes")}, "frontier", (glb, gub, rounds, bounded, reason))
    assert rounds == len(want["depth"]) >= 2 and max(want["depth"]) == 3
    assert [t["depth"] for t in trace] == want["depth"]
    assert [t["decisions"] for t in trace] == want["decisions"]
    assert [t["nodes"] for t in trace] == want["nodes"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == want["child_bounds"]      # bit for bit
    last = want["records"][-1]
    assert glb == min(last[S.FS_LOWEST_OPEN], last[S.FS_CLOSED_LB], last[S.FS_GLOBAL_UB])
    assert abs(gub - last[S.FS_GLOBAL_UB]) <= 1e-9 * max(1.0, abs(last[S.FS_GLOBAL_UB]))
    for a, b in zip(records, want["records"]):                    # open domains, slots in use, kept / closed / infeasible / dropped
        assert a[S.FS_N_OPEN:] == b[S.FS_N_OPEN:] and a[S.FS_CLOSED_LB] == b[S.FS_CLOSED_LB] and a[S.FS_LOWEST_OPEN] == b[S.FS_LOWEST_OPEN]
    assert bounded == 1 + sum(int(st[S.FS_KEPT] + st[S.FS_CLOSED] + st[S.FS_INFEASIBLE]) for st in records[1:])


@pytest.mark.parametrize("D,K,capacity", [(3, 4, 64), (2, 2, None), (8, 4, 12)])
def test_every_round_runs_at_round_depth_of_the_record_before_it(D, K, capacity):
    res, records, trace = depth_run(D, K, 3, capacity)
    cap = max(1024, 4 * K + 1) if capacity is None else capacity
    assert len(records) == len(trace) + 1 >= 2
    for st, t in zip(records, trace):
        k = len(t["slots"])
        assert k == min(K, int(st[S.FS_N_OPEN]))
        d = frontier.round_depth(k, K, D, int(st[S.FS_N_OPEN]), cap)
        assert t["depth"] == d >= 1 and len(t["live"]) == k << d and len(t["nodes"]) == k
        assert all(len(ns) <= d for ns in t["nodes"])
    for st in records:
        assert st[S.FS_OVERFLOW] == 0 and st[S.FS_IN_USE] <= cap
    assert res[4] in ("max_rounds", "capacity", "gap", "exhausted")


def test_round_1_fills_the_child_rows():
    """The root of toy_kw has far more than 3 undecided nodes: round 1 of a D = 3, K = 4 run bounds min(2^D, 2K) = 8 live rows, and of a
    D = 8, K = 4 run 8 as well (2K caps the depth at 3)."""
    for D in (3, 8):
        _, records, trace = depth_run(D, 4, 3, 64 if D == 3 else 12)
        t = trace[0]
        assert t["depth"] == 3 and len(t["nodes"][0]) == 3 and t["live"] == [1] * 8
        assert records[1][S.FS_KEPT] + records[1][S.FS_CLOSED] + records[1][S.FS_INFEASIBLE] == 8


# ---- 6. soundness against certified minima ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,D", [("gnn_k16", 4), ("gnn_pgd", 2)])
@pytest.mark.parametrize("case", CASES)
def test_depth_runs_keep_the_sandwich_around_the_exact_minimum(case, mode, D):
    """``check_run`` holds every record to the sandwich, the witness to what it claims and the verdicts to the truth; no convergence asserted."""
    with split_depth(case_lp(case), D):                           # (``run_case`` runs on this cached root)
        # (the mode's own budget, named: ``run_case`` keeps the records of a run without arguments for the tests of its module)
        res, records, trace, witness = run_case(case, mode, max_rounds=max(1, BRANCHES // MODES[mode][0]))
    assert res[4] != "decision" and all("depth" in t for t in trace)


# ---- 7. device residency ------------------------------------------------------------------------------------------------------------------------
def test_a_depth_round_copies_nothing_but_the_state_record():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy()
    run = depth_frontier_run(lp, choice, 3, K=4)
    st = run.root()
    before = torch.cuda.get_sync_debug_mode()
    depths = []
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
            k = min(4, n_open)
            depths.append(frontier.round_depth(k, 4, 3, n_open, run.capacity))
            torch.cuda.set_sync_debug_mode("error")
            run.launch_round(k, in_use, depths[-1])
            with pytest.raises(RuntimeError):             # the mode is live: the state read is a synchronising copy
                run.read_state()
            torch.cuda.set_sync_debug_mode(before)        # the explicit exemption
            st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert depths[0] == 3 and st[S.FS_KEPT] + st[S.FS_CLOSED] + st[S.FS_INFEASIBLE] >= 2
    run.check_status()


# ---- 8. limits ---------------------------------------------------------------------------------------------------------------------------------
def test_limits(engine):
    """depth 0 and 9, kwg_over, an unbound handle and a workspace one byte short are refused before a launch with the entry point's name,
    and the handle stays usable."""
    from gnn_branching_amd.engine import ScorerEngine
    dev = engine.device
    fresh = ScorerEngine(None)
    pool_s, ch_s = _lib.Pool(), _lib.Children()
    assert fresh.lib.gnnb_frontier_expand_depth(fresh.h, C.byref(pool_s), None, 1, 1, None, None, None, None, None, None, None, None, None, None) == -3
    assert b"gnnb_frontier_expand_depth" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_commit_depth(fresh.h, C.byref(pool_s), None, 1, 1, C.byref(ch_s), 1e-4, 0.0, None, None, 0, None) == -3
    assert b"gnnb_frontier_commit_depth" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_commit_depth_workspace_bytes(fresh.h, 1, 1) == 0

    def buffers(n):
        R = engine.R
        layer = lambda: [torch.zeros(n, s, dtype=torch.float64, device=dev) for s in engine.sizes[1:]]      # noqa: E731
        i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)                                           # noqa: E731
        return {"mask": torch.zeros(n, R, dtype=torch.int8, device=dev), "lb": layer(), "ub": layer(), "alpha": torch.zeros(n, R, dtype=torch.float64, device=dev),
                "beta": torch.zeros(n, R, dtype=torch.float64, device=dev), "split": i32(), "live": i32(), "infeasible": i32(),
                "bound": torch.zeros(n, dtype=torch.float64, device=dev)}

    def expand(pool, depth, b):
        sl, c0, cd = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.zeros(1, 2, dtype=torch.int32, device=dev)
        engine.frontier_expand_depth(pool, sl, depth, c0, cd, b["mask"], b["lb"], b["ub"], b["split"], b["alpha"], b["beta"], b["live"])

    def commit(pool, depth, b, **kw):
        sl = torch.zeros(1, dtype=torch.int32, device=dev)
        engine.frontier_commit_depth(pool, sl, depth, b["mask"], b["lb"], b["ub"], b["infeasible"], b["bound"], b["alpha"], b["beta"], b["bound"], b["live"],
                                     pool.state, **kw)

    over = Net("kwg_over")
    engine.bind(over.fixed, tuple(over.shape))
    pool, b = DomainPool(engine, 3), buffers(2)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_expand_depth failed \(-1\).*4097 nodes"):
        expand(pool, 1, b)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit_depth failed \(-1\).*4097 nodes"):
        commit(pool, 1, b, workspace=torch.empty(1 << 16, dtype=torch.uint8, device=dev))

    # the handle stays usable: a network within the cap, then the depths outside 1..8, too many rows, the short workspace
    net = Net("kwg_mlp")
    pool = random_pool(engine, net, 8, 31)
    pool.state.copy_(torch.tensor([1.0, INF, INF, 8.0, 8.0, 0, 0, 0, 0], dtype=torch.float64))
    b = buffers(256)
    before = snapshot(pool)
    for depth in (0, 9):
        with pytest.raises(RuntimeError, match=rf"gnnb_frontier_expand_depth failed \(-1\).*depth = {depth}"):
            expand(pool, depth, b)
        with pytest.raises(RuntimeError, match=rf"gnnb_frontier_commit_depth failed \(-1\).*depth = {depth}"):
            commit(pool, depth, b, workspace=torch.empty(1 << 16, dtype=torch.uint8, device=dev))
        assert engine.lib.gnnb_frontier_commit_depth_workspace_bytes(engine.h, 1, depth) == 0
    st, keep = engine._pool(pool)                                # (keep: the pointer tables the struct names)
    assert engine.lib.gnnb_frontier_expand_depth(engine.h, C.byref(st), None, 32767, 2, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"gnnb_frontier_expand_depth" in engine.lib.gnnb_last_error() and b"65534" in engine.lib.gnnb_last_error()
    assert engine.lib.gnnb_frontier_commit_depth(engine.h, C.byref(st), None, 256, 8, C.byref(ch_s), 1e-4, 0.0, None, None, 0, None) == -1
    assert b"gnnb_frontier_commit_depth" in engine.lib.gnnb_last_error() and b"65534" in engine.lib.gnnb_last_error()
    assert engine.lib.gnnb_frontier_commit_depth_workspace_bytes(engine.h, 256, 8) == 0
    need = engine.lib.gnnb_frontier_commit_depth_workspace_bytes(engine.h, 1, 3)
    assert need > 0 and need == engine.lib.gnnb_frontier_commit_workspace_bytes(engine.h, 4)      # 8 child rows either way
    b["live"][:8] = 1
    b["bound"][:8] = -1.0
    b["mask"][:8] = -1
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit_depth failed \(-4\)"):
        commit(pool, 3, b, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    for x, y in zip(before, snapshot(pool)):
        assert torch.equal(x, y)
    assert math.isinf(float(pool.state[S.FS_CLOSED_LB]))
    expand(pool, 3, b)                                            # ... and both run once the arguments are right
    assert b["live"][:8].cpu().tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and int(b["split"][0]) == 0
    commit(pool, 3, b, workspace=torch.empty(need, dtype=torch.uint8, device=dev))
    assert float(pool.state[S.FS_KEPT]) + float(pool.state[S.FS_CLOSED]) == 2.0
