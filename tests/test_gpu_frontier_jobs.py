"""Many verification jobs in one device-resident frontier on the MI355X (gnn_branching_amd/frontier.py verify_properties;
csrc/gnnb_k_frontier.h k_frontier_pick_jobs / _rows_jobs / _decide_jobs).  Every comparison is exact.

1. gnnb_frontier_pick_jobs against ``FrontierRun.pick``'s expression on the segment's slice;
2. gnnb_frontier_rows_jobs against torch indexing;
3. gnnb_frontier_commit_jobs against the existing gnnb_frontier_commit, called once per entry on a view of the segment;
4. the defining property: every job of ``verify_properties`` gets the result and the per-round trace ``branch_and_bound_frontier`` gives
   it alone, for two segment counts and two segment sizes;
5. per-segment compaction against ``DomainPool.compact``'s rule; 6. a round copies nothing but the records; 7. the limits."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, lp_producer, nets
from gnn_branching_amd.frontier import DomainPool, FrontierJob, JobsRun, RoundPlan, branch_and_bound_frontier, plan_round, verify_properties
from tests.test_gpu_frontier import engine, poisoned, random_pool, six_children, snapshot, toy   # noqa: F401  (engine: the module's fixture)
from tests.test_gpu_kw_geometry import Net, seeded_domain

pytestmark = pytest.mark.gpu

S = _lib
INF = float("inf")
NAN = float("nan")


def records(dev, rows):
    """(segments, 9) records on the device from (global_ub, n_open, in_use) per segment; closed_lb and the lowest open bound +inf."""
    return torch.tensor([[gub, INF, INF, float(n_open), float(in_use), 0.0, 0.0, 0.0, 0.0] for gub, n_open, in_use in rows], dtype=torch.float64).to(dev)


def sent(dev, entries, segments, cap):
    plan = RoundPlan(dev, len(entries), segments, cap)
    plan.send(entries)
    return plan


# ---- 1. pick ------------------------------------------------------------------------------------------------------------------------
def test_pick_against_the_stable_sort_of_the_segment(engine):
    """kwg_mlp, 4 segments of 700 slots.  Segment 0 (in_use 40): k = 1; segment 2 (in_use 300): k = its open count, its two lowest open
    bounds EQUAL (slots 170 and 31: the lower slot first); segment 3 (in_use 650: more slots than threads): k = 130, more picks than half
    a workgroup.  In every segment closed slots hold the lowest bounds, and open = 1 garbage with a lower bound still sits above in_use."""
    net, cap, nseg = Net("kwg_mlp"), 700, 4
    pool = random_pool(engine, net, nseg * cap, 51)
    dev = engine.device
    g = torch.Generator().manual_seed(52)
    in_use = [40, 123, 300, 650]
    opn = (torch.rand(nseg * cap, generator=g) < 0.5).to(torch.int32)
    bound = torch.randn(nseg * cap, generator=g, dtype=torch.float64)
    for s in range(nseg):
        b = s * cap
        closed = torch.nonzero(opn[b:b + in_use[s]] == 0).reshape(-1)[:5] + b
        bound[closed] = -50.0 - torch.arange(len(closed), dtype=torch.float64)      # closed slots with the lowest bounds
        opn[b + in_use[s]:b + cap] = 1                                             # garbage above in_use
        bound[b + in_use[s]:b + cap] = -99.0
    opn[2 * cap + 170] = opn[2 * cap + 31] = 1
    bound[2 * cap + 170] = bound[2 * cap + 31] = -7.5                              # a tie between the two lowest open bounds
    pool.open.copy_(opn)
    pool.bound.copy_(bound)
    n_open = [int(opn[s * cap:s * cap + in_use[s]].sum()) for s in range(nseg)]
    assert n_open[2] > 100 and n_open[3] >= 130
    state = records(dev, [(1.0, n_open[s], in_use[s]) for s in range(nseg)])
    before = snapshot(pool)

    def want(seg, k):                                         # FrontierRun.pick's expression on the segment's slice, plus its first slot
        b = seg * cap
        key = torch.where(pool.open[b:b + in_use[seg]] > 0, pool.bound[b:b + in_use[seg]], float("inf"))
        return torch.sort(key, stable=True).indices[:k].to(torch.int32) + b

    def run(entries):
        n = sum(e[2] for e in entries)
        slots, row_seg = torch.full((n + 3,), 77, dtype=torch.int32, device=dev), torch.full((n + 3,), 77, dtype=torch.int32, device=dev)
        engine.frontier_pick_jobs(pool, sent(dev, entries, nseg, cap), state, slots, row_seg)
        for seg, row0, k in entries:
            assert torch.equal(slots[row0:row0 + k], want(seg, k)), (seg, k)
            assert bool((row_seg[row0:row0 + k] == seg).all())
        assert bool((slots[n:] == 77).all()) and bool((row_seg[n:] == 77).all())
        return slots

    k2 = n_open[2]
    slots = run([(0, 0, 1), (2, 1, k2), (3, 1 + k2, 130)])
    assert slots[1:3].cpu().tolist() == [2 * cap + 31, 2 * cap + 170]              # the tie went by slot
    assert bool((pool.open[slots[:1 + k2 + 130].long()] == 1).all())               # no closed slot, nothing above in_use
    # neither the number of entries nor their order matters: each entry alone, and the segments in another order
    for e in ([(0, 0, 1)], [(2, 0, k2)], [(3, 0, 130)], [(3, 0, 130), (0, 130, 1), (2, 131, k2)]):
        run(e)
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a, b)


# ---- 2. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
def test_rows_against_torch_indexing(name, engine):
    net = Net(name)
    engine.bind(net.fixed, tuple(net.shape))
    dev, N0, NL, nseg = engine.device, engine.sizes[0], engine.sizes[-2], 3
    g = torch.Generator().manual_seed(61)
    seg_lo, seg_hi = (torch.randn(nseg, N0, generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    seg_pw, seg_pb = torch.randn(nseg, NL, generator=g).to(dev), torch.randn(nseg, generator=g).to(dev)
    entries = [(2, 0, 1), (0, 1, 3), (1, 4, 2)]
    n = 6
    row_seg = torch.tensor([2, 0, 0, 0, 1, 1], dtype=torch.int32, device=dev)
    f64, f32 = torch.float64, torch.float32
    out = [poisoned(r, c, dt, dev) for r in (n + 1, 2 * n + 1) for c, dt in ((N0, f64), (N0, f64), (NL, f32), (1, f32))]
    engine.frontier_rows_jobs(sent(dev, entries, nseg, 5), row_seg, seg_lo, seg_hi, seg_pw, seg_pb, *out)
    idx = row_seg.long()
    for rows, (x_lo, x_hi, pw, pb), ix in ((n, out[:4], idx), (2 * n, out[4:], idx.repeat_interleave(2))):      # child c belongs to parent c >> 1
        assert torch.equal(x_lo[:rows], seg_lo[ix]) and torch.equal(x_hi[:rows], seg_hi[ix])
        assert torch.equal(pw[:rows], seg_pw[ix]) and torch.equal(pb[:rows, 0], seg_pb[ix])
        for t in (x_lo, x_hi, pw, pb):
            assert bool(torch.isnan(t[rows]).all())           # the row past the last one is as it was


# ---- 3. commit ----------------------------------------------------------------------------------------------------------------------
def random_children(sizes, R, n, seed):
    """n children with random masks, bounds astride 0 (so nearly every child has an undecided node), values above the incumbent 1.0 and
    bounds around 0: most live feasible children are kept."""
    g = torch.Generator().manual_seed(seed)
    return {"mask": torch.randint(-1, 2, (n, R), generator=g).to(torch.int8),
            "lb": [-torch.rand(n, s, generator=g, dtype=torch.float64) - 0.1 for s in sizes[1:]],
            "ub": [torch.rand(n, s, generator=g, dtype=torch.float64) + 0.1 for s in sizes[1:]],
            "infeasible": (torch.rand(n, generator=g) < 0.1).to(torch.int32), "live": (torch.rand(n, generator=g) < 0.9).to(torch.int32),
            "bound": torch.randn(n, generator=g, dtype=torch.float64), "ub_value": torch.rand(n, generator=g, dtype=torch.float64) + 2.0,
            "alpha": torch.rand(n, R, generator=g, dtype=torch.float64), "beta": torch.rand(n, R, generator=g, dtype=torch.float64)}


def segment_view(arrays, seg, cap):
    """The segment's slices of a pool's arrays (``DomainPool.arrays()`` order) as a pool of ``cap`` slots: writes land in the arrays."""
    sl = [t[seg * cap:(seg + 1) * cap] for t in arrays]
    L1 = (len(sl) - 5) // 2
    return types.SimpleNamespace(capacity=cap, mask=sl[0], lb=sl[1:1 + L1], ub=sl[1 + L1:1 + 2 * L1], alpha=sl[-4], beta=sl[-3], bound=sl[-2], open=sl[-1])


@pytest.mark.parametrize("bounds", [[NAN] * 6, [0.1, 0.3, NAN, NAN, -5.0, 0.0]], ids=["no_decision_bound", "mixed_decision_bounds"])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_commit_against_the_one_job_commit_per_entry(name, bounds, engine):
    """6 segments of 300 slots, entries on segments 0 (k = 3: the six kinds of children), 2 (k = 1, the segment full: its second kept
    child finds no slot) and 5 (k = 130: 2k exceeds the workgroup's 256 threads, kept children beyond the parents' slots)."""
    net, cap, nseg, eps = Net(name), 300, 6, 1e-4
    pool = random_pool(engine, net, nseg * cap, 71)
    dev, sizes, R = engine.device, engine.sizes, engine.R
    six, rnd = six_children(sizes, R, 21, eps), random_children(sizes, R, 260, 72)
    parts = [six, {k: ([t[[3, 5]] for t in v] if isinstance(v, list) else v[[3, 5]]) for k, v in six.items()}, rnd]
    ch = {k: ([torch.cat([p[k][i] for p in parts]).to(dev) for i in range(len(six[k]))] if isinstance(six[k], list)
              else torch.cat([p[k] for p in parts]).to(dev)) for k in six}
    entries = [(0, 0, 3), (2, 3, 1), (5, 4, 130)]
    n = 134
    g = torch.Generator().manual_seed(73)
    parents = [torch.tensor([5, 0, 3]), torch.tensor([290]), torch.randperm(150, generator=g)[:130]]
    slots = torch.cat([p + seg * cap for p, (seg, _, _) in zip(parents, entries)]).to(torch.int32).to(dev)
    opn = (torch.rand(nseg * cap, generator=g) < 0.3).to(torch.int32)
    opn[5 * cap + 150:6 * cap] = 0
    opn[slots.cpu().long()] = 1
    pool.open.copy_(opn)
    in_use = [6, 17, cap, 0, 40, 150]
    state = records(dev, [(1.0, int(opn[s * cap:s * cap + in_use[s]].sum()), in_use[s]) for s in range(nseg)])
    table = torch.tensor(bounds, dtype=torch.float64).to(dev)
    before, state_before = snapshot(pool), state.clone()
    # the yardstick: the existing commit per entry on a copy, through a view of the segment with segment-relative slots
    want, want_state = snapshot(pool), state.clone()
    for seg, row0, k in entries:
        c = slice(2 * row0, 2 * row0 + 2 * k)
        engine.frontier_commit(segment_view(want, seg, cap), slots[row0:row0 + k] - seg * cap, ch["mask"][c], [t[c] for t in ch["lb"]],
                               [t[c] for t in ch["ub"]], ch["infeasible"][c], ch["bound"][c], ch["alpha"][c], ch["beta"][c], ch["ub_value"][c],
                               ch["live"][c], want_state[seg], eps=eps, decision_bound=None if math.isnan(bounds[seg]) else bounds[seg])
    engine.frontier_commit_jobs(pool, sent(dev, entries, nseg, cap), slots, ch["mask"], ch["lb"], ch["ub"], ch["infeasible"], ch["bound"], ch["alpha"],
                                ch["beta"], ch["ub_value"], ch["live"], state, table, eps=eps)
    print("records", state.cpu().tolist())
    assert torch.equal(state, want_state)
    for a, b in zip(snapshot(pool), want):
        assert torch.equal(a, b)
    for seg in (1, 3, 4):                                     # took no part: bit-identical, records included
        assert torch.equal(state[seg], state_before[seg])
        for a, b in zip(snapshot(pool), before):
            assert torch.equal(a[seg * cap:(seg + 1) * cap], b[seg * cap:(seg + 1) * cap])
    st = state.cpu().tolist()
    # the test's own conditions: the full segment overflowed, the big entry kept more children than it has parents
    assert st[2][S.FS_OVERFLOW] == 1 and st[2][S.FS_KEPT] == 1 and st[0][S.FS_OVERFLOW] == 0 and st[5][S.FS_OVERFLOW] == 0
    assert st[5][S.FS_KEPT] > 130 or not math.isnan(bounds[5])
    assert st[5][S.FS_IN_USE] == 150 + max(0, st[5][S.FS_KEPT] - 130)
    assert st[0][S.FS_KEPT] == (2 if math.isnan(bounds[0]) else 1) and st[0][S.FS_INFEASIBLE] == 1


# ---- 4. the defining property ---------------------------------------------------------------------------------------------------------
K, N_ITER, LR, EPS_BAB, ROUNDS = 2, 20, 0.1, 1e-4, 3
# (x seed, class, box eps, decision bound) on toy_kw (ground truth 2).  The first five branch through every round; the sixth has an upper
# value below 0 at its root ("decision" there); the seventh has no ambiguous ReLU and closes at its root.
JOBS = [(9, 6, 0.04, None), (9, 3, 0.04, None), (10, 1, 0.04, None), (11, 5, 0.02, 0.0), (12, 7, 0.04, 0.0), (9, 6, 0.04, 0.0), (9, 6, 1e-6, None)]
_shared = {}


def toy_jobs():
    if "jobs" not in _shared:
        _, choice, _ = toy()
        lps = []
        for seed, cls, eps, _ in JOBS:
            layers = nets.load_verified_net("toy_kw", 2, cls)
            x = torch.from_numpy(np.random.RandomState(seed).standard_normal((3, 32, 32)).astype(np.float32))
            lps.append(lp_producer.LayerGraphLP(layers, x - eps, x + eps, bounds="kw_device", engine=choice.model.engine()))
        _shared["jobs"] = (choice, lps)
    return _shared["jobs"]


def alone(cap):
    """Every job through the existing one-job loop with capacity = cap: [(result, trace)], and how often a pool was compacted."""
    if ("alone", cap) not in _shared:
        choice, lps = toy_jobs()
        compactions, orig = [], DomainPool.compact

        def counting(self, n_open):
            compactions.append(n_open)
            return orig(self, n_open)
        DomainPool.compact = counting
        try:
            out = []
            for lp, (_, _, _, db) in zip(lps, JOBS):
                trace = []
                res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, decision_bound=db,
                                                capacity=cap, log=lambda s: None, trace=trace)
                out.append((res, trace))
        finally:
            DomainPool.compact = orig
        _shared[("alone", cap)] = (out, len(compactions))
    return _shared[("alone", cap)]


@pytest.mark.parametrize("segments", [3, 7])
@pytest.mark.parametrize("cap", [9, 5])
def test_every_job_gets_the_result_it_gets_alone(cap, segments):
    """Seven jobs in 3 segments (two admission waves, a segment reused after a root-only job, jobs that start in different iterations) and
    in 7: the five-tuple and the per-round traces of every job equal the one-job loop's with capacity = cap, bit for bit.

    cap = 9 is the setting's; with K = 2 and three rounds a pool never holds more than 6 slots in use (1, 2, 4, 6), so no one-job run
    compacts or stops for capacity at any cap above 2K + 1 = 5.  At cap = 5 a job that keeps all four children of its second round stops
    there ("capacity": 4 + 2 > 5), which is the condition asserted below for that value."""
    choice, lps = toy_jobs()
    single, compactions = alone(cap)
    for (res, trace), job in zip(single, JOBS):
        print("alone", job, res)
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], db) for lp, (_, _, _, db) in zip(lps, JOBS)]
    trace = []
    got = verify_properties(choice, lps[0].layers[:-1], jobs, K=K, segments=segments, capacity=cap, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS,
                            log=lambda s: None, trace=trace)
    for j, ((res, one), g) in enumerate(zip(single, got)):
        print("job", j, "together", g)
        assert g == res, (j, g, res)                          # floats by ==
        mine = sorted((t for t in trace if t["job"] == j), key=lambda t: t["round"])
        assert [t["round"] for t in mine] == list(range(len(one)))
        for a, b in zip(mine, one):
            for key in ("parent_bounds", "decisions", "child_bounds", "child_ub", "live", "infeasible"):
                assert a[key] == b[key], (j, a["round"], key)
            assert [s - a["segment"] * cap for s in a["slots"]] == b["slots"], (j, a["round"])
    # the test's own conditions
    assert all(res[3] >= 7 for res, _ in single[:5]), [res for res, _ in single[:5]]
    if cap == 5:
        assert compactions > 0 or any(res[4] == "capacity" for res, _ in single), [res for res, _ in single]
    assert single[5][0][4] == "decision" and single[5][0][2] == 0 and single[6][0][4] == "exhausted" and single[6][0][2] == 0
    if segments == 3:                                          # the root-only jobs 5 and 6 both sat in one segment, one after the other
        assert len({t["segment"] for t in trace}) == 3 and {t["job"] for t in trace} == {0, 1, 2, 3, 4}


# ---- 5. compaction --------------------------------------------------------------------------------------------------------------------
def test_compaction_inside_the_flagged_segments_only():
    """``DomainPool.compact``'s rule per flagged segment -- open slots to the front in slot order, slots in use = the open count -- and the
    segments not flagged bit-identical, against torch indexing."""
    choice, lps = toy_jobs()
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps[:3]]
    cap = 7
    run = JobsRun(choice, lps[0].layers[:-1], jobs, tuple(lps[0].input_lb.shape), 2, 3, cap, N_ITER, LR, EPS_BAB)
    pool, g = run.pool, torch.Generator().manual_seed(81)
    for t in pool.lb + pool.ub + [pool.alpha, pool.beta, pool.bound]:
        t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64))
    pool.mask.copy_(torch.randint(-1, 2, pool.mask.shape, generator=g).to(torch.int8))
    flags = [[1, 0, 1, 1, 0, 0, 1], [0, 1, 0, 1, 1, 0, 0], [0, 0, 1, 0, 1, 1, 1]]
    pool.open.copy_(torch.tensor(flags, dtype=torch.int32).reshape(-1))
    pool.state.copy_(records(run.eng.device, [(1.0, 4, 7), (1.0, 3, 5), (1.0, 4, 7)]))
    before = snapshot(pool)
    run.compact([True, False, True])
    after = snapshot(pool)
    assert pool.state[:, S.FS_IN_USE].cpu().tolist() == [4.0, 5.0, 4.0]
    assert pool.open.cpu().tolist() == [1, 1, 1, 1, 0, 0, 0] + flags[1] + [1, 1, 1, 1, 0, 0, 0]
    for seg, keep in ((0, [0, 2, 3, 6]), (2, [2, 4, 5, 6])):
        idx = torch.tensor(keep, device=run.eng.device) + seg * cap
        for a, b in zip(before, after):
            assert torch.equal(a[idx], b[seg * cap:seg * cap + 4]) and b.is_contiguous()
    for a, b in zip(before, after):
        assert torch.equal(a[cap:2 * cap], b[cap:2 * cap])


# ---- 6. device residency --------------------------------------------------------------------------------------------------------------
def test_a_round_of_three_segments_copies_nothing_but_the_records():
    """As tests/test_gpu_frontier.py: with the sync debug mode at "error" every synchronising call of torch raises; planning (host only),
    the plan's non_blocking copy and the round's launches run under it, the read of the records is the one exemption."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    choice, lps = toy_jobs()
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps[:3]]
    run = JobsRun(choice, lps[0].layers[:-1], jobs, tuple(lps[0].input_lb.shape), K, 3, 9, N_ITER, LR, EPS_BAB)
    for s in range(3):
        run.admit(s, s)
    run.launch_roots([0, 1, 2])
    st = run.read_state()
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
            assert all(r[S.FS_N_OPEN] >= 1 for r in st)
            torch.cuda.set_sync_debug_mode("error")
            entries, compact, stopped = plan_round(st, K, 9)
            assert len(entries) == 3 and not stopped
            run.compact([True, False, True])                  # (moves nothing the rule would not: exercised here for its copies only)
            run.launch_round(entries)
            with pytest.raises(RuntimeError):                 # the mode is live: the read of the records is a synchronising copy
                run.read_state()
            torch.cuda.set_sync_debug_mode(before)            # the explicit exemption
            st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(r[S.FS_KEPT] + r[S.FS_CLOSED] + r[S.FS_INFEASIBLE] >= 2 for r in st)
    run.check_status()


# ---- 7. limits ------------------------------------------------------------------------------------------------------------------------
def job_arrays(engine, pool_slots, nseg, n):
    """Zeroed arguments of the three entry points for the bound network: (pool, state, table, slots, row_seg, segment tables, rows, children)."""
    dev, R, sizes = engine.device, engine.R, engine.sizes
    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    z = lambda r, c, dt: torch.zeros(r, c, dtype=dt, device=dev)       # noqa: E731
    pool = DomainPool(engine, pool_slots)
    seg = [z(nseg, sizes[0], f64), z(nseg, sizes[0], f64), z(nseg, sizes[-2], f32), z(nseg, 1, f32)]
    rows = [z(r, c, dt) for r in (n, 2 * n) for c, dt in ((sizes[0], f64), (sizes[0], f64), (sizes[-2], f32), (1, f32))]
    ch = [z(2 * n, R, torch.int8), [z(2 * n, s, f64) for s in sizes[1:]], [z(2 * n, s, f64) for s in sizes[1:]], z(2 * n, 1, i32), z(2 * n, 1, f64),
          z(2 * n, R, f64), z(2 * n, R, f64), z(2 * n, 1, f64), z(2 * n, 1, i32)]
    return pool, records(dev, [(1.0, 0, 0)] * nseg), torch.full((nseg,), NAN, dtype=f64, device=dev), z(n, 1, i32), z(n, 1, i32), seg, rows, ch


def test_limits(engine):
    """kwg_over (a 4097-node layer) is refused by the three entry points before a launch and the handle stays usable; an unbound handle
    is GNNB_E_STATE; a plan entry naming a segment outside the pool, or with k < 1, or rows that do not add up, GNNB_E_INVALID; a
    workspace one byte short GNNB_E_NOMEM with the pool unchanged."""
    from gnn_branching_amd.engine import ScorerEngine
    dev = engine.device
    fresh = ScorerEngine(None)
    host = torch.tensor([[0, 0, 1]], dtype=torch.int32)
    pl, pool_s, ch_s = _lib.Plan(host.data_ptr(), host.data_ptr(), 1, 1, 1, 8), _lib.Pool(), _lib.Children()
    assert fresh.lib.gnnb_frontier_pick_jobs(fresh.h, C.byref(pool_s), C.byref(pl), None, None, None, None) == -3
    assert b"gnnb_frontier_pick_jobs" in fresh.lib.gnnb_last_error() and b"gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_rows_jobs(fresh.h, C.byref(pl), *([None] * 14)) == -3
    assert fresh.lib.gnnb_frontier_commit_jobs(fresh.h, C.byref(pool_s), C.byref(pl), None, C.byref(ch_s), 1e-4, None, None, None, 0, None) == -3
    assert fresh.lib.gnnb_frontier_commit_jobs_workspace_bytes(fresh.h, 1) == 0

    over = Net("kwg_over")
    d = seeded_domain(over, 0)
    with pytest.raises(RuntimeError, match=r"gnnb_net_eval failed \(-1\).*4097 nodes"):      # (binds the network)
        engine.net_eval(over.fixed, [over.prop(d.gt, d.cls)], d.x_lo[None].float().to(dev))
    pool, state, table, slots, row_seg, seg, rows, ch = job_arrays(engine, 3, 1, 1)
    plan = sent(dev, [(0, 0, 1)], 1, 3)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_pick_jobs failed \(-1\).*4097 nodes"):
        engine.frontier_pick_jobs(pool, plan, state, slots, row_seg)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_rows_jobs failed \(-1\).*4097 nodes"):
        engine.frontier_rows_jobs(plan, row_seg, *seg, *rows)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit_jobs failed \(-1\).*4097 nodes"):
        engine.frontier_commit_jobs(pool, plan, slots, *ch, state, table, workspace=torch.empty(1 << 20, dtype=torch.uint8, device=dev))

    # the handle stays usable: a network within the cap, the plans that are refused, the short workspace
    net, cap, nseg = Net("kwg_mlp"), 8, 2
    engine.bind(net.fixed, tuple(net.shape))
    pool, state, table, slots, row_seg, seg, rows, ch = job_arrays(engine, nseg * cap, nseg, 3)
    pool = random_pool(engine, net, nseg * cap, 31)
    state.copy_(records(dev, [(1.0, 8, 8), (1.0, 8, 8)]))
    good = [(0, 0, 1), (1, 1, 2)]
    engine.frontier_pick_jobs(pool, sent(dev, good, nseg, cap), state, slots, row_seg)
    assert row_seg.reshape(-1).cpu().tolist() == [0, 1, 1] and all(s // cap == r for s, r in zip(slots.reshape(-1).cpu().tolist(), [0, 1, 1]))
    before = snapshot(pool)
    for bad, what in (([(0, 0, 1), (2, 1, 2)], "segment 2 outside"), ([(0, 0, 1), (-1, 1, 2)], "segment -1 outside"), ([(0, 0, 3), (1, 3, 0)], "k = 0"),
                      ([(0, 0, 1), (1, 2, 2)], "starts at row 2"), ([(0, 0, 1), (1, 1, 1)], "hold 2 rows")):
        plan = sent(dev, bad, nseg, cap)
        plan.n = 3
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_pick_jobs failed \(-1\).*" + what):
            engine.frontier_pick_jobs(pool, plan, state, slots, row_seg)
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_rows_jobs failed \(-1\).*" + what):
            engine.frontier_rows_jobs(plan, row_seg, *seg, *rows)
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit_jobs failed \(-1\).*" + what):
            engine.frontier_commit_jobs(pool, plan, slots, *ch, state, table)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_pick_jobs failed \(-1\).*3 segments of 8 slots in a pool of 16"):
        engine.frontier_pick_jobs(pool, sent(dev, good, 3, cap), records(dev, [(1.0, 8, 8)] * 3), slots, row_seg)
    need = engine.lib.gnnb_frontier_commit_jobs_workspace_bytes(engine.h, 3)
    assert need > 0
    state_before = state.clone()
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_commit_jobs failed \(-4\)"):
        engine.frontier_commit_jobs(pool, sent(dev, good, nseg, cap), slots, *ch, state, table, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    for a, b in zip(before, snapshot(pool)):
        assert torch.equal(a, b)
    assert torch.equal(state, state_before)
