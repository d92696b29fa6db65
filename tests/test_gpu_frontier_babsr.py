"""Branching on the BaBSR heuristic alone inside the device-resident frontier, on the MI355X (DESIGN.md section 7.10;
gnn_branching_amd/frontier.py ``branching="babsr"`` and ``verify_properties_babsr``; csrc/gnnb_k_frontier.h k_frontier_babsr_decide /
_decide_jobs).  Every comparison is exact unless it says otherwise.

1. gnnb_frontier_babsr_decide against plnn.kw_score_conv.decide on crafted rows that take every branch of the rule;
2. against the existing gnnb_frontier_fallback on a pool whose every row is below the branching threshold;
3. gnnb_frontier_babsr_decide_jobs against the one-job call per entry;
4. branch_and_bound_frontier(branching="babsr") on toy_kw against a host loop of public pieces (tests/frontier_babsr_twin.py);
5. the GNN is not consulted; 6. ``verify_properties_babsr`` against the runs alone; 7. branching="gnn" is the default run; 8. the limits
   that need a handle."""
import copy
import ctypes as C

import pytest
import torch

from gnn_branching_amd import _lib, bab_caller
from gnn_branching_amd.frontier import (DomainPool, FrontierJob, FrontierJobs, RoundPlan, branch_and_bound_frontier, verify_properties_babsr)
from tests.frontier_babsr_twin import DTHR, SEQ, SPARSEST, babsr_twin, crafted_rows, rule_reference
from tests.frontier_twin import CKPT, EPS_BAB, LR, N_ITER, bind, engine, masked, toy   # noqa: F401  (engine: the module's fixture)

pytestmark = pytest.mark.gpu

I32, F64, F32 = torch.int32, torch.float64, torch.float32
NET = "kwg_rect"                    # ReLU layers of 1920, 960 and 24 nodes: two wider than a workgroup's 256 threads and no multiple of them, one narrower
FORWARD_CLASSES = ("k_embed", "k_pre", "k_pre_inp", "k_conv_fwd", "k_convT_bwd", "k_dense_agg", "k_prop", "k_node_update", "k_input_update", "k_score",
                   "k_argmax", "k_gather", "k_gather_input_update", "k_classify", "k_livesum", "k_top", "k_gather_update")


def quiet(s):
    pass


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------------
def decide_on_device(engine, rows, idx, icp0, extra=1, **kw):
    """gnnb_frontier_babsr_decide on the rows ``idx``; ``extra`` rows more in every array, which must stay as they were.  Returns (decisions,
    the counter after)."""
    dev, K = engine.device, len(idx)
    pad = lambda t: torch.cat([t[idx], torch.full((extra, t.shape[1]), 3.0)]).contiguous().to(dev)      # noqa: E731
    dec = torch.full((K + extra, 2), -7, dtype=I32, device=dev)
    icp = torch.tensor([icp0], dtype=I32).to(dev)
    engine.frontier_babsr_decide(pad(rows["scores"]), pad(rows["icps"]), pad(rows["amb"]), icp, dec, K, SPARSEST, DTHR, **kw)
    dec = dec.cpu()
    assert dec[K:].tolist() == [[-7, -7]] * extra            # rows from K on are not written
    return dec[:K].tolist(), int(icp.cpu()[0])


@pytest.fixture(scope="module")
def crafted(engine):
    relu = bind(engine, NET)
    assert len(relu) >= 3 and min(relu) < 256 and any(r > 256 and r % 256 for r in relu), relu
    return relu, crafted_rows(relu)


def test_the_crafted_rows_take_the_branches_they_were_built_for(crafted):
    """The host rule alone, from the counter 0: what every kind of row decides, so that the device comparison below covers the rule."""
    relu, rows = crafted
    decs, icp, before = rule_reference(relu, rows, range(len(SEQ)), 0)
    by = {}
    for kind, d, b in zip(SEQ, decs, before):
        by.setdefault(kind, []).append((d, b))
    hi, lo = len(relu) - 1, len(relu) - 2
    assert by["score"] == [([hi, 11], 0)]
    assert by["sparsest_max"][0][0][0] == hi and by["at_threshold"][0][0][0] == hi and by["below_threshold"][0][0][0] == hi      # the order branch
    assert by["tie_layer"] == [([1, 14], 0)] and by["tie_across_hi"] == [([hi, 6], 0)] and by["tie_across_lo"] == [([lo, 6], 0)]
    assert by["tie_across_same"] == [([lo, 5], 0)]
    assert [b for _, b in by["icp0"]] == [0, 1, 2, 0, 0, 1, 2]                 # three running: the third falls to the order branch
    assert [d for d, _ in by["icp0"]] == [[0, 5], [0, 5], by["icp0"][2][0], [0, 5], [0, 5], [0, 5], by["icp0"][6][0]]
    assert by["icp0"][2][0][0] == hi and by["icp0"][6][0][0] == hi
    assert by["icp_late"] == [([1, 4], 1)] and before[SEQ.index("icp_late") + 1] == 0      # a later layer resets the counter
    assert by["popped"][0][0][0] == lo
    for kind in ("nan", "nan_icp", "no_open"):                                 # device-defined: no decision, the counter as it was (1)
        assert by[kind] == [([-1, -1], 1)], kind
    assert icp == 0


@pytest.mark.parametrize("icp0", [0, 1, 2])
def test_all_rows_in_one_call_against_decide(icp0, crafted, engine):
    relu, rows = crafted
    idx = list(range(len(SEQ)))
    want, want_icp, _ = rule_reference(relu, rows, idx, icp0)
    got, got_icp = decide_on_device(engine, rows, idx, icp0)
    print("icp0", icp0, "decisions", got, "counter", got_icp)
    assert got == want and got_icp == want_icp


def test_every_row_alone_against_decide(crafted, engine):
    """K = 1: each row from the counter the host rule had before it, and from the other two counters."""
    relu, rows = crafted
    _, _, before = rule_reference(relu, rows, range(len(SEQ)), 0)
    for i, kind in enumerate(SEQ):
        for icp0 in sorted({before[i], 0, 2}):
            want, want_icp, _ = rule_reference(relu, rows, [i], icp0)
            got, got_icp = decide_on_device(engine, rows, [i], icp0)
            assert got == want and got_icp == want_icp, (kind, i, icp0, got, want, got_icp, want_icp)


@pytest.mark.parametrize("cut", [9, 10, 16])
def test_two_calls_that_carry_the_counter_equal_one(cut, crafted, engine):
    """Split inside the run of three layer-0 intercepts and among the rows that leave the counter alone."""
    relu, rows = crafted
    idx = list(range(len(SEQ)))
    whole, whole_icp = decide_on_device(engine, rows, idx, 0)
    first, mid = decide_on_device(engine, rows, idx[:cut], 0)
    second, last = decide_on_device(engine, rows, idx[cut:], mid)
    assert first + second == whole and last == whole_icp


def test_an_order_that_names_no_usable_layer_gives_no_decision(crafted, engine):
    """random_order = [], and one that names only the layer the "popped" row has nothing undecided in: a row that reaches the order branch
    and finds no layer gets [-1, -1] and the counter stays (the host rule raises there); rows decided by score or intercept are as before."""
    relu, rows = crafted
    hi = len(relu) - 1
    idx = list(range(len(SEQ)))
    full, _, _ = rule_reference(relu, rows, idx, 1)
    for order in ([], [hi]):
        want, want_icp, _ = rule_reference(relu, rows, idx, 1, order=order)
        got, got_icp = decide_on_device(engine, rows, idx, 1, random_order=order)
        assert got == want and got_icp == want_icp, (order, got, want, got_icp, want_icp)
        assert want[SEQ.index("popped")] == [-1, -1] and want[SEQ.index("score")] == full[SEQ.index("score")]
        assert (want[SEQ.index("sparsest_max")] == [-1, -1]) == (order == [])


# ---- 2. agreement with the fall-back's kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("icp0", [0, 2])
def test_the_fall_back_below_its_threshold_decides_the_same(icp0, crafted, engine):
    """Pair A's bounds equal the parents' (all below 0): every improvement is 0, every row is below the branching threshold, so
    gnnb_frontier_fallback's kw_decisions and counter are the new entry point's."""
    relu, rows = crafted
    dev, K, R = engine.device, len(SEQ), engine.R
    pool = DomainPool(engine, K + 3)
    slots = torch.randperm(K + 3, generator=torch.Generator().manual_seed(4))[:K].to(I32)
    parent = -(torch.rand(K, generator=torch.Generator().manual_seed(5), dtype=F64) + 0.5)
    pb = torch.full((K + 3,), -9.0, dtype=F64)
    pb[slots.long()] = parent
    pool.bound.copy_(pb)
    pool.open.fill_(1)
    imp, kw = torch.full((K,), -5.0, dtype=F64, device=dev), torch.full((K, 2), -7, dtype=I32, device=dev)
    sel_rows, sel_slots, sel_dec = (torch.full(s, -7, dtype=I32, device=dev) for s in ((K,), (K,), (K, 2)))
    m, icp = torch.full((1,), -7, dtype=I32, device=dev), torch.tensor([icp0], dtype=I32).to(dev)
    engine.frontier_fallback(pool, slots.to(dev), torch.ones(2 * K, dtype=I32, device=dev), torch.zeros(2 * K, dtype=I32, device=dev),
                             parent.repeat_interleave(2).to(dev), rows["scores"].to(dev), rows["icps"].to(dev), rows["amb"].to(dev), icp,
                             torch.zeros(R, dtype=I32, device=dev), imp, kw, sel_rows, sel_slots, sel_dec, m, 0.5, 10, SPARSEST, DTHR)
    assert imp.cpu().tolist() == [0.0] * K
    got, got_icp = decide_on_device(engine, rows, list(range(K)), icp0)
    assert kw.cpu().tolist() == got and int(icp.cpu()[0]) == got_icp
    assert int(m.cpu()[0]) == sum(d != [-1, -1] for d in got)          # (the old entry point still selects; the new one has no list)


# ---- 3. the jobs form -----------------------------------------------------------------------------------------------------------------
def test_jobs_form_per_entry_equals_the_one_job_call(crafted, engine):
    """Three entries over four segments, in an order that is not the segments'; segment 1 has no entry.  Per entry: the one-job call on its
    rows with its segment's counter.  Segment 1's counter and the rows from n on keep their sentinels."""
    relu, rows = crafted
    dev, K = engine.device, len(SEQ)
    spec = [(2, list(range(0, 9))), (0, list(range(9, 10))), (3, list(range(10, K)))]       # (a cut inside the run of intercepts)
    entries, row0 = [], 0
    for seg, ix in spec:
        entries.append((seg, row0, len(ix)))
        row0 += len(ix)
    n = row0
    plan = RoundPlan(dev, 4, 4, 8)
    plan.send(entries)
    icp0 = [2, 77, 1, 0]
    pad = lambda t: torch.cat([t, torch.full((2, t.shape[1]), 3.0)]).contiguous().to(dev)      # noqa: E731
    dec = torch.full((n + 2, 2), -7, dtype=I32, device=dev)
    icp = torch.tensor(icp0, dtype=I32).to(dev)
    engine.frontier_babsr_decide_jobs(plan, pad(rows["scores"]), pad(rows["icps"]), pad(rows["amb"]), icp, dec, SPARSEST, DTHR)
    dec, icp = dec.cpu(), icp.cpu().tolist()
    for (seg, ix), (_, r0, k) in zip(spec, entries):
        want, want_icp = decide_on_device(engine, rows, ix, icp0[seg])
        assert dec[r0:r0 + k].tolist() == want and icp[seg] == want_icp, (seg, r0, k)
        ref, ref_icp, _ = rule_reference(relu, rows, ix, icp0[seg])
        assert want == ref and want_icp == ref_icp, seg
    assert icp[1] == 77 and dec[n:].tolist() == [[-7, -7]] * 2


# ---- 4. the loop against the host twin ------------------------------------------------------------------------------------------------------
_shared = {}


def babsr_run(K, rounds, choice=None, **kw):
    lp, shared_choice, _ = toy()
    trace, stats = [], {}
    res = branch_and_bound_frontier(lp, shared_choice if choice is None else choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                    log=quiet, trace=trace, stats=stats, branching="babsr", **kw)
    return res, trace, stats


def runs(K, rounds, sparsest=0):
    if (K, rounds, sparsest) not in _shared:
        _shared[(K, rounds, sparsest)] = (babsr_twin(K, rounds, sparsest=sparsest), babsr_run(K, rounds, sparsest_layer=sparsest))
    return _shared[(K, rounds, sparsest)]


@pytest.mark.parametrize("K,rounds,sparsest", [(1, 4, 0), (3, 3, 0), (3, 3, 2)])
def test_the_loop_equals_the_host_loop_of_the_existing_pieces(K, rounds, sparsest):
    """sparsest_layer = 2 takes toy_kw's score decisions (all in its last layer) away: those rounds go through the intercept and the order
    branches, with the counter carried from row to row and from round to round."""
    twin, (res, trace, stats) = runs(K, rounds, sparsest)
    glb, gub, n_rounds, bounded, reason = res
    print("twin", twin, "frontier", res, stats)
    assert twin["branches"] >= 3
    assert [t["decisions"] for t in trace] == twin["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]   # bit for bit: Python floats of the same fp64 values
    assert glb == twin["global_lb"]
    assert abs(gub - twin["global_ub"]) <= 1e-9 * max(1.0, abs(twin["global_ub"]))
    assert bounded == 1 + sum(len(t["live"]) for t in trace)
    assert stats["branches"] == twin["branches"] and stats["domains_bounded"] == bounded
    assert [t["parent_bounds"] for t in trace] == twin["parent_bounds"]                                     # a traced round's parent bounds are the pool's


# ---- 5. the GNN is not consulted ----------------------------------------------------------------------------------------------------------
def test_a_round_launches_one_decide_and_no_forward_kernel():
    lp, choice, _ = toy()
    eng = choice.model.engine()
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.profile_trace()
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=3, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=3, log=quiet, branching="babsr")
        counts = eng.profile_read()
        names = [name for name, _ in eng.profile_trace(1 << 16)]
    finally:
        eng.profile_enable(False)
    rounds = res[2]
    assert rounds >= 2
    assert names.count("k_frontier_babsr_decide") == rounds == names.count("k_frontier_candidates") == names.count("k_frontier_gather")
    for k in FORWARD_CLASSES:
        assert k not in names and counts[k][1] == 0, k
    assert "k_frontier_fallback" not in names and "k_frontier_babsr_decide_jobs" not in names
    assert res == runs(3, 3)[1][0]                           # profiling changes nothing


def test_other_gnn_weights_change_nothing():
    _, (res, trace, _) = runs(3, 3)
    _, _, root_mask = toy()
    other = bab_caller.BatchedGraphChoice(root_mask, CKPT)
    other.verbose = False
    with torch.no_grad():
        for p in other.model.parameters():
            p.mul_(-0.5)
    res2, trace2, _ = babsr_run(3, 3, choice=other)
    assert res2 == res and trace2 == trace


# ---- 6. many jobs ---------------------------------------------------------------------------------------------------------------------------
def torch_fp64(layers, x):
    with torch.no_grad():
        act = x.double()
        for l in layers:
            act = copy.deepcopy(l).double()(act)
    return act


@pytest.mark.parametrize("pgd", [None, 2])
def test_every_job_gets_what_it_gets_alone(pgd):
    """Three jobs in two segments (the third is admitted late, into a reused segment): every result tuple equals the run alone, bit for
    bit; with FrontierJobs(jobs, witness=[], pgd_steps=2) every job's global_ub is the network's fp64 value at its witness."""
    from tests.test_gpu_frontier_jobs import JOBS, toy_jobs
    choice, lps = toy_jobs()
    K, cap, rounds = 2, 9, 3
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], db) for lp, (_, _, _, db) in zip(lps[:3], JOBS)]
    upper = {} if pgd is None else {"pgd_steps": pgd}
    alone, alone_stats = [], []
    for lp, job in zip(lps, jobs):
        st = {}
        alone.append(branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=cap,
                                               decision_bound=job.decision_bound, log=quiet, stats=st, branching="babsr", **upper))
        alone_stats.append({k: st[k] for k in ("branches", "domains_bounded")})
    points, trace, stats = [], [], []
    together = jobs if pgd is None else FrontierJobs(jobs, witness=points, pgd_steps=pgd)
    got = verify_properties_babsr(choice, lps[0].layers[:-1], together, K=K, segments=2, capacity=cap, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                                  max_rounds=rounds, log=quiet, trace=trace, stats=stats)
    assert {row["segment"] for row in trace if row["job"] == 2} <= {0, 1} and any(row["job"] == 2 for row in trace)
    assert sum(a[2] for a in alone) >= 3
    for j in range(3):
        print("job", j, "alone", alone[j], "together", got[j])
        assert got[j] == alone[j], j
    assert stats == alone_stats
    if pgd is not None:
        assert len(points) == 3 and any(p is not None for p in points)
        for j, (lp, p) in enumerate(zip(lps, points)):
            assert (p is None) == (got[j][1] == float("inf")), j
            if p is not None:
                f64 = float(torch_fp64(lp.layers, p[None]).reshape(()))
                assert abs(f64 - got[j][1]) <= 1e-9 * max(1.0, abs(f64)), (j, f64, got[j][1])


# ---- 7. branching="gnn" -----------------------------------------------------------------------------------------------------------------------
def test_branching_gnn_is_the_default_run():
    lp, choice, _ = toy()
    out = []
    for kw in ({}, {"branching": "gnn"}):
        trace = []
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=3, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=quiet, trace=trace, **kw)
        out.append((res, trace))
    assert out[0] == out[1] and len(out[0][1]) >= 1


# ---- 8. the limits that need a handle ---------------------------------------------------------------------------------------------------------
def test_limits(crafted, engine):
    """An unbound handle is GNNB_E_STATE; a null array GNNB_E_INVALID; a workspace one byte short GNNB_E_NOMEM, and nothing was written."""
    from gnn_branching_amd.engine import ScorerEngine
    relu, rows = crafted
    dev, K = engine.device, 4
    fresh = ScorerEngine(None)
    one = torch.zeros(8, dtype=F32, device=dev)
    assert fresh.lib.gnnb_frontier_babsr_decide(fresh.h, 1, one.data_ptr(), one.data_ptr(), one.data_ptr(), 0.001, 0, None, 0, one.data_ptr(), one.data_ptr(),
                                                one.data_ptr(), 32, None) == -3
    assert b"gnnb_frontier_babsr_decide: call gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_babsr_decide_workspace_bytes(fresh.h, 4) == 0
    need = engine.lib.gnnb_frontier_babsr_decide_workspace_bytes(engine.h, K)
    assert need > 0
    s, t, a = (rows[k][:K].contiguous().to(dev) for k in ("scores", "icps", "amb"))
    dec, icp = torch.full((K, 2), -7, dtype=I32, device=dev), torch.zeros(1, dtype=I32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    order = (C.c_int32 * 3)(0, 1, 2)
    lib, h = engine.lib, engine.h
    assert lib.gnnb_frontier_babsr_decide(h, K, s.data_ptr(), t.data_ptr(), a.data_ptr(), DTHR, 0, order, 3, icp.data_ptr(), dec.data_ptr(), ws.data_ptr(),
                                          need - 1, None) == -4
    assert lib.gnnb_frontier_babsr_decide(h, K, s.data_ptr(), None, a.data_ptr(), DTHR, 0, order, 3, icp.data_ptr(), dec.data_ptr(), ws.data_ptr(), need,
                                          None) == -1
    assert b"gnnb_frontier_babsr_decide: null argument" in lib.gnnb_last_error()
    assert lib.gnnb_frontier_babsr_decide(h, K, s.data_ptr(), t.data_ptr(), a.data_ptr(), DTHR, 0, None, 3, icp.data_ptr(), dec.data_ptr(), ws.data_ptr(), need,
                                          None) == -1           # an order of three layers and no array
    torch.cuda.synchronize()
    assert dec.cpu().tolist() == [[-7, -7]] * K
    with pytest.raises(ValueError, match="scores"):          # the Python wrapper checks rows and dtypes
        engine.frontier_babsr_decide(s.double(), t, a, icp, dec, K)
    with pytest.raises(ValueError, match="decisions"):
        engine.frontier_babsr_decide(s, t, a, icp, dec[:2], K)
    engine.frontier_babsr_decide(s, t, a, icp, dec, K, SPARSEST, DTHR, workspace=ws)
    assert dec.cpu().tolist() == rule_reference(relu, rows, range(K), 0)[0]
