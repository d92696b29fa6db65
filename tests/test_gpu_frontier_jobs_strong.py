"""Strong branching, its audit and the imitation step for many jobs in one pool on the MI355X (DESIGN.md section 7.13;
gnn_branching_amd/frontier.py verify_properties_strong, StrongJobsRun; csrc/gnnb_k_strong.h k_strong_rows_jobs).  Every comparison is
exact -- Python floats of the same fp64 values, fp32 bits for losses and parameters -- but global_ub, within 1e-9 max(1, |ub|).

1. gnnb_strong_rows_jobs against torch indexing;
2. the defining property: every job gets the result, the stats and the per-round trace ``branch_and_bound_frontier(branching="strong")``
   gives it alone, with chunks that span two jobs;
3. an audited "gnn" run is ``verify_properties``' run;
4. one job in one segment that learns is the one-job learning run;
5. several jobs that learn from one step, against a host loop of public pieces (tests/frontier_jobs_imitation_twin.py);
6. the launches and the reads of a round; 7. the limits that need a handle."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib
from gnn_branching_amd.frontier import (FrontierJob, FrontierJobs, StrongJobsRun, _Round, branch_and_bound_frontier, plan_round, verify_properties,
                                        verify_properties_babsr, verify_properties_strong)
from tests.frontier_strong_twin import same
from tests.frontier_twin import EPS_BAB, LR, N_ITER, bind, engine, masked, toy   # noqa: F401  (engine: the module's fixture)
from tests.test_gpu_frontier_babsr import FORWARD_CLASSES
from tests.test_gpu_frontier_jobs import JOBS, toy_jobs
from tests.test_gpu_imitation import FR_CANDIDATES, FR_MARGIN, FR_ROUNDS, bits, frontier_run, same_or_nan
from tests.test_gpu_kw_geometry import Net

pytestmark = pytest.mark.gpu

F64, F32, I32 = torch.float64, torch.float32, torch.int32
STRONG_CLASSES = ("k_strong_count", "k_strong_compact", "k_strong_pick")
K, CAP, ROUNDS, CANDIDATES = 2, 9, 3, 8
_runs = {}


def quiet(s):
    pass


def close_ub(a, b):
    return a == b or abs(a - b) <= 1e-9 * max(1.0, abs(b))


def same_result(got, want):
    """Two five-tuples: exact but for global_ub."""
    return got[0] == want[0] and close_ub(got[1], want[1]) and tuple(got[2:]) == tuple(want[2:])


def jobs_of(lps, ids):
    return [FrontierJob(lps[j].input_lb, lps[j].input_ub, lps[j].layers[-1], JOBS[j][3]) for j in ids]


# ---- 1. the rows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
@pytest.mark.parametrize("case", ["one", "interleaved", "outside"])
def test_rows_against_torch_indexing(name, case, engine):
    """3 segments of 7 slots with tables of distinct random values, the output rows NaN.  one: c = 1; interleaved: c = 5, slots of all three
    segments in turn, among them the first and the last slot of a segment; outside: a list that holds -1 and 21, whose rows stay NaN."""
    net = Net(name)
    engine.bind(net.fixed, tuple(net.shape))
    dev, N0, NL, nseg, cap = engine.device, engine.sizes[0], engine.sizes[-2], 3, 7
    g = torch.Generator().manual_seed(131)
    seg_lo, seg_hi = (torch.randn(nseg, N0, generator=g, dtype=F64).to(dev) for _ in range(2))
    seg_pw, seg_pb = torch.randn(nseg, NL, generator=g).to(dev), torch.randn(nseg, generator=g).to(dev)
    slots = {"one": [13], "interleaved": [14, 0, 7, 20, 6], "outside": [3, -1, 15, 21, 9]}[case]
    c = len(slots)
    cand_slot = torch.tensor(slots, dtype=I32, device=dev)
    rows = 2 * c + 3
    nan = lambda cols, dt: torch.full((rows, cols) if cols else (rows,), float("nan"), dtype=dt, device=dev)      # noqa: E731
    x_lo, x_hi, pw, pb = nan(N0, F64), nan(N0, F64), nan(NL, F32), nan(0, F32)
    engine.strong_rows_jobs(cand_slot, c, nseg, cap, seg_lo, seg_hi, seg_pw, seg_pb, x_lo, x_hi, pw, pb)
    torch.cuda.synchronize()
    written = 0
    for q, s in enumerate(slots):
        for r in (2 * q, 2 * q + 1):
            if 0 <= s < nseg * cap:
                seg = s // cap
                assert torch.equal(x_lo[r], seg_lo[seg]) and torch.equal(x_hi[r], seg_hi[seg]) and torch.equal(pw[r], seg_pw[seg]), (q, r)
                assert bool(pb[r] == seg_pb[seg]), (q, r)
                written += 1
            else:
                assert all(bool(torch.isnan(t[r]).all()) for t in (x_lo, x_hi, pw, pb)), (q, r)
    assert written == 2 * (c - (2 if case == "outside" else 0))
    for t in (x_lo, x_hi, pw, pb):
        assert bool(torch.isnan(t[2 * c:]).all())               # rows from 2c on are as they were
    if case == "interleaved":                                     # the case's own conditions
        assert {s // cap for s in slots} == {0, 1, 2} and {0, 6, 7, 14, 20} == set(slots)


# ---- 2. the defining property -----------------------------------------------------------------------------------------------------------------
def alone_strong(chunk, pgd):
    """Jobs 0..2 through the one-job loop, strong branching: [(result, trace, stats)]."""
    key = ("alone", chunk, pgd)
    if key not in _runs:
        choice, lps = toy_jobs()
        out = []
        for lp, (_, _, _, db) in list(zip(lps, JOBS))[:3]:
            trace, stats = [], {}
            res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, decision_bound=db, capacity=CAP,
                                            log=quiet, trace=trace, stats=stats, pgd_steps=pgd, strong_candidates=CANDIDATES, strong_chunk=chunk,
                                            branching="strong")
            out.append((res, trace, stats))
        _runs[key] = out
    return _runs[key]


@pytest.mark.parametrize("pgd", [None, 2])
@pytest.mark.parametrize("chunk", [3, 256])
def test_every_job_gets_the_result_it_gets_alone(chunk, pgd):
    """Three jobs in two segments, so the third is admitted late into a reused segment; K = 2, capacity 9, 3 rounds, 8 candidates.  At
    chunk = 3 the chunks span parents and jobs."""
    choice, lps = toy_jobs()
    single = alone_strong(chunk, pgd)
    jobs = jobs_of(lps, range(3))
    trace, stats = [], []
    got = verify_properties_strong(choice, lps[0].layers[:-1], jobs if pgd is None else FrontierJobs(jobs, pgd_steps=pgd), K=K, segments=2, capacity=CAP,
                                   n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, log=quiet, trace=trace, stats=stats,
                                   strong_candidates=CANDIDATES, strong_chunk=chunk)
    assert len(got) == len(stats) == 3
    for j, ((res, one, one_stats), g) in enumerate(zip(single, got)):
        print("job", j, "alone", res, one_stats, "together", g, stats[j])
        assert same_result(g, res), (j, g, res)
        assert stats[j] == {k: one_stats[k] for k in ("branches", "domains_bounded", "strong_bounded")}, (j, stats[j], one_stats)
        mine = sorted((t for t in trace if t["job"] == j), key=lambda t: t["round"])
        assert [t["round"] for t in mine] == list(range(len(one)))
        for a, b in zip(mine, one):
            assert a["decisions"] == b["decisions"], (j, a["round"])
            assert masked(a["child_bounds"], a["infeasible"], a["live"]) == masked(b["child_bounds"], b["infeasible"], b["live"]), (j, a["round"])
            assert a["strong_candidates"] == b["strong_candidates"] and same(a["strong_improvement"], b["strong_improvement"]), (j, a["round"])
            assert a["parent_bounds"] == b["parent_bounds"] and [s - a["segment"] * CAP for s in a["slots"]] == b["slots"], (j, a["round"])
    # the test's own conditions
    assert sum(res[2] for res, _, _ in single) >= 3
    assert any(t["job"] == 2 for t in trace) and {t["segment"] for t in trace} == {0, 1}
    boxes = [(lps[j].input_lb, lps[j].layers[-1].weight) for j in range(3)]
    assert all(not torch.equal(boxes[a][0], boxes[b][0]) or not torch.equal(boxes[a][1], boxes[b][1]) for a, b in ((0, 1), (0, 2), (1, 2)))
    if chunk == 3:                                                # a round of two jobs with more than 3 candidates: a chunk spans two jobs
        spans = False
        for i in range(len(trace) - 1):
            a, b = trace[i], trace[i + 1]
            if a["job"] != b["job"] and a["segment"] < b["segment"] and b["slots"][0] // CAP == b["segment"]:
                n_a, n_b = (sum(len(c) for c in t["strong_candidates"]) for t in (a, b))
                spans |= n_a % chunk != 0 and n_b > 0 and n_a + n_b > chunk
        assert spans, "no chunk of this run holds candidates of two jobs"


# ---- 3. the audit ---------------------------------------------------------------------------------------------------------------------------
def test_an_audited_gnn_run_is_the_run():
    choice, lps = toy_jobs()
    jobs = jobs_of(lps, range(3))
    args = dict(K=K, segments=2, capacity=CAP, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, log=quiet)
    t0, t1, audit, stats = [], [], [], []
    want = verify_properties(choice, lps[0].layers[:-1], jobs, trace=t0, **args)
    got = verify_properties_strong(choice, lps[0].layers[:-1], jobs, trace=t1, stats=stats, strong_candidates=CANDIDATES, strong_chunk=5,
                                   strong_audit=audit, branching="gnn", **args)
    assert got == want                                        # bit for bit: floats by ==
    assert len(t0) == len(t1) and all(same({k: a[k] for k in b}, b) for a, b in zip(t1, t0))
    assert "strong_candidates" not in t1[0]
    parents = [(t["job"], t["segment"], t["round"], s, d) for t in t1 for s, d in zip(t["slots"], t["decisions"])]
    assert [(a["job"], a["segment"], a["round"], a["slot"], a["decision"]) for a in audit] == parents and len(parents) >= 6
    relu = list(choice.model.engine().sizes[1:-1])
    off = [0] + list(np.cumsum(relu))
    inside = 0
    for a in audit:
        assert len(a["candidates"]) == len(a["improvements"]) <= CANDIDATES
        flat = off[a["decision"][0]] + a["decision"][1]
        if flat in a["candidates"] and a["improvement"] == a["improvement"]:
            inside += 1
            assert a["improvement"] <= a["best_improvement"], a
            assert a["improvement"] == a["improvements"][a["candidates"].index(flat)], a      # the round's own children: the candidate's, bit for bit
    assert inside >= 1
    assert [s["strong_bounded"] for s in stats] == [2 * sum(len(a["candidates"]) for a in audit if a["job"] == j) for j in range(3)]
    assert [s["branches"] for s in stats] == [sum(1 for a in audit if a["job"] == j) for j in range(3)]


# ---- 4. one job in one segment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branching", ["gnn", "strong"])
@pytest.mark.parametrize("K_,imitate", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_one_job_in_one_segment_is_the_one_job_learning_run(K_, imitate, branching):
    from gnn_branching_amd.engine import state_blob
    res, one, one_audit, one_stats, one_choice = frontier_run(K_, imitate, branching)
    lp, choice, _ = toy(online=True)
    trace, audit, stats, learned = [], [], [], {}
    got = verify_properties_strong(choice, lp.layers[:-1], [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1])], K=K_, segments=1, capacity=1024,
                                   n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=FR_ROUNDS, log=quiet, trace=trace, stats=stats, learned=learned,
                                   imitate=imitate, imitate_margin=FR_MARGIN[branching], strong_candidates=FR_CANDIDATES, strong_audit=audit,
                                   branching=branching)
    print("alone", res, one_stats, "as a job", got, stats, learned)
    assert len(got) == 1 and same_result(got[0], res)
    assert len(trace) == len(one) >= 2
    for a, b in zip(trace, one):
        assert (a["job"], a["segment"]) == (0, 0)
        for key in b:
            if key == "global_ub":
                assert close_ub(a[key], b[key])
            elif key == "imitation_loss":
                np.testing.assert_array_equal(bits(a[key]), bits(b[key]))
            else:
                assert same(a[key], b[key]), (a["round"], key)
    assert any("imitation_loss" in t for t in trace)
    assert same([{k: v for k, v in a.items() if k not in ("job", "segment", "round")} for a in audit], one_audit)
    assert learned == {"imitation_steps": one_stats["imitation_steps"], "imitation_rows": one_stats["imitation_rows"], "rounds": res[2]}
    assert learned["imitation_steps"] >= 1
    assert stats == [{k: one_stats[k] for k in ("branches", "domains_bounded", "strong_bounded")}]
    w, one_w = choice._eng().get_weights(), one_choice._eng().get_weights()
    np.testing.assert_array_equal(bits(w), bits(one_w))                                              # the final parameters, bit for bit
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(w))              # the nn.Module mirrors the device


# ---- 5. several jobs learn from one step ------------------------------------------------------------------------------------------------
LEARN_JOBS = (0, 6, 1)              # JOBS[6] ends at its root: its segment is reused at once, and the run's rounds are no job's


def learning_runs(imitate, branching):
    key = ("learn", imitate, branching)
    if key not in _runs:
        from tests.frontier_jobs_imitation_twin import host_loop, online_jobs
        choice, lps = online_jobs(LEARN_JOBS)
        trace, audit, stats, learned = [], [], [], {}
        got = verify_properties_strong(choice, lps[0].layers[:-1], jobs_of_list(lps), K=K, segments=2, capacity=CAP, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                                       max_rounds=ROUNDS, log=quiet, trace=trace, stats=stats, learned=learned, imitate=imitate,
                                       imitate_margin=FR_MARGIN[branching], strong_candidates=FR_CANDIDATES, strong_audit=audit, branching=branching)
        host = host_loop(LEARN_JOBS, K, 2, CAP, ROUNDS, imitate, branching, audit, FR_MARGIN[branching])
        _runs[key] = (host, got, trace, audit, stats, learned, choice)
    return _runs[key]


def jobs_of_list(lps):
    return [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], JOBS[j][3]) for lp, j in zip(lps, LEARN_JOBS)]


@pytest.mark.parametrize("branching", ["gnn", "strong"])
@pytest.mark.parametrize("imitate", [1, 2])
def test_several_jobs_learn_from_one_step(imitate, branching):
    from gnn_branching_amd.engine import state_blob
    host, got, trace, audit, stats, learned, choice = learning_runs(imitate, branching)
    print("host", {k: v for k, v in host.items() if not k.startswith("weights") and k != "entries"}, "device", got, learned)
    assert len(trace) == len(host["entries"])
    for t, e in zip(trace, host["entries"]):
        assert (t["job"], t["segment"], t["round"]) == (e["job"], e["segment"], e["round"])
        assert t["decisions"] == e["decisions"], e
        assert masked(t["child_bounds"], t["infeasible"], t["live"]) == e["child_bounds"], e
        assert ("imitation_loss" in t) == bool(e["loss"]), e
        assert t["global_lb"] == e["global_lb"] and close_ub(t["global_ub"], e["global_ub"]), e
        if e["loss"]:
            np.testing.assert_array_equal(bits(t["imitation_loss"]), bits(e["loss"]))                # the fp32 losses, bit for bit
            assert t["imitation_report"] == e["report"] and same_or_nan(t["imitation_regret"], e["regret"]), e
    for j, (g, w) in enumerate(zip(got, host["results"])):
        assert g[0] == w[0] and close_ub(g[1], w[1]) and g[2] == w[2] and g[4] == w[4], (j, g, w)
    assert learned == {"imitation_steps": host["steps"], "imitation_rows": host["rows"], "rounds": host["rounds"]}
    w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(w), bits(host["weights"]))                                    # the final parameters, bit for bit
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(w))
    # so that the comparison shows something
    assert host["steps"] >= 1 and any(v > 0 for e in host["entries"] for v in e["loss"]), "no step carried a gradient"
    first = min(e["run_round"] for e in host["entries"] if e["loss"])
    assert any(e["run_round"] > first for e in host["entries"]), "no decision was taken after a step"
    learning = [e for e in host["entries"] if e["loss"]]
    assert any(a["run_round"] == b["run_round"] and a["job"] != b["job"] for a in learning for b in learning), "no learning round held two jobs"
    assert any(e["run_round"] != e["round"] + 1 for e in host["entries"]), "the run's round numbers are every job's own"
    assert got[1][2] == 0 and got[1][4] == "exhausted"       # the job that ends at its root
    res, _, _, _, one_choice = frontier_run(K, imitate, branching, rounds=ROUNDS, capacity=CAP)      # job 0 learning alone
    assert (bits(one_choice._eng().get_weights()) != bits(w)).any()


# ---- 6. launches and reads ------------------------------------------------------------------------------------------------------------------
def profiled(eng, call):
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.profile_trace()
        out = call()
        counts = eng.profile_read()
        names = [name for name, _ in eng.profile_trace(1 << 16)]
    finally:
        eng.profile_enable(False)
    return out, names, counts


@pytest.mark.parametrize("imitate", [None, 1])
def test_a_strong_run_launches_no_forward_kernel_and_one_row_copy_per_chunk(imitate, monkeypatch):
    from tests.frontier_jobs_imitation_twin import online_jobs
    chunk = 5
    if imitate is None:
        choice, lps = toy_jobs()
        eng, jobs, extra = choice.model.engine(), jobs_of(lps, range(3)), {}
    else:
        choice, lps = online_jobs((0, 1, 2))
        eng, jobs, extra = choice._eng(), jobs_of(lps, range(3)), {"imitate": 1}
    counts_read, read = [], StrongJobsRun.read_candidates

    def counting(self, n):
        counts_read.append(read(self, n))
        return counts_read[-1]
    monkeypatch.setattr(StrongJobsRun, "read_candidates", counting)
    learned = {}
    got, names, counts = profiled(eng, lambda: verify_properties_strong(choice, lps[0].layers[:-1], jobs, K=K, segments=2, capacity=CAP, n_iter=N_ITER,
                                                                       lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, log=quiet, learned=learned,
                                                                       strong_candidates=CANDIDATES, strong_chunk=chunk, **extra))
    rounds = learned["rounds"]
    chunks = sum(-(-n // chunk) for n in counts_read)
    assert rounds >= 3 and len(counts_read) == rounds and chunks > rounds
    for k in FORWARD_CLASSES:
        assert k not in names and counts[k][1] == 0, k
    for k in STRONG_CLASSES:
        assert names.count(k) == rounds, k
    assert names.count("k_frontier_rows_sel") == chunks and names.count("k_frontier_expand") == chunks + rounds
    assert "k_frontier_fallback_jobs" not in names and "k_frontier_select_jobs" not in names and "k_frontier_babsr_decide_jobs" not in names
    assert names.count("k_frontier_pick_jobs") == rounds and names.count("k_frontier_gather") == rounds
    assert names.count("k_trows_gather") == (0 if imitate is None else learned["imitation_steps"])
    assert learned["imitation_steps"] == (0 if imitate is None else rounds)


def test_the_other_jobs_loops_launch_no_strong_kernel_and_read_no_candidate_count(monkeypatch):
    choice, lps = toy_jobs()
    jobs = jobs_of(lps, range(3))

    def never(self, n):
        raise AssertionError("a run without a table read a candidate count")
    monkeypatch.setattr(_Round, "read_candidates", never)
    monkeypatch.setattr(StrongJobsRun, "read_candidates", never)
    args = dict(K=K, segments=2, capacity=CAP, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, log=quiet)
    for f in (verify_properties, verify_properties_babsr):
        got, names, counts = profiled(choice.model.engine(), lambda: f(choice, lps[0].layers[:-1], jobs, **args))
        assert len(got) == 3 and names.count("k_frontier_pick_jobs") >= 3
        for k in STRONG_CLASSES + ("k_frontier_rows_sel", "k_trows_gather"):
            assert k not in names and counts[k][1] == 0, (f.__name__, k)


@pytest.mark.parametrize("imitate", [None, 1])
def test_a_round_of_three_segments_copies_nothing_but_the_candidate_counts_and_the_records(imitate):
    """One round of three segments under torch.cuda.set_sync_debug_mode("error"): the read of the candidate counts (ONE copy of
    4 (entries + 1) bytes) and the read of the records are the two exemptions; a learning round's step runs under the mode (its own stream
    synchronisation inside the library is not torch's)."""
    from gnn_branching_amd.frontier import JobsRun
    from tests.frontier_jobs_imitation_twin import online_jobs
    from tests.test_gpu_frontier_online import sync_mode_is_live
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    choice, lps = toy_jobs() if imitate is None else online_jobs((0, 1, 2))
    jobs = jobs_of(lps, range(3))
    extra = {} if imitate is None else {"imitate": 1}
    run = StrongJobsRun(choice, lps[0].layers[:-1], jobs, tuple(lps[0].input_lb.shape), K, 3, CAP, N_ITER, LR, EPS_BAB, strong_candidates=CANDIDATES,
                        strong_chunk=5, **extra)
    for s in range(3):
        run.admit(s, s)
    run.launch_roots([0, 1, 2])
    st = run.read_state()
    if not sync_mode_is_live(run):
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
    before = torch.cuda.get_sync_debug_mode()
    w0 = run.eng.get_weights().copy()
    reads, read_candidates = [], run.read_candidates

    def exempt_read(n):
        with pytest.raises(RuntimeError):
            read_candidates(n)
        torch.cuda.set_sync_debug_mode(before)
        try:
            reads.append(read_candidates(n))
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return reads[-1]
    run.read_candidates = exempt_read
    try:
        torch.cuda.set_sync_debug_mode("error")
        entries, compact, stopped = plan_round(st, K, CAP)
        assert len(entries) == 3 and not stopped
        run.launch_round(entries)
        with pytest.raises(RuntimeError):
            run.read_state()                                  # the records: a synchronising copy
        torch.cuda.set_sync_debug_mode(before)
        st = JobsRun.read_state(run)                          # ... exempted by hand
        assert run.imitate_pending == run.learning == (imitate is not None)
        torch.cuda.set_sync_debug_mode("error")
        if imitate is not None:
            run._imitate()                                    # no read of its own: the candidate count is the host's copy
        torch.cuda.set_sync_debug_mode(before)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert reads == [3 * CANDIDATES] and run.cand_entry == [0, CANDIDATES, 2 * CANDIDATES, 3 * CANDIDATES] and run.round == 1
    assert all(r[_lib.FS_KEPT] + r[_lib.FS_CLOSED] + r[_lib.FS_INFEASIBLE] >= 2 for r in st)
    run.check_status()
    if imitate is not None:
        assert run.imitation_steps == 1 and run.imitation_rows == 3 and not run.imitate_pending
        assert (bits(run.eng.get_weights()) != bits(w0)).any()


# ---- 7. the limits that need a handle -------------------------------------------------------------------------------------------------------
def test_limits(engine):
    """An unbound handle is GNNB_E_STATE; a null array GNNB_E_INVALID; the handle stays usable."""
    from gnn_branching_amd.engine import ScorerEngine
    bind(engine, "kwg_mlp")
    dev, N0, NL = engine.device, engine.sizes[0], engine.sizes[-2]
    fresh = ScorerEngine(None)
    one = torch.zeros(64, dtype=F64, device=dev)
    p = one.data_ptr()
    assert fresh.lib.gnnb_strong_rows_jobs(fresh.h, p, 1, 1, 1, p, p, p, p, p, p, p, p, None) == -3
    assert b"gnnb_strong_rows_jobs: call gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    lib, h = engine.lib, engine.h
    seg = [torch.randn(2, N0, dtype=F64, device=dev), torch.randn(2, N0, dtype=F64, device=dev), torch.randn(2, NL, device=dev), torch.randn(2, device=dev)]
    out = [torch.full((2, N0), 7.0, dtype=F64, device=dev), torch.full((2, N0), 7.0, dtype=F64, device=dev), torch.full((2, NL), 7.0, device=dev),
           torch.full((2,), 7.0, device=dev)]
    slot = torch.tensor([5], dtype=I32, device=dev)
    ptrs = [slot.data_ptr()] + [t.data_ptr() for t in seg + out]
    for i in range(len(ptrs)):
        a = list(ptrs)
        a[i] = None
        assert lib.gnnb_strong_rows_jobs(h, a[0], 1, 2, 4, *a[1:], None) == -1, i
        assert b"gnnb_strong_rows_jobs: null argument" in lib.gnnb_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)           # nothing was launched
    engine.strong_rows_jobs(slot, 1, 2, 4, *seg, *out)        # the handle is still usable: slot 5 of segments of 4 is segment 1
    torch.cuda.synchronize()
    assert all(torch.equal(o[r], s[1]) for o, s in zip(out, seg) for r in (0, 1))
    assert engine.lib.gnnb_strong_rows_jobs(h, ptrs[0], C.c_int(0), 2, 4, *ptrs[1:], None) == -1 and b"c = 0 " in lib.gnnb_last_error()
