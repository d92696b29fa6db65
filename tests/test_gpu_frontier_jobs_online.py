"""Online learning for every job of a many-property frontier, on the MI355X (gnn_branching_amd/frontier.py
verify_properties_online / OnlineJobsRun; csrc/gnnb_k_frontier.h k_frontier_learn_jobs / k_frontier_learn_compact).  Every comparison is
exact unless said.

1. gnnb_frontier_learn_jobs against the existing gnnb_frontier_learn called once per entry on that entry's rows with that segment's table
   (and against the restatement of tests/frontier_jobs_online_twin.py);
2. one job in one segment equals ``branch_and_bound_frontier(branching_threshold=T, online_threshold=N)`` bit for bit;
3. with a threshold nobody reaches every job equals ``verify_properties_threshold(kwbd_threshold=2**31-1)``;
4. many jobs against the host twin: one step per round over the learn rows of all jobs in flight;
5. a reused segment starts from a zero table; 6. what crosses the link in a round; 7. repack="device"; 8. the limits."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, frontier
from gnn_branching_amd.engine import ScorerEngine, state_blob
from gnn_branching_amd.frontier import FrontierJob, OnlineJobsRun, plan_round, verify_properties_online, verify_properties_threshold
from tests import test_gpu_frontier_online as tfo
from tests.frontier_jobs_imitation_twin import online_jobs
from tests.frontier_jobs_online_twin import host_loop, learn_jobs_reference
from tests.frontier_twin import EPS_BAB, LR, N_ITER, bind, engine, masked   # noqa: F401  (engine: the module's fixture)
from tests.test_gpu_frontier_jobs import JOBS, sent
from tests.test_gpu_frontier_jobs_threshold import same_value
from tests.test_gpu_frontier_online import LSEQ, bits, learn_rows, run_learn

pytestmark = pytest.mark.gpu

S = _lib
I32, F32 = torch.int32, torch.float32
QUIET = lambda s: None      # noqa: E731


# ---- 1. gnnb_frontier_learn_jobs -------------------------------------------------------------------------------------------------------
class LearnCase:
    """The arguments of one gnnb_frontier_learn_jobs call: ``spec`` = [(segment, rows of ``rows`` (tests/test_gpu_frontier_online.py
    learn_rows))] in plan order, ``wrong0`` the (segments, R) tables it starts from."""

    def __init__(self, engine, nseg, spec, rows, wrong0, thr):
        self.engine, self.nseg, self.spec, self.rows, self.wrong0, self.thr, self.dev = engine, nseg, spec, rows, wrong0, thr, engine.device
        self.entries, row0 = [], 0
        for seg, idx in spec:
            self.entries.append((seg, row0, len(idx)))
            row0 += len(idx)
        self.n, self.idx = row0, [i for _, ix in spec for i in ix]
        self.plan = sent(self.dev, self.entries, nseg, 8)

    def run(self, workspace=None, thr=None):
        dev, n, E, ix = self.dev, self.n, len(self.entries), torch.tensor(self.idx)
        o = {"rows": torch.full((n + 1,), -7, dtype=I32, device=dev), "kw": torch.full((n + 1,), -7, dtype=I32, device=dev),
             "imp": torch.full((n + 1,), -7.0, dtype=F32, device=dev), "entry": torch.full((E + 2,), -7, dtype=I32, device=dev),
             "wrong": self.wrong0.clone().to(dev)}
        r = self.rows
        self.engine.frontier_learn_jobs(self.plan, r["gnn_dec"][ix].contiguous().to(dev), r["kw_dec"][ix].contiguous().to(dev),
                                        r["used"][ix].contiguous().to(dev), r["gnn_imp"][ix].contiguous().to(dev), r["kw_imp"][ix].contiguous().to(dev),
                                        self.thr if thr is None else thr, o["wrong"], o["rows"], o["kw"], o["imp"], o["entry"], workspace=workspace)
        return {k: v.cpu() for k, v in o.items()}

    def per_entry(self, got):
        """Per segment what its entry got: its count and its slice of the dense lists (GLOBAL rows), its table afterwards."""
        per, a = {}, 0
        for e, (seg, row0, k) in enumerate(self.entries):
            m = int(got["entry"][e])
            per[seg] = {"n": m, "rows": got["rows"][a:a + m].tolist(), "kw": got["kw"][a:a + m].tolist(), "imp": got["imp"][a:a + m].tolist(),
                        "wrong": got["wrong"][seg].tolist(), "row0": row0}
            a += m
        return per

    def one_job(self, e):
        """The existing gnnb_frontier_learn on entry e's rows with its segment's table: the reference."""
        seg, row0, k = self.entries[e]
        g = run_learn(self.engine, self.rows, self.spec[e][1], self.wrong0[seg].clone(), self.thr)
        m = int(g["n"][0])
        return {"n": m, "rows": [row0 + r for r in g["rows"][:m].tolist()], "kw": g["kw"][:m].tolist(), "imp": g["imp"][:m].tolist(),
                "wrong": g["wrong"].tolist(), "row0": row0}


def assert_learn_call(case, got, relu):
    """Everything one jobs call wrote against the one-job entry point per entry and against the restatement; what it must not touch is
    as it was.  Returns the per-entry results."""
    n, E = case.n, len(case.entries)
    per = case.per_entry(got)
    for e, (seg, row0, k) in enumerate(case.entries):
        assert per[seg] == case.one_job(e), (seg, row0, k)
    N = sum(p["n"] for p in per.values())
    assert got["entry"][E].item() == N and got["entry"][E + 1].item() == -7
    assert bool((got["rows"][N:] == -7).all()) and bool((got["kw"][N:] == -7).all()) and bool((got["imp"][N:] == -7.0).all())      # beyond N: as they were
    taking = {seg for seg, _, _ in case.entries}
    for seg in range(case.nseg):
        if seg not in taking:
            assert torch.equal(got["wrong"][seg], case.wrong0[seg]), seg
    ix = case.idx
    rows = {k: [case.rows[k][i].tolist() for i in ix] for k in ("gnn_dec", "kw_dec", "used", "gnn_imp", "kw_imp")}
    want = learn_jobs_reference(relu, case.entries, rows, {s: case.wrong0[s].tolist() for s in taking}, case.thr)
    assert (got["rows"][:N].tolist(), got["kw"][:N].tolist(), got["imp"][:N].tolist(), got["entry"][:E + 1].tolist()) == want[:4]
    assert all(got["wrong"][s].tolist() == want[4][s] for s in taking)
    return per


@pytest.mark.parametrize("thr", [1, 5])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_learn_jobs_against_the_one_job_call_per_entry(name, thr, engine):
    """Six segments with three different preloaded tables; entries of k = 3 (segment 4: a "reach", an "unused" and an "above" row of LSEQ:
    n_e = 2), k = 1 (segment 0: a "none" row: n_e = 0, an empty entry between two others) and k = 130 (segment 2: ten cycles of every
    kind, counts carried between rows that meet).  Then each entry alone, and the entries in another plan order: the same per-entry
    results, with the global row numbers of that plan."""
    relu = bind(engine, name)
    rows = learn_rows(relu, 160, thr, 71)
    reach, unused, above, none = (LSEQ.index(k) for k in ("reach", "unused", "above", "none"))
    spec = [(4, [reach, unused, above]), (0, [none]), (2, list(range(13, 143)))]
    nseg, R = 6, sum(relu)
    g = torch.Generator().manual_seed(72)
    wrong0 = torch.zeros(nseg, R, dtype=I32)
    wrong0[4], wrong0[0] = rows["wrong"], torch.randint(0, 3, (R,), generator=g).to(I32)
    wrong0[2] = torch.randint(max(thr - 2, 0), thr + 1, (R,), generator=g).to(I32)      # astride the threshold: some nodes reach it, some do not
    wrong0[1], wrong0[3], wrong0[5] = 7, 8, 9                 # the segments that take no part
    case = LearnCase(engine, nseg, spec, rows, wrong0, thr)
    got = case.run()
    print(name, thr, "learn_entry", got["entry"].tolist(), "rows", got["rows"].tolist()[:12], "kw", got["kw"].tolist()[:12], "improve", got["imp"].tolist()[:12])
    per = assert_learn_call(case, got, relu)
    # the test's own conditions
    assert per[4]["n"] == 2 and per[0]["n"] == 0 and per[2]["n"] > 2 and per[4]["rows"] == [0, 2] and per[4]["imp"][1] == 1.0
    assert min(per[2]["rows"]) >= 4 and {0.0, 1.0} == set(per[2]["imp"])
    assert per[2]["n"] == 130 if thr == 1 else per[2]["n"] < 130      # (at threshold 1 every row that took its KW pair learns; at 5 some counts stay below)
    assert len({tuple(wrong0[s].tolist()) for s in (4, 0, 2)}) == 3
    for sub in ([spec[0]], [spec[1]], [spec[2]], [spec[2], spec[0], spec[1]], [spec[1], spec[2]]):
        other = LearnCase(engine, nseg, sub, rows, wrong0, thr)
        p2 = assert_learn_call(other, other.run(), relu)
        for seg in p2:                                        # the same results, the rows counted from the entry's first
            a, b = p2[seg], per[seg]
            assert (a["n"], a["kw"], a["imp"], a["wrong"]) == (b["n"], b["kw"], b["imp"], b["wrong"]), ("alone", seg)
            assert [r - a["row0"] for r in a["rows"]] == [r - b["row0"] for r in b["rows"]], ("alone", seg)


def test_learn_jobs_prefix_over_more_entries_than_threads(engine):
    """kwg_mlp, 300 entries of k = 1 in 300 segments at online_threshold 2: the prefix over the entries runs past the workgroup's 256
    threads, every thread holds more than one entry, and the tables differ from segment to segment -- every row names one node, which
    the even segments have counted once (a learn row) and the odd ones never (none)."""
    relu = bind(engine, "kwg_mlp")
    nseg, R = 300, sum(relu)
    rows = learn_rows(relu, nseg, 2, 73)
    for k in ("gnn_dec", "kw_dec", "used", "gnn_imp", "kw_imp"):
        rows[k] = rows[k][2:3].expand(nseg, *rows[k].shape[1:]).contiguous()      # the "reach" row, 300 times
    node = int(rows["gnn_dec"][0, 1]) + [0, *np.cumsum(relu)][int(rows["gnn_dec"][0, 0])]
    wrong0 = torch.zeros(nseg, R, dtype=I32)
    wrong0[0::2, node] = 1
    case = LearnCase(engine, nseg, [(s, [s]) for s in range(nseg)], rows, wrong0, 2)
    got = case.run()
    per = assert_learn_call(case, got, relu)
    ns = [per[s]["n"] for s in range(nseg)]
    print("n over the entries", ns[:40], "N", sum(ns))
    assert ns == [1, 0] * 150 and got["rows"][:150].tolist() == list(range(0, 300, 2))
    assert 0 in ns[256:] and 1 in ns[256:] and 0 in ns[:256] and 1 in ns[:256]


# ---- the runs on toy_kw -----------------------------------------------------------------------------------------------------------------
CAP = 64
_shared = {}


def device_run(ids, segments, K, rounds, online_threshold, threshold=1.0, repack="host", cap=CAP, trace_on=True):
    """``verify_properties_online`` on the jobs ``ids`` of JOBS with a fresh online GraphChoice: (results, trace, stats, learned, choice)."""
    choice, lps = online_jobs(ids)
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], JOBS[j][3]) for lp, j in zip(lps, ids)]
    trace, stats, learned = [] if trace_on else None, [], {}
    got = verify_properties_online(choice, lps[0].layers[:-1], jobs, threshold, online_threshold, K=K, segments=segments, capacity=cap, n_iter=N_ITER, lr=LR,
                                   eps=EPS_BAB, max_rounds=rounds, repack=repack, log=QUIET, trace=trace, stats=stats, learned=learned)
    return got, trace, stats, learned, choice


ONLINE_KEYS = ("decisions", "gnn_decisions", "kw_decisions", "used_kw", "selected", "learn_rows", "learn_kw", "learn_improve")


# ---- 2. one job -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,rounds", [(1, tfo.ROUNDS_K1), (4, tfo.ROUNDS_K4)])
def test_one_job_in_one_segment_is_the_one_job_run(K, rounds):
    """toy_kw's property (2, 6) at eps 0.04 (JOBS[0]), T = 1.0, N = 1: the runs tests/test_gpu_frontier_online.py shows do learn."""
    (res, one, st, one_choice) = tfo.frontier_online(K, rounds, 1)
    got, trace, stats, learned, choice = device_run([0], 1, K, rounds, 1, cap=max(1024, 4 * K + 1))
    print("alone", res, st, "pool of one", got, stats, learned)
    assert st["online_steps"] >= 1 and got == [res]
    assert stats == [{k: v for k, v in st.items() if k != "online_steps"}]
    assert learned == {"online_steps": st["online_steps"], "online_rows": st["online_rows"], "rounds": res[2]}
    assert len(trace) == len(one)
    for r, (a, b) in enumerate(zip(trace, one)):
        assert (a["job"], a["segment"], a["round"]) == (0, 0, r) and set(b) | {"job", "segment", "round"} == set(a)
        for key in b:
            if key == "loss":
                np.testing.assert_array_equal(bits(a[key]), bits(b[key]))
            else:
                assert same_value(a[key], b[key]), (r, key, a[key], b[key])
    np.testing.assert_array_equal(bits(choice._eng().get_weights()), bits(one_choice._eng().get_weights()))
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(choice._eng().get_weights()))      # the nn.Module mirrors the device


# ---- 3. learning off in effect ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [3, 7])
def test_a_threshold_never_reached_is_the_threshold_run_with_every_kw_point_bounded(segments, monkeypatch):
    """online_threshold = 2^30, every job of JOBS at K = 2, three rounds, cap 9: the results, stats and traces of
    ``verify_properties_threshold(kwbd_threshold=2**31-1)`` bit for bit, the parameters untouched, no step; in 7 segments (no segment is
    reused) ``wrong[segment]`` is the per-node sum of that job's traced used_kw."""
    made = []

    class Spy(OnlineJobsRun):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(frontier, "OnlineJobsRun", Spy)
    ids = list(range(len(JOBS)))
    choice, lps = online_jobs(ids)
    w0 = choice._eng().get_weights().copy()
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], JOBS[j][3]) for lp, j in zip(lps, ids)]
    common = dict(K=2, segments=segments, capacity=9, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=3, log=QUIET)
    ref_trace, ref_stats = [], []
    ref = verify_properties_threshold(choice, lps[0].layers[:-1], jobs, 1.0, kwbd_threshold=2 ** 31 - 1, trace=ref_trace, stats=ref_stats, **common)
    trace, stats, learned = [], [], {}
    got = verify_properties_online(choice, lps[0].layers[:-1], jobs, 1.0, 2 ** 30, trace=trace, stats=stats, learned=learned, **common)
    assert got == ref and len(trace) == len(ref_trace) >= 5
    for a, b in zip(trace, ref_trace):
        for key in b:
            assert same_value(a[key], b[key]), (key, a[key], b[key])
        assert a["learn_rows"] == [] and a["learn_kw"] == [] and a["learn_improve"] == [] and a["loss"] == []
    assert learned == {"online_steps": 0, "online_rows": 0, "rounds": made[-1].round}
    assert [{k: v for k, v in s.items() if k != "online_rows"} for s in stats] == ref_stats and all(s["online_rows"] == 0 for s in stats)
    assert sum(s["kw_used"] for s in ref_stats) >= 1
    np.testing.assert_array_equal(bits(choice._eng().get_weights()), bits(w0))
    if segments < len(JOBS):
        return
    relu = list(made[-1].eng.sizes[1:-1])
    off = [0] + list(np.cumsum(relu))
    want = torch.zeros(segments, sum(relu), dtype=I32)
    for t in trace:
        for d, u in zip(t["gnn_decisions"], t["used_kw"]):
            if u:
                want[t["segment"], off[d[0]] + d[1]] += 1
    assert int(want.sum()) == sum(s["kw_used"] for s in ref_stats) and torch.equal(made[-1].wrong.cpu(), want)


# ---- 4. many jobs against the twin ------------------------------------------------------------------------------------------------------
POOL_IDS, POOL_K, POOL_ROUNDS = [0, 0, 1], 2, 4


def pool_runs(repack="host"):
    """The twin and the device run of [JOBS[0], JOBS[0], JOBS[1]] in two segments (the third job is admitted late), T = 1.0, N = 1, K = 2.
    With ``repack`` "device" the twin's engine is in that mode too (section 7.15's condition)."""
    if repack not in _shared:
        choice, lps = online_jobs(POOL_IDS)
        if repack == "device":
            choice._eng().set_repack("device")
        try:
            host = host_loop(choice, lps, [JOBS[j][3] for j in POOL_IDS], POOL_K, 2, CAP, POOL_ROUNDS, 1.0, 1, N_ITER, LR)
        finally:
            choice._eng().set_repack("host")
        _shared[repack] = (host, device_run(POOL_IDS, 2, POOL_K, POOL_ROUNDS, 1, repack=repack))
    return _shared[repack]


def assert_pool_equals_twin(host, run):
    got, trace, stats, learned, choice = run
    print("twin", {k: v for k, v in host.items() if k not in ("weights", "entries")}, "device", got, stats, learned)
    assert len(trace) == len(host["entries"])
    for t, e in zip(trace, host["entries"]):
        what = (e["job"], e["run_round"])
        print("entry", what, {k: t[k] for k in ONLINE_KEYS + ("gnn_improvement", "kw_improvement", "loss", "global_lb", "global_ub")})
        assert (t["job"], t["segment"], t["round"]) == (e["job"], e["segment"], e["round"]), what
        for key in ONLINE_KEYS:
            assert t[key] == e[key], (what, key, t[key], e[key])
        assert t["gnn_improvement"] == e["gnn_improvement"] and t["kw_improvement"] == e["kw_improvement"], what      # Python floats of the same fp64 values
        assert masked(t["child_bounds"], t["infeasible"], t["live"]) == e["child_bounds"], what
        np.testing.assert_array_equal(bits(t["loss"]), bits(e["loss"]))                      # the fp32 losses, bit for bit
        assert t["global_lb"] == e["global_lb"], what
        assert abs(t["global_ub"] - e["global_ub"]) <= 1e-9 * max(1.0, abs(e["global_ub"])), what
    for g, w in zip(got, host["results"]):
        assert g[0] == w[0] and abs(g[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])) and (g[2], g[4]) == (w[2], w[4])
    assert learned == {"online_steps": host["steps"], "online_rows": host["rows"], "rounds": host["rounds"]}
    assert [s["online_rows"] for s in stats] == [sum(len(e["learn_rows"]) for e in host["entries"] if e["job"] == j) for j in range(len(got))]
    got_w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(got_w), bits(host["weights"]))                        # the final parameters, bit for bit
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(got_w))


def test_many_jobs_equal_the_twin():
    """ONE step per round over the learn rows of all jobs in flight (the twin asserts that a step summed rows of two jobs, and that a
    forward ran after a step); the two copies of JOBS[0] stay identical throughout; every round up to the run's first step equals the
    jobs' alone online runs."""
    host, run = pool_runs()
    assert_pool_equals_twin(host, run)
    got, trace, stats, learned, choice = run
    assert got[0] == got[1] and stats[0] == stats[1]
    twins = [[t for t in trace if t["job"] == j] for j in (0, 1)]
    assert len(twins[0]) == len(twins[1]) >= 2
    for a, b in zip(*twins):
        assert {k for k in a if k not in ("job", "segment", "slots")} == {k for k in b if k not in ("job", "segment", "slots")}
        for key in a:
            if key not in ("job", "segment", "slots"):
                assert same_value(a[key], b[key]), (key, a[key], b[key])
        assert [s - a["segment"] * CAP for s in a["slots"]] == [s - b["segment"] * CAP for s in b["slots"]]
    (res, one, st, _) = tfo.frontier_online(POOL_K, POOL_ROUNDS, 1)       # JOBS[0] alone: until the first step the pool changes nothing
    first = host["first_step"]
    assert first >= 1
    for mine in twins:
        for a, b in zip(mine[:first], one[:first]):
            for key in b:
                if key == "loss":
                    np.testing.assert_array_equal(bits(a[key]), bits(b[key]))
                elif key != "slots":
                    assert same_value(a[key], b[key]), (a["job"], a["round"], key, a[key], b[key])


# ---- 5. a reused segment starts from a zero table ---------------------------------------------------------------------------------------
def test_a_job_admitted_into_a_released_segment_starts_from_a_zero_table():
    """JOBS[0] twice through ONE segment, one round each, N = 2.  The first tenant's root loses to its KW pair (count 1: no learn row);
    nothing was learnt, so the second tenant makes the same decisions and its root loses at the SAME node -- on the table of the
    previous tenant that would be count 2 and a learn row; on its own zero table it is count 1 and none."""
    got, trace, stats, learned, _ = device_run([0, 0], 1, 1, 1, 2)
    assert len(trace) == 2 and [t["job"] for t in trace] == [0, 1] and [t["segment"] for t in trace] == [0, 0]
    a, b = trace
    assert a["used_kw"] == [1] and b["used_kw"] == [1] and a["gnn_decisions"] == b["gnn_decisions"] != [[-1, -1]]
    assert a["learn_rows"] == [] and b["learn_rows"] == [] and learned["online_steps"] == 0 and learned["online_rows"] == 0
    assert got[0] == got[1]
    both, *_ = device_run([0], 1, 1, 1, 1)                    # the same round at N = 1 does learn: the count is what decides
    assert both[0][:2] == got[0][:2]


# ---- 6. device residency ----------------------------------------------------------------------------------------------------------------
def online_run(n_jobs, threshold=1.0, online_threshold=1, repack="host", K=2):
    choice, lps = online_jobs(list(range(n_jobs)))
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps]
    return OnlineJobsRun(choice, lps[0].layers[:-1], jobs, tuple(lps[0].input_lb.shape), K, n_jobs, 9, N_ITER, LR, EPS_BAB, branching_threshold=threshold,
                         online_threshold=online_threshold, repack=repack)


def test_an_online_round_of_three_segments_copies_nothing_but_m_entry_the_records_and_learn_entry():
    """Two rounds under torch.cuda.set_sync_debug_mode("error"): the read of m_entry, the records and -- in a round with M > 0 -- the read
    of learn_entry are the exemptions; everything else of the learning half runs under the mode.  Then a run whose threshold nobody is
    below: M = 0 every round, nothing is pending behind the records and learn_entry is never read."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    before = torch.cuda.get_sync_debug_mode()
    for threshold in (1.0, 1e-300):
        run = online_run(3, threshold)
        for s in range(3):
            run.admit(s, s)
        run.launch_roots([0, 1, 2])
        st = run.read_state()
        if not tfo.sync_mode_is_live(run):
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
        ms, learns = [], []
        run.read_selected = tfo.exempting(run.read_selected, before, ms)
        run.read_learn = tfo.exempting(run.read_learn, before, learns)
        try:
            for _ in range(2):
                assert all(r[S.FS_N_OPEN] >= 1 for r in st)
                torch.cuda.set_sync_debug_mode("error")
                entries, compact, stopped = plan_round(st, 2, 9)
                assert len(entries) == 3 and not stopped and not any(compact)
                run.launch_round(entries)
                with pytest.raises(RuntimeError):
                    run.read_state()                       # the records: a synchronising copy
                torch.cuda.set_sync_debug_mode(before)
                st = run.pool.state.cpu().tolist()         # ... exempted by hand
                assert run.learn_pending == (ms[-1][-1] > 0)
                n_reads = len(learns)
                if run.learn_pending:
                    torch.cuda.set_sync_debug_mode("error")
                    run._learn()                           # the read of learn_entry exempted inside; the step's launches run under the mode
                    torch.cuda.set_sync_debug_mode(before)
                assert len(learns) == n_reads + (ms[-1][-1] > 0) and not run.learn_pending
        finally:
            torch.cuda.set_sync_debug_mode(before)
            run.close()
        if threshold == 1.0:
            assert len(ms) == 2 and all(len(m) == 4 and m[3] == sum(m[:3]) for m in ms) and max(m[3] for m in ms) >= 1
            assert len(learns) >= 1 and run.online_steps == sum(n > 0 for n in learns) >= 1
            assert all(len(e) == 4 and e[3] == sum(e[:3]) for e in [run.learn_e])
        else:
            assert [m[-1] for m in ms] == [0, 0] and learns == [] and run.online_steps == 0
        run.check_status()


# ---- 7. repack="device" -----------------------------------------------------------------------------------------------------------------
def test_the_pool_in_device_mode_equals_its_twin_on_a_mode_1_engine():
    host, run = pool_runs("device")
    assert run[4]._eng().repack_mode == "host"               # the run puts the engine's mode back
    assert_pool_equals_twin(host, run)


def test_a_refused_learn_row_raises_with_the_next_records_and_names_the_round_that_learnt():
    run = online_run(2, repack="device", K=1)
    try:
        for s in range(2):
            run.admit(s, s)
        run.launch_roots([0, 1])
        st = run.read_state()
        entries, _, _ = plan_round(st, 1, 9)
        run.launch_round(entries)
        decided = (run.P.amb[0] == 0).nonzero().view(-1)
        assert decided.numel() > 0, "toy_kw's root has no decided node: the test cannot name one"
        run.learn_kw[0] = int(decided[0])                     # the first learn row names a decided node of its row: the step refuses it
        st = run.read_state()                                 # round 1's step is issued; nothing is raised in its round
        assert run.learn_e[-1] >= 1 and run.learn_rows[:1].cpu().tolist() == [0], "round 1 has no learn row at row 0: the plant names nothing"
        assert run.pending_step["round"] == 1 and run.online_steps == 1
        run.launch_round(plan_round(st, 1, 9)[0])
        with pytest.raises(RuntimeError, match=r"gnnb_online_step_rows refused a learn row \(status bit 3\).*learning step of round 1$"):
            run.read_state()
        assert run.round == 2 and run.pending_step is None
    finally:
        run.close()


# ---- 8. limits --------------------------------------------------------------------------------------------------------------------------
def test_a_step_refused_for_memory_names_segments_and_K(monkeypatch):
    run = online_run(2, K=1)
    try:
        for s in range(2):
            run.admit(s, s)
        run.launch_roots([0, 1])
        st = run.read_state()
        call = run.eng._call

        def no_memory(name, *args):
            if name == "gnnb_online_step_rows":
                raise RuntimeError(f"{name} failed (-4): gnnb_online_step_rows: out of device memory")      # what _lib.check raises for GNNB_E_NOMEM
            return call(name, *args)
        monkeypatch.setattr(run.eng, "_call", no_memory)
        run.launch_round(plan_round(st, 1, 9)[0])
        with pytest.raises(RuntimeError, match=r"lower segments or K \(segments \* K = 2 rows at most per step\)"):
            run.read_state()
    finally:
        monkeypatch.undo()
        run.close()


def test_limits(engine):
    """An unbound handle is GNNB_E_STATE and its sizer 0; on a live handle a workspace one byte short is GNNB_E_NOMEM, online_threshold < 1,
    a null array and every plan error GNNB_E_INVALID -- each with a message that names the entry point, with nothing written, and the
    handle stays usable."""
    fresh = ScorerEngine(None)
    host = torch.tensor([[0, 0, 1]], dtype=I32)
    pl = _lib.Plan(host.data_ptr(), host.data_ptr(), 1, 1, 1, 8)
    assert fresh.lib.gnnb_frontier_learn_jobs(fresh.h, C.byref(pl), *([None] * 5), 1, *([None] * 5), None, 0, None) == -3
    assert b"gnnb_frontier_learn_jobs" in fresh.lib.gnnb_last_error() and b"gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_learn_jobs_workspace_bytes(fresh.h, 1) == 0
    relu = bind(engine, "kwg_mlp")
    rows = learn_rows(relu, 3, 1, 3)
    wrong0 = torch.zeros(2, sum(relu), dtype=I32)
    wrong0[0] = rows["wrong"]
    case = LearnCase(engine, 2, [(0, [0]), (1, [1, 2])], rows, wrong0, 1)
    dev = engine.device
    need = engine.lib.gnnb_frontier_learn_jobs_workspace_bytes(engine.h, 3)
    assert need > 0 and engine.lib.gnnb_frontier_learn_jobs_workspace_bytes(engine.h, 0) == 0
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_learn_jobs failed \(-4\)"):
        case.run(workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    for thr in (0, -4):
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_learn_jobs failed \(-1\).*online_threshold"):
            case.run(thr=thr)
    pl2 = engine._plan(case.plan)
    assert engine.lib.gnnb_frontier_learn_jobs(engine.h, C.byref(pl2), *([None] * 5), 1, *([None] * 5), None, 0, None) == -1
    assert b"gnnb_frontier_learn_jobs: null argument" in engine.lib.gnnb_last_error()
    for bad, what in (([(0, 0, 1), (2, 1, 2)], "segment 2 outside"), ([(0, 0, 3), (1, 3, 0)], "k = 0"), ([(0, 0, 1), (1, 2, 2)], "starts at row 2"),
                      ([(0, 0, 1), (1, 1, 1)], "hold 2 rows")):
        plan = sent(dev, bad, 2, 8)
        plan.n = 3
        other = LearnCase(engine, 2, case.spec, rows, wrong0, 1)
        other.plan = plan
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_learn_jobs failed \(-1\).*" + what):
            other.run()
    assert_learn_call(case, case.run(), relu)                 # the handle stays usable
