"""The device frontier run to a stop reason against certified exact minima (tests/golden/exact_minima.npz; tests/exact_minimum.py).
Every assertion holds for any correct branch and bound, whatever it decides to branch on: a sandwich around the truth in every state
record of every run, a witness that is what it claims to be, and verdicts that are never wrong.  None asserts convergence the algorithm
does not promise -- a fully split leaf is bounded by 20 ascent steps, not by an exact LP, so global_lb need not reach the minimum -- but
for one budget: a BaBSR run decides within four times the branches a best-first host loop of the same pieces needs.

Every run's reason, rounds and final bounds are printed as one "EXACT-RUN {json}" line (profiles/exact_minima_runs.json is a copy of
one GPU run's lines)."""
import json
import math

import pytest

from gnn_branching_amd import _lib, frontier
from gnn_branching_amd.frontier import FrontierJob, FrontierRun, JobsRun, branch_and_bound_frontier
from tests import exact_minimum as E
from tests.frontier_twin import CKPT

pytestmark = pytest.mark.gpu

S = _lib
FIX = E.load()
CASES = list(FIX)
REASONS = {"exhausted", "gap", "decision", "max_rounds", "capacity"}
N_ITER, LR, EPS_BAB = 20, 0.1, 1e-4
BRANCHES = 192                      # a run's budget: max_rounds * K
# name -> (K, keywords of branch_and_bound_frontier)
MODES = {
    "gnn_k1": (1, {}),
    "gnn_k16": (16, {}),
    "babsr": (4, {"branching": "babsr"}),
    "strong8": (2, {"branching": "strong", "strong_candidates": 8}),
    "threshold": (4, {"branching_threshold": 0.2}),
    "gnn_pgd": (4, {"pgd_steps": 4, "pgd_restarts": 3}),
}
_shared = {}


def choice_of(lp):
    from gnn_branching_amd import bab_caller
    key = tuple(int(m.numel()) for m in E.root_mask(lp))
    if key not in _shared:
        c = bab_caller.BatchedGraphChoice(E.root_mask(lp), CKPT)
        c.verbose = False
        _shared[key] = c
    return _shared[key]


def case_lp(case):
    if ("lp", case) not in _shared:
        _shared[("lp", case)] = E.case_lp(case, FIX[case])
    return _shared[("lp", case)]


class recorded:
    """Inside the block every state record a run reads (``FrontierRun.read_state`` / ``JobsRun.read_state``) is also appended to
    ``records``: the loop under test is the library's own, untouched."""

    def __init__(self, cls=FrontierRun, trace=None):
        self.cls, self.records, self.trace, self.seen = cls, [], trace, []      # seen[i]: entries in ``trace`` when record i was read

    def __enter__(self):
        self.orig = self.cls.read_state
        records, orig, me = self.records, self.orig, self

        def read_state(run):
            st = orig(run)
            me.seen.append(0 if me.trace is None else len(me.trace))
            records.append([list(r) for r in st] if st and isinstance(st[0], (list, tuple)) else list(st))
            return st
        self.cls.read_state = read_state
        return self.records

    def __exit__(self, *exc):
        self.cls.read_state = self.orig


def global_lb(st):
    return min(st[S.FS_LOWEST_OPEN], st[S.FS_CLOSED_LB], st[S.FS_GLOBAL_UB])


def run_case(case, mode, decision_bound=None, capacity=None, max_rounds=None, K=None, **extra):
    """One run of ``branch_and_bound_frontier`` with its trace and every state record; the checks every run gets (``check_run``)."""
    lp, e = case_lp(case), FIX[case]
    k, kw = MODES[mode]
    K = k if K is None else K
    kw = {**kw, **extra}
    rounds = max(1, BRANCHES // K) if max_rounds is None else max_rounds
    trace, witness = [], []
    with recorded() as records:
        res = branch_and_bound_frontier(lp, choice_of(lp), lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, decision_bound=decision_bound,
                                        capacity=capacity, log=lambda s: None, trace=trace, witness=witness, **kw)
    out = {"case": case, "mode": mode, "K": K, "decision_bound": decision_bound, "capacity": capacity, "reason": res[4], "rounds": res[2],
           "domains_bounded": res[3], "global_lb": res[0], "global_ub": res[1], "m_lo": float(e["m_lo"][0]), "m_up": float(e["m_up"][0])}
    print("EXACT-RUN " + json.dumps(out))
    check_run(case, res, records, trace, witness[0], decision_bound)
    if decision_bound is None and capacity is None and max_rounds is None and not extra:
        _shared[("run", case, mode)] = records
    return res, records, trace, witness[0]


def check_run(case, res, records, trace, witness, decision_bound):
    lp, e = case_lp(case), FIX[case]
    m_lo, m_up = float(e["m_lo"][0]), float(e["m_up"][0])
    sl = E.slack(m_up)
    glb, gub, rounds, _, reason = res
    assert reason in REASONS, reason
    assert len(records) == rounds + 1 and len(trace) == rounds
    # every round: the sandwich; the upper bound and the closed leaves' bound only tighten
    prev = None
    for r, st in enumerate(records):
        lb, ub = global_lb(st), st[S.FS_GLOBAL_UB]
        assert lb <= m_up + sl, (case, r, "global_lb above the exact minimum", lb, m_up)
        assert ub >= m_lo - sl, (case, r, "global_ub below the exact minimum", ub, m_lo)
        # (the minimum over the open bounds, closed_lb and global_ub IS global_lb: no part of it may hide above the truth alone)
        assert min(st[S.FS_LOWEST_OPEN], st[S.FS_CLOSED_LB]) <= m_up + sl or ub <= m_up + sl, (case, r, st)
        if prev is not None:                                      # (global_lb from round to round: test_global_lb_never_falls)
            assert ub <= prev[S.FS_GLOBAL_UB], (case, r, "global_ub rose", prev[S.FS_GLOBAL_UB], ub)
            assert st[S.FS_CLOSED_LB] <= prev[S.FS_CLOSED_LB], (case, r, "closed_lb rose")
        prev = st
    assert (glb, gub) == (global_lb(records[-1]), records[-1][S.FS_GLOBAL_UB])
    # every upper value a round reports is the network's value at a point of the box
    for r, t in enumerate(trace):
        for c, ub in enumerate(t["child_ub"]):
            if t["live"][c] and not t["infeasible"][c]:
                assert ub >= m_lo - sl, (case, r, c, "a child's upper value below the exact minimum", ub, m_lo)
    # the witness is a point of the box and global_ub is the network there
    if math.isinf(gub):
        assert witness is None
    else:
        x = witness.double()
        assert bool((x >= lp.input_lb).all()) and bool((x <= lp.input_ub).all()), (case, "witness outside the box")
        v = float(E.net_value(lp, x)[0])
        assert abs(v - gub) <= 1e-9 * max(1.0, abs(v)), (case, "global_ub is not the network at the witness", v, gub)
        assert v >= m_lo - sl
    if reason == "decision":
        assert decision_bound is not None
        if gub < decision_bound:                                  # a counter-example: it must be a real one, and the truth on its side
            assert m_lo - sl < decision_bound, (case, "decided below a bound the exact minimum is not below", decision_bound, m_lo)
            assert float(E.net_value(lp, witness.double())[0]) < decision_bound
        else:
            # (no run takes this branch: a child at or above the bound is closed, never kept, so while a domain is open global_lb is
            # below the bound, and with none open the reason is "exhausted"; test_verdicts_are_never_wrong holds the final bounds to
            # the truth under every reason)
            assert glb >= decision_bound
            assert m_up + sl >= decision_bound, (case, "proved a bound the exact minimum is below", decision_bound, m_up)


GNN_CASES = CASES                    # every network of the fixture binds the scorer (they are geometries of tests/common.py FWD_ARCHS)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", GNN_CASES)
def test_every_round_keeps_the_sandwich(case, mode):
    res, records, trace, witness = run_case(case, mode)
    # (without a decision bound a run stops for no decision)
    assert res[4] != "decision"


def test_global_lb_never_falls():
    """global_lb is monotone non-decreasing from record to record, in every mode on every case (the runs of
    test_every_round_keeps_the_sandwich, run here where that test has not).

    This test found what the twins could not: before ``_Round._at_least_the_parent_s`` 18 of these 60 runs reported a global_lb below
    the one of the record before, in 65 records, by one unit in the last place up to 2.6e-4 (kwg_mlp@0.02:2:6 babsr, round 2:
    -0.48072420838 -> -0.48098427690), median 1.9e-5 -- sound every time, but not monotone.  A child is bounded by 20 ascent steps from
    its parent's dual point with the split node's new multiplier beta at 0, and the child's dual function there can lie below the
    parent's bound: on the fp64 host twin (``kw_bounds`` with the parent, ``dual_ascent_host`` from the parent's alpha and beta) 5.3e-3
    below for the blocked child of node 39 of ReLU layer 1 at the root of kwg_mlp@0.01:2:6, and still 3.35e-5 below after the 20 steps,
    which was the device's fall in round 1 of that case to the digit.  A round now raises such a child's bound to its parent's, which
    holds for every part of the parent, before anything reads it."""
    falls, runs = [], 0
    for case in GNN_CASES:
        for mode in MODES:
            if ("run", case, mode) not in _shared:
                run_case(case, mode)
            records = _shared[("run", case, mode)]
            runs += 1
            for r in range(1, len(records)):
                a, b = global_lb(records[r - 1]), global_lb(records[r])
                if b < a:
                    falls.append((case, mode, r, a, b))
    for f in falls:
        print("global_lb fell:", f)
    print(f"{len({f[:2] for f in falls})} of {runs} runs, {len(falls)} records")
    assert not falls, falls[:10]


@pytest.mark.parametrize("mode", ["gnn_k16", "babsr"])
@pytest.mark.parametrize("side", ["above", "below", "zero"])
@pytest.mark.parametrize("case", CASES)
def test_verdicts_are_never_wrong(case, side, mode):
    """decision_bound = m_up + d (the minimum is below it), m_lo - d (it is above) and 0: ``check_run`` holds a "decision" to the truth."""
    e = FIX[case]
    db = {"above": float(e["m_up"][0] + e["d"]), "below": float(e["m_lo"][0] - e["d"]), "zero": 0.0}[side]
    res, records, trace, witness = run_case(case, mode, decision_bound=db)
    glb, gub, reason = res[0], res[1], res[4]
    # whatever the reason, final bounds that decide decide rightly (the sandwich says so; stated once more on the verdict itself)
    if gub < db:
        assert float(e["m_lo"][0]) < db
    if glb >= db:
        assert float(e["m_up"][0]) >= db - E.slack(db)
    if side == "above":
        assert not glb >= db, (case, "proved a bound the minimum lies below", glb, db)
    if side == "below":
        assert not gub < db, (case, "found a counter-example to a bound the minimum lies above", gub, db)


REACH = [(c, i) for c in CASES for i in (0, 1) if 0 <= int(FIX[c]["n_host"][i]) <= E.N_HOST_MAX]


@pytest.mark.parametrize("case,which", REACH)
def test_verdicts_are_reached_within_four_times_the_host_loop_s_branches(case, which):
    """decision_bound = m_lo - d (which = 0) or 0 (which = 1): a best-first host loop of kw_bounds with parent intersection, 20 cold ascent
    steps and the BaBSR rule (tests/exact_minimum.py host_loop) decided after n_host branches.  The device "babsr" run with the same
    rule's arguments gets max_rounds * K = 4 n_host branches: K parents per round are not best-first, and the device warm-starts where
    the host loop does not.  Its final bounds must decide -- under whichever stop reason: a pool without an open domain reports
    "exhausted" before it looks at the decision bound."""
    e = FIX[case]
    n_host = int(e["n_host"][which])
    db = (float(e["m_lo"][0] - e["d"]), 0.0)[which]
    K = 4
    rounds = math.ceil(4 * n_host / K)
    res, records, trace, witness = run_case(case, "babsr", decision_bound=db, max_rounds=rounds, K=K, sparsest_layer=-1)
    glb, gub, reason = res[0], res[1], res[4]
    print(f"{case} to {db}: host {n_host} branches; device {res[2]} rounds of {K}, {reason}, lb {glb} ub {gub}")
    assert glb >= db or gub < db, (case, db, n_host, res)
    assert (glb >= db) == (float(e["m_up"][0]) >= db)


@pytest.mark.parametrize("case", CASES)
def test_pool_pressure_keeps_the_sandwich(case):
    """K = 16 again in a pool of 4K + 1 slots: it compacts often and may stop with "capacity"; every record keeps the sandwich
    (``check_run``).  Up to its stop the tight run IS the roomy run (the picks depend on bounds and slot order, and a compaction keeps
    the slot order), so its records are the roomy run's first records and its final global_lb is no higher than the roomy run's."""
    compactions, orig = [], frontier.DomainPool.compact

    def counting(self, n_open):
        compactions.append(n_open)
        return orig(self, n_open)
    roomy = run_case(case, "gnn_k16")
    frontier.DomainPool.compact = counting
    try:
        tight = run_case(case, "gnn_k16", capacity=4 * 16 + 1)
    finally:
        frontier.DomainPool.compact = orig
    print(f"{case}: roomy {roomy[0]}, tight {tight[0]}, {len(compactions)} compactions")
    n = len(tight[1])
    assert n <= len(roomy[1])
    for a, b in zip(tight[1], roomy[1][:n]):
        for key in (S.FS_GLOBAL_UB, S.FS_CLOSED_LB, S.FS_LOWEST_OPEN, S.FS_N_OPEN):
            assert a[key] == b[key], (case, key, a, b)
    assert tight[0][0] <= roomy[0][0]
    if tight[0][4] != "capacity":
        assert tight[0] == roomy[0]


# ---- many jobs in one pool -------------------------------------------------------------------------------------------------------------
JOB_CASES = [c for c in CASES if c.startswith("kwg_mlp@")]       # one network, two boxes (eps 0.01 and 0.02), two properties each


def jobs_of(decision_bound):
    lps = [case_lp(c) for c in JOB_CASES]
    return lps, [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], decision_bound) for lp in lps]


RUNNERS = {
    "gnn": lambda choice, fixed, jobs, **kw: frontier.verify_properties(choice, fixed, jobs, **kw),
    "babsr": lambda choice, fixed, jobs, **kw: frontier.verify_properties_babsr(choice, fixed, jobs, **kw),
    "threshold": lambda choice, fixed, jobs, **kw: frontier.verify_properties_threshold(choice, fixed, jobs, 0.2, **kw),
    "strong8": lambda choice, fixed, jobs, **kw: frontier.verify_properties_strong(choice, fixed, jobs, strong_candidates=8, **kw),
}


@pytest.mark.parametrize("decision_bound", [None, 0.0])
@pytest.mark.parametrize("runner", list(RUNNERS))
def test_many_jobs_each_against_its_own_truth(runner, decision_bound):
    """Four jobs in two segments -- a segment is released and used again --, K = 4, pools of 4K + 1 slots.  A round's trace entries
    (appended before the round's records are read) say which job a segment held, so every record a job's segment shows behind one of
    the job's rounds is held to that job's own truth: the sandwich, global_ub and closed_lb that only fall, and global_lb that never
    falls.  Every traced upper value is at least its job's exact minimum, the final bounds keep the sandwich, and a "decision" at bound 0
    carries the sign of the exact minimum.  (The record behind a job's root phase is not traced; the job's first round follows it.)"""
    assert len(JOB_CASES) == 4
    lps, jobs = jobs_of(decision_bound)
    K, cap = 4, 17
    trace = []
    rec = recorded(JobsRun, trace)
    with rec as records:
        got = RUNNERS[runner](choice_of(lps[0]), lps[0].layers[:-1], jobs, K=K, segments=2, capacity=cap, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                              max_rounds=24, log=lambda s: None, trace=trace)
    assert len(got) == 4 and {t["job"] for t in trace} <= {0, 1, 2, 3} and {t["segment"] for t in trace} <= {0, 1}
    truth = [(float(FIX[c]["m_lo"][0]), float(FIX[c]["m_up"][0])) for c in JOB_CASES]
    per_job, before = {j: [] for j in range(4)}, 0
    for st, n in zip(records, rec.seen):                      # the entries a read follows are the round's
        for t in trace[before:n]:
            per_job[t["job"]].append((t["round"], st[t["segment"]]))
        before = n
    assert before == len(trace)
    for j, (case, res) in enumerate(zip(JOB_CASES, got)):
        m_lo, m_up = truth[j]
        sl = E.slack(m_up)
        glb, gub, rounds, _, reason = res
        print("EXACT-RUN " + json.dumps({"case": case, "mode": "jobs_" + runner, "K": K, "decision_bound": decision_bound, "capacity": cap,
                                         "reason": reason, "rounds": rounds, "domains_bounded": res[3], "global_lb": glb, "global_ub": gub,
                                         "m_lo": m_lo, "m_up": m_up}))
        assert reason in REASONS, (case, reason)
        assert glb <= m_up + sl and gub >= m_lo - sl, (case, res, m_lo, m_up)
        assert [r for r, _ in per_job[j]] == list(range(rounds)), (case, rounds)
        prev = None
        for r, seg in per_job[j]:
            lb, ub = global_lb(seg), seg[S.FS_GLOBAL_UB]
            assert lb <= m_up + sl, (case, r, "global_lb above the job's exact minimum", lb, m_up)
            assert ub >= m_lo - sl, (case, r, "global_ub below the job's exact minimum", ub, m_lo)
            if prev is not None:
                assert lb >= global_lb(prev) and ub <= prev[S.FS_GLOBAL_UB] and seg[S.FS_CLOSED_LB] <= prev[S.FS_CLOSED_LB], (case, r, prev, seg)
            prev = seg
        if prev is not None:                                  # the job's last record is its result
            assert (glb, gub) == (global_lb(prev), prev[S.FS_GLOBAL_UB]), (case, res, prev)
        for t in trace:
            if t["job"] != j:
                continue
            for c, ub in enumerate(t["child_ub"]):
                if t["live"][c] and not t["infeasible"][c]:
                    assert ub >= m_lo - sl, (case, t["round"], c, ub, m_lo)
        if reason == "decision":
            assert (gub < 0.0) == (m_up < 0.0) and (glb >= 0.0) == (m_lo >= 0.0), (case, res)
    assert any(len(v) for v in per_job.values())
