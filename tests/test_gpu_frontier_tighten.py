"""The device frontier with tightened root bounds (``LayerGraphLP(..., tighten_root=n)`` for one job,
``FrontierJobs(jobs, tighten_root=n)`` for many) on the cases of tests/golden/exact_minima.npz: without the option a run is the run it
was; with it the root's bounds are gnnb_kw_tighten's, every child's lie inside them, every record keeps the sandwich around the exact
minimum, verdicts are never wrong, global_lb never falls, and the root's bounding synchronises nothing."""
import pytest
import torch

from gnn_branching_amd import _lib, frontier
from gnn_branching_amd.frontier import FrontierJob, FrontierJobs, FrontierRun, JobsRun, branch_and_bound_frontier
from tests import exact_minimum as E
from tests.test_gpu_exact_frontier import CASES, EPS_BAB, FIX, LR, N_ITER, check_run, choice_of, global_lb

pytestmark = pytest.mark.gpu

S = _lib
T = 20                              # iterations of the root's tightening
K, ROUNDS = 4, 12
_shared = {}


def tight_lp(case, n=T):
    if (case, n) not in _shared:
        lp = E.case_lp(case, FIX[case])
        lp.tighten_root = n
        _shared[(case, n)] = lp
    return _shared[(case, n)]


class probed:
    """Inside the block every state record a ``FrontierRun`` reads is kept, with the root's intermediate bounds (behind the first read)
    and, behind every later read, whether the intermediate bounds of every live feasible child row lie inside them."""

    def __enter__(self):
        self.orig = FrontierRun.read_state
        self.records, self.root, self.inside, self.run = [], None, [], None
        me = self

        def read_state(run):
            st = me.orig(run)
            me.records.append(list(st))
            me.run = run
            lb, ub = [t.cpu() for t in run.Ch.lb], [t.cpu() for t in run.Ch.ub]
            if me.root is None:
                me.root = ([t[0].clone() for t in lb], [t[0].clone() for t in ub])
            else:
                live = (run.Ch.live.cpu() == 1) & (run.Ch.infeasible.cpu() == 0)
                me.inside.append(all(bool((a[live] >= r).all()) and bool((b[live] <= s).all()) for a, b, r, s in zip(lb, ub, *me.root)))
            return st
        FrontierRun.read_state = read_state
        return self

    def __exit__(self, *exc):
        FrontierRun.read_state = self.orig


def run_case(lp, decision_bound=None, rounds=ROUNDS):
    trace, witness = [], []
    with probed() as p:
        res = branch_and_bound_frontier(lp, choice_of(lp), lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                        decision_bound=decision_bound, log=lambda s: None, trace=trace, witness=witness)
    return res, p, trace, witness[0]


def test_without_the_option_a_run_is_the_run_it_was():
    """kwg_mlp@0.02, K = 4, 3 rounds: an lp with tighten_root = 0 and one that has never heard of the option give the same state records
    and the same trace, exactly."""
    case = "kwg_mlp@0.02:8:3"
    plain = E.case_lp(case, FIX[case])
    del plain.tighten_root                                    # a LayerGraphLP of before the option
    a = run_case(plain, rounds=3)
    b = run_case(tight_lp(case, 0), rounds=3)
    assert a[0] == b[0] and a[1].records == b[1].records and a[2] == b[2]
    assert all(torch.equal(x, y) for x, y in zip(a[1].root[0] + a[1].root[1], b[1].root[0] + b[1].root[1]))
    assert not hasattr(a[1].run, "ws_tighten") and not hasattr(b[1].run, "ws_tighten")


@pytest.mark.parametrize("case", CASES)
def test_a_tightened_root_keeps_the_sandwich_and_its_children_inside(case):
    lp = tight_lp(case)
    res, p, trace, witness = run_case(lp)
    check_run(case, res, p.records, trace, witness, None)     # the sandwich in every record, the witness, the upper values
    for r in range(1, len(p.records)):
        assert global_lb(p.records[r]) >= global_lb(p.records[r - 1]), (case, r, "global_lb fell")
    assert all(p.inside), (case, p.inside)
    # the root's bounds are gnnb_kw_tighten's of the same domain, bit for bit, and no looser than gnnb_kw_bounds'
    eng, R = p.run.eng, sum(int(m.numel()) for m in E.root_mask(lp))
    args = (lp.layers[:-1], [lp.layers[-1]], lp.input_lb[None], lp.input_ub[None], torch.full((1, R), -1, dtype=torch.int8))
    tight, plain = eng.kw_bounds(*args, tighten=T), eng.kw_bounds(*args)
    assert all(torch.equal(x[0].cpu(), y) for x, y in zip(tight.lb + tight.ub, p.root[0] + p.root[1])), case
    assert all(bool((x >= y).all()) for x, y in zip(tight.lb, plain.lb)) and all(bool((x <= y).all()) for x, y in zip(tight.ub, plain.ub))
    ran, decided = tight.counts.cpu().tolist()[0]
    strictly = any(not torch.equal(x, y) for x, y in zip(tight.lb + tight.ub, plain.lb + plain.ub))
    print(f"{case}: tightened {ran} nodes, decided {decided}; root bound {p.records[0][S.FS_LOWEST_OPEN]}; {res[4]} after {res[2]} rounds")
    if ran == 0:
        assert not strictly, case
    if case.startswith(("kwg_mlp@0.02", "kwg_gap")):
        assert decided >= 1 and strictly, (case, ran, decided)


@pytest.mark.parametrize("side", ["above", "below", "zero"])
@pytest.mark.parametrize("case", CASES)
def test_verdicts_are_never_wrong(case, side):
    e = FIX[case]
    db = {"above": float(e["m_up"][0] + e["d"]), "below": float(e["m_lo"][0] - e["d"]), "zero": 0.0}[side]
    res, p, trace, witness = run_case(tight_lp(case), decision_bound=db)
    check_run(case, res, p.records, trace, witness, db)
    glb, gub = res[0], res[1]
    if gub < db:
        assert float(e["m_lo"][0]) < db
    if glb >= db:
        assert float(e["m_up"][0]) >= db - E.slack(db)
    if side == "above":
        assert not glb >= db, (case, "proved a bound the minimum lies below", glb, db)
    if side == "below":
        assert not gub < db, (case, "found a counter-example to a bound the minimum lies above", gub, db)


def test_the_roots_bounding_synchronises_nothing():
    """The root's gnnb_kw_tighten / gnnb_dual_ascent / gnnb_net_eval under torch.cuda.set_sync_debug_mode("error"), for one job and for
    the root phase of two; the mode is live (a read of the state record raises)."""
    case = "kwg_mlp@0.02:8:3"
    lp = tight_lp(case)
    run = FrontierRun(lp, choice_of(lp), lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB)
    run.set_tighten_root(T)
    run.root()
    want = [t[0].clone() for t in run.Ch.lb + run.Ch.ub]
    jobs = [FrontierJob(l.input_lb, l.input_ub, l.layers[-1]) for l in (lp, tight_lp("kwg_mlp@0.01:8:6"))]
    many = JobsRun(choice_of(lp), lp.layers[:-1], jobs, tuple(lp.input_lb.shape), K, 2, 17, N_ITER, LR, EPS_BAB)
    many.set_tighten_root(T)
    many.admit(0, 0)
    many.admit(1, 1)
    many.launch_roots([0, 1])
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            run.pool.state.cpu()
        for t in run.Ch.lb + run.Ch.ub:
            t.zero_()
        run._bound_children(run.Ch, 1, warm=False, tighten=T)
        many._bound_children(many.Ch, 4, warm=False, tighten=T)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(torch.equal(t[0], w) for t, w in zip(run.Ch.lb + run.Ch.ub, want))
    assert all(torch.equal(t[0], w) for t, w in zip(many.Ch.lb + many.Ch.ub, want))        # job 0 is the one-job run's root: row independence
    run.close()
    many.close()


def test_two_jobs_of_different_boxes_get_what_each_gets_alone():
    """One ``verify_properties`` call, ``FrontierJobs(jobs, tighten_root=20)``: every job's result is its own one-job run's with the same
    capacity, bit for bit, and keeps the sandwich around its own exact minimum."""
    cases = ["kwg_mlp@0.02:8:3", "kwg_mlp@0.01:2:6"]
    lps = [tight_lp(c) for c in cases]
    jobs = FrontierJobs([FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1]) for lp in lps], tighten_root=T)
    got = frontier.verify_properties(choice_of(lps[0]), lps[0].layers[:-1], jobs, K=K, segments=2, capacity=64, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                                     max_rounds=ROUNDS, log=lambda s: None)
    for case, lp, res in zip(cases, lps, got):
        alone = branch_and_bound_frontier(lp, choice_of(lp), lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, capacity=64,
                                          log=lambda s: None)
        assert tuple(res) == tuple(alone), (case, res, alone)
        m_lo, m_up = float(FIX[case]["m_lo"][0]), float(FIX[case]["m_up"][0])
        assert res[0] <= m_up + E.slack(m_up) and res[1] >= m_lo - E.slack(m_lo), (case, res)
    off = frontier.verify_properties(choice_of(lps[0]), lps[0].layers[:-1], list(jobs), K=K, segments=2, capacity=64, n_iter=N_ITER, lr=LR,
                                     eps=EPS_BAB, max_rounds=ROUNDS, log=lambda s: None)
    assert [tuple(r) for r in off] != [tuple(r) for r in got]     # the option reaches the run: the tightened roots start from other bounds


def test_bad_values_are_refused():
    lp = tight_lp("kwg_mlp@0.02:8:3", 0)
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            frontier._check_tighten(bad)
        with pytest.raises(ValueError):
            type(lp)(lp.layers, lp.input_lb, lp.input_ub, tighten_root=bad)
