"""The upper bound from many starts inside the device frontier, on the MI355X:
``branch_and_bound_frontier(pgd_steps=..., pgd_restarts=..., pgd_seed=...)`` on toy_kw, property (2, 6), eps 0.04 (the runs of
tests/test_gpu_frontier_witness.py): the device's incumbent against the state record every round, the point against the network, soundness,
the root's bound against the run without restarts, the option off against the launches of a round as they were, repeats, and
``verify_properties`` / ``verify_properties_threshold``: every job's result and witness against its run alone -- what the row key is for."""
import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib as S
from gnn_branching_amd.frontier import FrontierJob, FrontierJobs, FrontierRun, branch_and_bound_frontier, verify_properties, verify_properties_threshold
from tests.frontier_twin import EPS_BAB, LR, N_ITER, engine, toy  # noqa: F401  (engine: the module fixture)
from tests.test_gpu_frontier_witness import value64

pytestmark = pytest.mark.gpu

NEW_CLASSES = ("k_net_starts", "k_net_descend_tile", "k_net_starts_pick")
RESTARTS = 3
_runs = {}


def toy_run(K, rounds, threshold=None, pgd=4, restarts=RESTARTS, seed=0, repeat=0):
    key = (K, rounds, threshold, pgd, restarts, seed, repeat)
    if key not in _runs:
        lp, choice, _ = toy()
        trace, point = [], []
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace,
                                        branching_threshold=threshold, witness=point, pgd_steps=pgd, pgd_restarts=restarts, pgd_seed=seed)
        _runs[key] = (res, trace, point)
    return _runs[key]


@pytest.mark.parametrize("pgd", [4, 0])
@pytest.mark.parametrize("threshold", [None, 1.0])
@pytest.mark.parametrize("K,rounds", [(1, 4), (4, 5)])
def test_the_witness_is_the_point_of_global_ub(K, rounds, threshold, pgd):
    lp, choice, _ = toy()
    res, trace, point = toy_run(K, rounds, threshold, pgd)
    global_lb, global_ub = res[0], res[1]
    assert len(trace) >= 1 and len(point) == 1 and point[0] is not None
    for r, row in enumerate(trace):                                     # best_value == the record's global_ub, every round: the same bits
        assert row["witness_value"] == row["global_ub"], (r, row["witness_value"], row["global_ub"])
    assert trace[-1]["global_ub"] == global_ub
    x = point[0]
    assert x.dtype == torch.float32 and x.device.type == "cpu" and tuple(x.shape) == tuple(lp.input_lb.shape)
    eng = choice.model.engine()
    on_device = float(eng.net_eval(lp.layers[:-1], [lp.layers[-1]], x[None].to(eng.device)).cpu()[0])
    assert on_device == global_ub, (on_device, global_ub)               # gnnb_net_eval(witness), bit for bit
    f64 = value64(lp, x)
    assert abs(f64 - global_ub) <= 1e-9, (f64, global_ub)
    assert bool((x >= lp.input_lb.float().cpu()).all()) and bool((x <= lp.input_ub.float().cpu()).all())
    rng = np.random.RandomState(3)                                      # soundness: global_lb below the network everywhere we look
    lo, hi = lp.input_lb.double().cpu(), lp.input_ub.double().cpu()
    for _ in range(16):
        s = (lo + (hi - lo) * torch.from_numpy(rng.uniform(0, 1, tuple(lo.shape)))).float()
        assert global_lb <= value64(lp, s) + 1e-9
    assert global_lb <= f64 + 1e-9


@pytest.mark.parametrize("pgd", [4, 0])
def test_restarts_do_not_raise_the_root_s_upper_bound(pgd):
    """The root child is the same and its start 0 is the same trajectory: the least over the starts is at most the run's without restarts."""
    with_r, without = toy_run(4, 0, None, pgd), toy_run(4, 0, None, pgd, restarts=None)
    print(f"root global_ub pgd_steps {pgd}: without restarts {without[0][1]!r}, with {RESTARTS} {with_r[0][1]!r}")
    assert with_r[0][1] <= without[0][1] and with_r[0][2] == 0
    assert with_r[0][0] == without[0][0]                                # (the lower bound does not see the option)


@pytest.mark.parametrize("threshold", [None, 1.0])
def test_no_restarts_is_the_run_without_the_option(threshold):
    """pgd_restarts = 0 and None: the pgd_steps-only run's five-tuple, trace and witness, bit for bit."""
    plain = toy_run(4, 5, threshold, 4, restarts=None)
    zero = toy_run(4, 5, threshold, 4, restarts=0)
    assert zero[0] == plain[0] and zero[1] == plain[1] and len(plain[1]) >= 2 and torch.equal(zero[2][0], plain[2][0])
    seeded = toy_run(4, 5, threshold, 4, restarts=0, seed=99)          # (without restarts the seed is not read)
    assert seeded[0] == plain[0] and seeded[1] == plain[1]


@pytest.mark.parametrize("threshold", [None, 1.0])
def test_a_run_repeats_itself_and_the_seed_is_read(threshold):
    a, b = toy_run(4, 5, threshold), toy_run(4, 5, threshold, repeat=1)
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2][0], b[2][0])
    other = toy_run(4, 5, threshold, seed=2 ** 64 - 1)
    print("global_ub per round, seed 0", [row["global_ub"] for row in a[1]], "seed 2^64 - 1", [row["global_ub"] for row in other[1]])
    assert other[0][0] <= other[0][1]


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
def test_the_option_off_launches_none_of_the_new_kernels(threshold):
    for off_kw in ({}, {"pgd_steps": 0}, {"pgd_steps": 0, "pgd_restarts": 0}, {"pgd_steps": 0, "pgd_restarts": None, "pgd_seed": 5}):
        off = launches(threshold, **off_kw)
        assert not set(off) & set(NEW_CLASSES), (off_kw, set(off) & set(NEW_CLASSES))
    off = launches(threshold, pgd_steps=4)
    on = launches(threshold, pgd_steps=4, pgd_restarts=RESTARTS)
    assert "k_net_descend" in off and "k_net_descend" not in on and "k_net_eval" not in on
    # the two launches (three kernels) in gnnb_net_descend's place, for the root and both pairs: the root's, then per set of children
    assert on.count("k_net_starts") == on.count("k_net_descend_tile") == on.count("k_net_starts_pick") >= 3
    assert on.index("k_net_starts") < on.index("k_net_descend_tile") < on.index("k_net_starts_pick")
    if on.count("k_net_starts") == off.count("k_net_descend"):          # (the same rounds: nothing else moved)
        assert [k for k in on if k not in NEW_CLASSES] == [k for k in off if k != "k_net_descend"]


@pytest.mark.parametrize("threshold", [None, 1.0])
def test_every_job_is_what_it_gets_alone(threshold):
    """Three jobs in two segments (the third is admitted late, into a reused segment) with pgd_steps 4 and 3 restarts: bounds, counts and
    witnesses bit-equal to the runs alone.  A job's rows sit at other indices of larger batches in the pool: their start points do not see it."""
    from tests.test_gpu_frontier_jobs import JOBS, toy_jobs
    choice, lps = toy_jobs()
    K, cap, rounds = 2, 9, 3
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], db) for lp, (_, _, _, db) in zip(lps[:3], JOBS)]
    alone, alone_points = [], []
    for lp, job in zip(lps, jobs):
        kw = {} if threshold is None else {"branching_threshold": threshold}
        alone.append(branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, capacity=cap,
                                               decision_bound=job.decision_bound, log=lambda s: None, witness=alone_points, pgd_steps=4,
                                               pgd_restarts=RESTARTS, **kw))
    points, trace = [], []
    jobs = FrontierJobs(jobs, witness=points, pgd_steps=4, pgd_restarts=RESTARTS)
    common = dict(K=K, segments=2, capacity=cap, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace)
    if threshold is None:
        got = verify_properties(choice, lps[0].layers[:-1], jobs, **common)
    else:
        got = verify_properties_threshold(choice, lps[0].layers[:-1], jobs, threshold, **common)
    assert len(points) == len(alone_points) == 3
    assert any(row["job"] == 2 for row in trace)
    for row in trace:
        assert row["witness_value"] == row["global_ub"], row["job"]
    for j in range(3):
        print("job", j, "alone", alone[j], "together", got[j])
        assert got[j] == alone[j], j
        assert (points[j] is None) == (alone_points[j] is None), j
        if points[j] is not None:
            assert torch.equal(points[j], alone_points[j]), j
    assert any(p is not None for p in points)


def test_a_round_with_restarts_copies_nothing_but_the_state_record():
    """Two rounds under torch.cuda.set_sync_debug_mode("error"): the read of the state record is the one exemption."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy()
    run = FrontierRun(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, witness=[], pgd_steps=4, pgd_restarts=RESTARTS)
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
            with pytest.raises(RuntimeError):
                run.read_state()
            torch.cuda.set_sync_debug_mode(before)
            st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert float(run.best_value.cpu()[0]) == st[S.FS_GLOBAL_UB]
    run.check_status()
