"""CPU: the witness of the upper bound and the descent on the network.  The entry points gnnb_net_descend /
gnnb_frontier_witness / gnnb_frontier_witness_jobs are declared, bound and exported, their kernels have one profile class each, they refuse
a null handle and every value outside its range with a message that names them and the value; the three loops reject bad options before
they touch a device; and the fp64 twin of tests/test_gpu_net_descend.py meets its own conditions on the seeds that file uses.  (A handle
needs a GPU to exist: the other refusals are in the two GPU files.)"""
import ctypes as C

import pytest

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_net_descend_workspace_bytes", "gnnb_net_descend", "gnnb_frontier_witness", "gnnb_frontier_witness_jobs")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def descend(lib, h, B=2, n_steps=1, step=0.5):
    return lib.gnnb_net_descend(h, *([None] * 5), B, n_steps, step, *([None] * 4), None, 0, None)


def witness(lib, h, K=2, m=0):
    return lib.gnnb_frontier_witness(h, K, C.byref(_lib.Children()), C.byref(_lib.WitnessSrc(None, None, None, None, m)), None, None, None)


def witness_jobs(lib, h, n_entries=1, n=2, M=0):
    plan = _lib.Plan(None, None, n_entries, n, 1, 8)
    return lib.gnnb_frontier_witness_jobs(h, C.byref(plan), M, None, C.byref(_lib.Children()), C.byref(_lib.WitnessSrc()), None, None, None)


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert "} gnnb_witness_src;" in header
    assert lib.gnnb_abi_version() == 2                       # the additions are additive
    assert "#define GNNB_ABI_VERSION 2" in header and "#define GNNB_FRONTIER_STATE_DOUBLES 9" in header
    assert _lib.FRONTIER_STATE_DOUBLES == 9
    from gnn_branching_amd.engine import ScorerEngine
    for m in ("net_descend", "frontier_witness", "frontier_witness_jobs"):
        assert callable(getattr(ScorerEngine, m)), m


def test_every_new_kernel_has_one_profile_class_and_no_name_is_doubled(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in ("k_net_descend", "k_frontier_witness", "k_frontier_witness_jobs", "k_net_eval"):
        assert classes.count(k) == 1, k
    assert len(set(classes)) == len(classes) and "" not in classes


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in (("gnnb_net_descend", lambda: descend(lib, None)), ("gnnb_frontier_witness", lambda: witness(lib, None)),
                       ("gnnb_frontier_witness_jobs", lambda: witness_jobs(lib, None))):
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() + b":" in msg and b"null handle" in msg, (name, msg)
    assert lib.gnnb_net_descend_workspace_bytes(None, 4) == 0


@pytest.mark.parametrize("kw,word", [({"B": 0}, "B = 0"), ({"B": -2}, "B = -2"), ({"n_steps": -1}, "n_steps = -1"), ({"step": 0.0}, "step = 0"),
                                     ({"step": -0.25}, "step = -0.25"), ({"step": 1.5}, "step = 1.5"), ({"step": float("nan")}, "step = nan"),
                                     ({"step": float("inf")}, "step = inf")])
def test_descend_refuses_values_outside_their_ranges_with_a_message(lib, kw, word):
    assert descend(lib, None, **kw) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_net_descend:" in msg and word.encode() in msg and b"null handle" not in msg, msg


@pytest.mark.parametrize("K,m,word", [(0, 0, "K = 0"), (-3, 0, "K = -3"), (32768, 0, "K = 32768"), (4, -1, "m = -1"), (4, 5, "m = 5")])
def test_witness_refuses_values_outside_their_ranges_with_a_message(lib, K, m, word):
    assert witness(lib, None, K, m) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_witness:" in msg and word.encode() in msg and b"null handle" not in msg, msg


@pytest.mark.parametrize("n_entries,n,M,word", [(1, 0, 0, "n = 0 "), (1, -3, 0, "n = -3 "), (0, 2, 0, "0 plan entries"), (1, 32768, 0, "n = 32768 "),
                                                (1, 4, -1, "M = -1"), (1, 4, 5, "M = 5")])
def test_witness_jobs_refuses_values_outside_their_ranges_with_a_message(lib, n_entries, n, M, word):
    assert witness_jobs(lib, None, n_entries, n, M) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_witness_jobs:" in msg and word.encode() in msg and b"null handle" not in msg, msg


def test_a_null_plan_is_refused(lib):
    assert lib.gnnb_frontier_witness_jobs(None, None, 0, None, None, None, None, None, None) == -1
    assert b"gnnb_frontier_witness_jobs: null plan" in lib.gnnb_last_error()


BAD = [{"witness": ()}, {"witness": True}, {"witness": "x"}, {"witness": {}},                                    # not None, not a list
       {"pgd_steps": -1}, {"pgd_steps": True}, {"pgd_steps": False}, {"pgd_steps": 2.0}, {"pgd_steps": "4"},     # not None, not an integer >= 0
       {"pgd_step": 0}, {"pgd_step": 0.0}, {"pgd_step": -0.5}, {"pgd_step": 1.5}, {"pgd_step": True}, {"pgd_step": None},
       {"pgd_step": float("nan")}, {"pgd_steps": 4, "pgd_step": 2}]


@pytest.mark.parametrize("kw", BAD)
def test_bad_options_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, **kw)
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, branching_threshold=0.5, **kw)
    with pytest.raises(ValueError):
        frontier.FrontierRun(NoDevice(), NoDevice(), [], K=4, **kw)
    with pytest.raises(ValueError):
        frontier.verify_properties(NoDevice(), [], frontier.FrontierJobs([job()], **kw), K=4)
    with pytest.raises(ValueError):
        frontier.verify_properties_threshold(NoDevice(), [], frontier.FrontierJobs([job()], **kw), 0.5, K=4)


def test_the_jobs_loops_take_the_options_on_their_jobs():
    """``FrontierJobs`` is a list of jobs with the run's options; any other sequence of jobs runs with everything off."""
    point = []
    jobs = frontier.FrontierJobs([job(), job()], witness=point, pgd_steps=4, pgd_step=0.25)
    assert isinstance(jobs, list) and len(jobs) == 2
    off = {"pgd_restarts": None, "pgd_seed": 0}              # (the restart options, tests/test_net_starts_cpu.py)
    assert frontier._options_of(jobs) == {"witness": point, "pgd_steps": 4, "pgd_step": 0.25, **off} and frontier._options_of(jobs)["witness"] is point
    assert frontier._options_of(list(jobs)) == {} and frontier._options_of(frontier.FrontierJobs([job()])) == {"witness": None, "pgd_steps": None,
                                                                                                              "pgd_step": 1.0 / 64, **off}


def test_good_options_pass_the_check():
    for kw in ({}, {"witness": []}, {"pgd_steps": 0}, {"pgd_steps": 16, "pgd_step": 1}, {"witness": [], "pgd_steps": 4, "pgd_step": 1.0 / 64}):
        frontier._check_witness(kw.get("witness"), kw.get("pgd_steps"), kw.get("pgd_step", frontier.PGD_STEP_DEFAULT))
    assert frontier.PGD_STEP_DEFAULT == 1.0 / 64


@pytest.mark.parametrize("B", [5, 1])
def test_the_twin_meets_its_own_conditions_on_the_chosen_seeds(B):
    """tests/test_gpu_net_descend.py holds the device to signs and step counts of its fp64 twin; the twin asserts that none of them hangs on
    rounding (pre-activations, gradient entries, consecutive values) and that the first step lowers f by 1e-6.  Checked here without a GPU."""
    from tests import test_gpu_net_descend as t
    for name in t.NETS:
        out = t.twin_conditions(name, B)
        assert all(1 <= o[2] <= 8 and o[1] <= o[3] for o in out), name
        if B == 5:
            t.big_step_twin(name)
