"""CPU: branching on the BaBSR heuristic alone inside the device-resident frontier.  The entry points
gnnb_frontier_babsr_decide / _decide_jobs and their workspace sizer are declared, bound and exported, their kernels have one profile class
each and every older frontier class stays single, no option was added; they refuse a null handle, K outside 1..32767, n_order outside 0..8,
a NaN decision threshold and a null plan with a message that names them; ``branch_and_bound_frontier`` takes ``branching`` and
``verify_properties_babsr`` its documented arguments, both rejecting bad ones before a device is touched.  (A handle needs a GPU to exist:
the other refusals are in tests/test_gpu_frontier_babsr.py.)"""
import ctypes as C
import inspect

import pytest
from torch import nn

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_frontier_babsr_decide_workspace_bytes", "gnnb_frontier_babsr_decide", "gnnb_frontier_babsr_decide_jobs")
NEW_KERNELS = ("k_frontier_babsr_decide", "k_frontier_babsr_decide_jobs")
OLD_KERNELS = ("k_frontier_candidates", "k_frontier_fallback", "k_frontier_choose", "k_frontier_choose_copy", "k_frontier_fallback_jobs",
               "k_frontier_select_jobs", "k_frontier_rows_sel", "k_frontier_choose_jobs", "k_frontier_gather", "k_frontier_expand", "k_net_eval",
               "k_frontier_resolve", "k_frontier_decide", "k_frontier_store", "k_frontier_pick_jobs", "k_frontier_rows_jobs", "k_frontier_decide_jobs",
               "k_frontier_learn", "k_frontier_witness", "k_frontier_witness_jobs")
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def calls(lib, h, K, n_order=0, threshold=0.001, plan=True, n_entries=1):
    """The two entry points with handle ``h``; every pointer is null or an empty struct (nothing may be dereferenced).  K is the one-job
    form's batch and the jobs form's n."""
    plan_s = _lib.Plan(None, None, n_entries, K, 1, 8)
    pl = C.byref(plan_s) if plan else None
    return {"gnnb_frontier_babsr_decide": lambda: lib.gnnb_frontier_babsr_decide(h, K, None, None, None, threshold, 0, None, n_order, None, None, None, 0,
                                                                               None),
            "gnnb_frontier_babsr_decide_jobs": lambda: lib.gnnb_frontier_babsr_decide_jobs(h, pl, None, None, None, threshold, 0, None, n_order, None, None,
                                                                                         None, 0, None)}


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2                       # the additions are additive
    assert "GNNB_ABI_VERSION 2" in header.replace("  ", " ")


def test_every_new_kernel_has_one_profile_class_and_the_old_names_stay_single(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in NEW_KERNELS + OLD_KERNELS:
        assert classes.count(k) == 1, k
    assert len(set(classes)) == len(classes)


def test_no_option_was_added(lib):
    names = [lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())]
    assert sorted(names) == sorted(_lib.OPTIONS) and len(names) == 10


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in calls(lib, None, 2, n_order=3).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and b"null handle" in msg, (name, msg)


@pytest.mark.parametrize("K", [0, -3, 32768])
def test_a_row_count_outside_the_range_is_refused_with_a_message(lib, K):
    for name, call in calls(lib, None, K).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and f"= {K} ".encode() in msg and b"null handle" not in msg, (name, msg)
    for ok in (1, 32767):                                    # the edges of the range pass this check (and stop at the null handle)
        for name, call in calls(lib, None, ok).items():
            assert call() == -1 and b"null handle" in lib.gnnb_last_error(), (name, ok)


@pytest.mark.parametrize("n_order", [-1, 9])
def test_an_order_outside_the_range_is_refused_with_a_message(lib, n_order):
    for name, call in calls(lib, None, 2, n_order=n_order).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and f"n_order = {n_order} ".encode() in msg and b"null handle" not in msg, (name, msg)
    for ok in (0, 8):
        for name, call in calls(lib, None, 2, n_order=ok).items():
            assert call() == -1 and b"null handle" in lib.gnnb_last_error(), (name, ok)


def test_a_nan_threshold_is_refused_with_a_message(lib):
    for name, call in calls(lib, None, 2, threshold=NAN).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and b"decision_threshold = nan" in msg and b"null handle" not in msg, (name, msg)
    for ok in (float("inf"), -float("inf"), 0.0):            # any number is a threshold
        for name, call in calls(lib, None, 2, threshold=ok).items():
            assert call() == -1 and b"null handle" in lib.gnnb_last_error(), (name, ok)


def test_a_null_plan_or_a_plan_without_an_entry_is_refused(lib):
    assert calls(lib, None, 1, plan=False)["gnnb_frontier_babsr_decide_jobs"]() == -1
    assert b"gnnb_frontier_babsr_decide_jobs: null plan" in lib.gnnb_last_error()
    assert calls(lib, None, 2, n_entries=0)["gnnb_frontier_babsr_decide_jobs"]() == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_babsr_decide_jobs:" in msg and b"0 plan entries" in msg, msg


def test_workspace_sizer_returns_zero_for_a_null_handle(lib):
    assert lib.gnnb_frontier_babsr_decide_workspace_bytes(None, 4) == 0


# ---- the Python arguments ---------------------------------------------------------------------------------------------------------------
def test_branching_is_the_last_keyword_and_defaults_to_gnn():
    for f in (frontier.branch_and_bound_frontier, frontier.FrontierRun.__init__, frontier.JobsRun.__init__):
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "branching" and params["branching"].default == "gnn", f
    assert frontier._Round.branching == "gnn"


@pytest.mark.parametrize("kw", [{"branching": "sb"}, {"branching": None}, {"branching": "GNN"}, {"branching": 1}, {"branching": ["babsr"]},
                                {"branching": "babsr", "branching_threshold": 0.2}, {"branching": "babsr", "online_threshold": 5},
                                {"branching": "babsr", "branching_threshold": 0.2, "online_threshold": 5}])
def test_bad_branching_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError, match="branching"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], **kw)


@pytest.mark.parametrize("kw", [{}, {"branching": "gnn"}, {"branching": "babsr"}, {"branching": "babsr", "sparsest_layer": 1, "decision_threshold": 0.01},
                                {"branching": "gnn", "branching_threshold": 0.2}])
def test_good_branching_arguments_reach_the_device(kw):
    """The checks pass and the first thing touched is the choice's engine: NoDevice raises there, so nothing before it refused."""
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [nn.Linear(5, 1)], K=4, **kw)


def test_the_signature_of_verify_properties_babsr_is_the_documented_one():
    sig = inspect.signature(frontier.verify_properties_babsr)
    assert list(sig.parameters) == ["choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr", "eps", "max_rounds", "sparsest_layer",
                                    "decision_threshold", "log", "trace", "stats"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["K"], d["segments"], d["capacity"], d["n_iter"], d["lr"], d["eps"], d["max_rounds"]) == (16, None, None, 20, 0.1, 1e-4, 50)
    assert (d["sparsest_layer"], d["decision_threshold"], d["log"], d["trace"], d["stats"]) == (0, 0.001, print, None, None)
    # the two older jobs loops keep theirs
    assert list(inspect.signature(frontier.verify_properties).parameters) == ["choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr",
                                                                            "eps", "max_rounds", "log", "trace"]
    assert list(inspect.signature(frontier.verify_properties_threshold).parameters)[:4] == ["choice", "fixed_layers", "jobs", "branching_threshold"]


@pytest.mark.parametrize("kw", [{"K": 0}, {"K": -1}, {"K": 2.5}, {"K": True}, {"K": 4, "capacity": 8}, {"K": 1, "capacity": 2}, {"n_iter": -1},
                                {"max_rounds": -1}, {"eps": -1.0}, {"lr": 0.0}, {"segments": 0}, {"segments": 2.0}, {"segments": True},
                                {"K": 16, "segments": 1024}, {"K": 4, "segments": 4096}])
def test_bad_jobs_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.verify_properties_babsr(NoDevice(), [], [job(), job()], **kw)


def test_bad_jobs_are_rejected_before_a_device_is_touched():
    with pytest.raises(ValueError, match="no job"):
        frontier.verify_properties_babsr(NoDevice(), [], [])
    with pytest.raises(ValueError, match="one input shape"):
        frontier.verify_properties_babsr(NoDevice(), [], [job(), job((3, 4, 5))])
    with pytest.raises(ValueError, match="property layer"):
        frontier.verify_properties_babsr(NoDevice(), [], [job(), job(prop=nn.Linear(5, 2))])
    with pytest.raises(ValueError, match="pgd_steps"):       # a FrontierJobs' options are checked as for verify_properties
        frontier.verify_properties_babsr(NoDevice(), [], frontier.FrontierJobs([job()], pgd_steps=-1))


def test_good_jobs_arguments_reach_the_device():
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.verify_properties_babsr(NoDevice(), [], [job(), job()], K=4)
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.verify_properties_babsr(NoDevice(), [], frontier.FrontierJobs([job(), job()], witness=[], pgd_steps=2), K=4, sparsest_layer=1)
