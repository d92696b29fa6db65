"""CPU: the BaBSR fall-back for every job of a multi-property frontier.  The entry points
gnnb_frontier_fallback_jobs / gnnb_frontier_choose_jobs are declared, bound and exported, their kernels have one profile class each, they
refuse a null handle, a null plan or pool, n outside 1..32767 and an M outside its range with a message that names them, and the
workspace sizer returns 0 for a null handle; ``verify_properties_threshold`` rejects bad threshold and jobs arguments before it touches
a device.  (A handle needs a GPU to exist: the other refusals are in tests/test_gpu_frontier_jobs_threshold.py.)"""
import ctypes as C
import inspect

import pytest
from torch import nn

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_frontier_fallback_jobs_workspace_bytes", "gnnb_frontier_fallback_jobs", "gnnb_frontier_choose_jobs")
NEW_KERNELS = ("k_frontier_fallback_jobs", "k_frontier_select_jobs", "k_frontier_rows_sel", "k_frontier_choose_jobs")
OLD_KERNELS = ("k_frontier_candidates", "k_frontier_fallback", "k_frontier_choose", "k_frontier_choose_copy", "k_frontier_gather", "k_frontier_expand",
               "k_net_eval", "k_frontier_resolve", "k_frontier_decide", "k_frontier_store", "k_frontier_pick_jobs", "k_frontier_rows_jobs",
               "k_frontier_decide_jobs")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def calls(lib, h, n_entries, n, M=0, plan=True, pool=True):
    """The two steps with handle ``h``; every pointer is null or an empty struct (nothing may be dereferenced)."""
    pool_s, fb, pa, pb, plan_s = _lib.Pool(), _lib.Fallback(), _lib.Children(), _lib.Children(), _lib.Plan(None, None, n_entries, n, 1, 8)
    pl, po = C.byref(plan_s) if plan else None, C.byref(pool_s) if pool else None
    return {"gnnb_frontier_fallback_jobs": lambda: lib.gnnb_frontier_fallback_jobs(h, po, pl, None, C.byref(fb), *([None] * 14), None, 0, None),
            "gnnb_frontier_choose_jobs": lambda: lib.gnnb_frontier_choose_jobs(h, po, pl, M, *([None] * 6), C.byref(pa), C.byref(pb), *([None] * 4),
                                                                             None)}


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
    assert sorted(lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())) == sorted(_lib.OPTIONS)


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in calls(lib, None, 1, 2).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and b"null handle" in msg, (name, msg)


@pytest.mark.parametrize("n_entries,n", [(1, 0), (1, -3), (0, 2), (1, 32768)])
def test_no_entry_or_a_row_count_outside_the_range_is_refused_with_a_message(lib, n_entries, n):
    for name, call in calls(lib, None, n_entries, n).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and f"n = {n} ".encode() in msg and b"null handle" not in msg, (name, msg)


@pytest.mark.parametrize("M", [-1, 5, 40000])
def test_a_count_of_selected_parents_outside_the_range_is_refused_with_a_message(lib, M):
    """M must lie in 0..n (n = 4 here); like a batch outside its range, this is refused before the handle is looked at."""
    call = calls(lib, None, 1, 4, M=M)["gnnb_frontier_choose_jobs"]
    assert call() == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_choose_jobs" in msg and f"M = {M} ".encode() in msg and b"null handle" not in msg, msg
    for ok in (0, 4):                                        # the edges of the range pass this check (and stop at the null handle)
        assert calls(lib, None, 1, 4, M=ok)["gnnb_frontier_choose_jobs"]() == -1
        assert b"null handle" in lib.gnnb_last_error()


def test_a_null_plan_or_pool_is_refused(lib):
    for name, call in calls(lib, None, 1, 1, plan=False).items():
        assert call() == -1, name
        assert (name + ": null plan").encode() in lib.gnnb_last_error(), name
    for name, call in calls(lib, None, 1, 1, pool=False).items():
        assert call() == -1, name
        assert name.encode() in lib.gnnb_last_error(), name


def test_workspace_sizer_returns_zero_for_a_null_handle(lib):
    assert lib.gnnb_frontier_fallback_jobs_workspace_bytes(None, 4) == 0


# ---- verify_properties_threshold's arguments ------------------------------------------------------------------------------------------
def test_the_signature_is_the_documented_one():
    sig = inspect.signature(frontier.verify_properties_threshold)
    assert list(sig.parameters) == ["choice", "fixed_layers", "jobs", "branching_threshold", "K", "segments", "capacity", "n_iter", "lr", "eps", "max_rounds",
                                    "kwbd_threshold", "sparsest_layer", "decision_threshold", "log", "trace", "stats"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["K"], d["segments"], d["capacity"], d["n_iter"], d["lr"], d["eps"], d["max_rounds"]) == (16, None, None, 20, 0.1, 1e-4, 50)
    assert (d["kwbd_threshold"], d["sparsest_layer"], d["decision_threshold"], d["trace"], d["stats"]) == (10, 0, 0.001, None, None)
    assert d["branching_threshold"] is inspect.Parameter.empty
    # verify_properties keeps its signature
    assert list(inspect.signature(frontier.verify_properties).parameters) == ["choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr",
                                                                            "eps", "max_rounds", "log", "trace"]


@pytest.mark.parametrize("kw", [{"branching_threshold": 0}, {"branching_threshold": 0.0}, {"branching_threshold": -0.2}, {"branching_threshold": 1.5},
                                {"branching_threshold": float("nan")}, {"branching_threshold": "0.2"}, {"branching_threshold": True},
                                {"branching_threshold": None},
                                {"branching_threshold": 0.2, "kwbd_threshold": -1}, {"branching_threshold": 0.2, "kwbd_threshold": 2.5},
                                {"branching_threshold": 0.2, "kwbd_threshold": True}, {"branching_threshold": 0.2, "kwbd_threshold": None}])
def test_bad_threshold_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.verify_properties_threshold(NoDevice(), [], [job(), job()], **kw)


@pytest.mark.parametrize("kw", [{"K": 0}, {"K": -1}, {"K": 2.5}, {"K": True}, {"K": 4, "capacity": 8}, {"K": 1, "capacity": 2}, {"n_iter": -1},
                                {"max_rounds": -1}, {"eps": -1.0}, {"lr": 0.0}, {"segments": 0}, {"segments": 2.0}, {"segments": True},
                                {"K": 16, "segments": 1024}, {"K": 4, "segments": 4096}])
def test_bad_jobs_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.verify_properties_threshold(NoDevice(), [], [job(), job()], 0.2, **kw)


def test_bad_jobs_are_rejected_before_a_device_is_touched():
    with pytest.raises(ValueError, match="no job"):
        frontier.verify_properties_threshold(NoDevice(), [], [], 0.2)
    with pytest.raises(ValueError, match="one input shape"):
        frontier.verify_properties_threshold(NoDevice(), [], [job(), job((3, 4, 5))], 0.2)
    with pytest.raises(ValueError, match="property layer"):
        frontier.verify_properties_threshold(NoDevice(), [], [job(), job(prop=nn.Linear(5, 2))], 0.2)
    with pytest.raises(TypeError):                           # the threshold is not optional
        frontier.verify_properties_threshold(NoDevice(), [], [job()])


def test_good_arguments_reach_the_device():
    """The checks pass and the first thing touched is the choice's engine: NoDevice raises there, so nothing before it refused."""
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.verify_properties_threshold(NoDevice(), [], [job(), job()], 0.2, K=4)
