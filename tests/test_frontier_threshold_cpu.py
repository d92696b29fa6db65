"""CPU: the BaBSR fall-back below a branching threshold inside the device frontier.  The entry points
gnnb_frontier_fallback / gnnb_frontier_choose are declared, bound and exported, their kernels have one profile class each, they refuse a
null handle and K < 1 with a message; ``branch_and_bound_frontier`` rejects bad threshold arguments before it touches a device and
``verify_properties`` does not take the option.  (A handle needs a GPU to exist: the other refusals are in
tests/test_gpu_frontier_threshold.py.)"""
import ctypes as C

import pytest

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_frontier_fallback_workspace_bytes", "gnnb_frontier_fallback", "gnnb_frontier_choose")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def calls(lib, h, K, m=0):
    """The two steps with handle ``h``; every pointer is null or an empty struct (nothing may be dereferenced)."""
    pool, fb, pa, pb = _lib.Pool(), _lib.Fallback(), _lib.Children(), _lib.Children()
    return {"gnnb_frontier_fallback": lambda: lib.gnnb_frontier_fallback(h, C.byref(pool), None, K, C.byref(fb), *([None] * 6), None, 0, None),
            "gnnb_frontier_choose": lambda: lib.gnnb_frontier_choose(h, C.byref(pool), K, m, *([None] * 5), C.byref(pa), C.byref(pb), *([None] * 4), None)}


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert "} gnnb_fallback;" in header and "} gnnb_children_rw;" in header
    assert lib.gnnb_abi_version() == 2                       # the additions are additive


def test_every_new_kernel_has_one_profile_class_and_the_old_names_stay_single(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in ("k_frontier_candidates", "k_frontier_fallback", "k_frontier_choose", "k_frontier_choose_copy",
              "k_frontier_gather", "k_frontier_expand", "k_net_eval", "k_frontier_resolve", "k_frontier_decide", "k_frontier_store",
              "k_frontier_pick_jobs", "k_frontier_rows_jobs", "k_frontier_decide_jobs"):
        assert classes.count(k) == 1, k
    assert len(set(classes)) == len(classes)


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in calls(lib, None, 2).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and b"null handle" in msg, (name, msg)


@pytest.mark.parametrize("K", [0, -3, 32768])
def test_a_batch_outside_the_range_is_refused_with_a_message(lib, K):
    for name, call in calls(lib, None, K).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and str(K).encode() in msg and b"null handle" not in msg, (name, msg)


def test_a_null_pool_is_refused(lib):
    assert lib.gnnb_frontier_fallback(None, None, None, 1, None, *([None] * 6), None, 0, None) == -1
    assert lib.gnnb_frontier_choose(None, None, 1, 0, *([None] * 5), None, None, *([None] * 4), None) == -1


def test_workspace_sizer_returns_zero_for_a_null_handle(lib):
    assert lib.gnnb_frontier_fallback_workspace_bytes(None, 4) == 0


@pytest.mark.parametrize("kw", [{"branching_threshold": 0}, {"branching_threshold": 0.0}, {"branching_threshold": -0.2}, {"branching_threshold": 1.5},
                                {"branching_threshold": float("nan")}, {"branching_threshold": "0.2"}, {"branching_threshold": True},
                                {"branching_threshold": 0.2, "kwbd_threshold": -1}, {"branching_threshold": 0.2, "kwbd_threshold": 2.5},
                                {"branching_threshold": 0.2, "kwbd_threshold": True}, {"branching_threshold": 0.2, "kwbd_threshold": None}])
def test_bad_threshold_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, **kw)


def test_the_edges_of_the_ranges_are_accepted_by_the_argument_check():
    for bt, kb in ((1, 0), (1.0, 10), (1e-300, 0), (0.2, 10 ** 6), (None, -5)):      # (None: the mode is off, kwbd_threshold is not read)
        frontier._check_threshold(bt, kb)


def test_verify_properties_does_not_take_the_option():
    with pytest.raises(TypeError):
        frontier.verify_properties(NoDevice(), [], [job()], branching_threshold=0.2)
