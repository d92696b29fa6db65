"""CPU: strong branching inside the device-resident frontier.  The entry points gnnb_strong_list / gnnb_strong_pick
and the list's workspace sizer are declared, bound and exported, their kernels have one profile class each and every older class stays
single, no option was added; they refuse a null handle, K outside 1..32767, a negative top_m and a top_m without scores with a message that
names them; ``branch_and_bound_frontier`` takes ``strong_candidates``, ``strong_chunk`` and ``strong_audit`` in front of ``branching`` and
rejects bad ones before a device is touched.  (A handle needs a GPU to exist: the other refusals are in tests/test_gpu_frontier_strong.py.)"""
import inspect

import pytest
from torch import nn

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_babsr_cpu import NEW_KERNELS as BABSR_KERNELS, OLD_KERNELS
from tests.test_frontier_cpu import NoDevice

NEW = ("gnnb_strong_list_workspace_bytes", "gnnb_strong_list", "gnnb_strong_pick")
NEW_KERNELS = ("k_strong_count", "k_strong_compact", "k_strong_pick")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def calls(lib, h, K, top_m=0):
    """The two entry points with handle ``h``; every pointer is null (nothing may be dereferenced)."""
    return {"gnnb_strong_list": lambda: lib.gnnb_strong_list(h, None, None, K, None, None, top_m, None, None, None, None, None, 0, None),
            "gnnb_strong_pick": lambda: lib.gnnb_strong_pick(h, None, None, K, None, None, None, None, None, None, None, None, None, None)}


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert "gnnb_k_strong.h" in _lib.SOURCES
    assert lib.gnnb_abi_version() == 2                       # the additions are additive
    assert "GNNB_ABI_VERSION 2" in header.replace("  ", " ")


def test_every_new_kernel_has_one_profile_class_and_the_old_names_stay_single(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in NEW_KERNELS + BABSR_KERNELS + OLD_KERNELS:
        assert classes.count(k) == 1, k
    assert len(set(classes)) == len(classes)
    assert tuple(classes[-3:]) == NEW_KERNELS                # appended: no older class changed its number


def test_no_option_was_added(lib):
    names = [lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())]
    assert sorted(names) == sorted(_lib.OPTIONS) and len(names) == 10


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in calls(lib, None, 2).items():
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


def test_a_negative_top_m_and_a_top_m_without_scores_are_refused_with_a_message(lib):
    assert calls(lib, None, 2, top_m=-1)["gnnb_strong_list"]() == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_list:" in msg and b"top_m = -1 " in msg and b"null handle" not in msg, msg
    assert calls(lib, None, 2, top_m=4)["gnnb_strong_list"]() == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_list:" in msg and b"top_m = 4 " in msg and b"scores" in msg and b"null handle" not in msg, msg
    assert calls(lib, None, 2, top_m=0)["gnnb_strong_list"]() == -1 and b"null handle" in lib.gnnb_last_error()      # 0 needs no scores


def test_workspace_sizer_returns_zero_for_a_null_handle(lib):
    assert lib.gnnb_strong_list_workspace_bytes(None, 4) == 0


# ---- the Python arguments ---------------------------------------------------------------------------------------------------------------
def test_the_new_keywords_stand_in_front_of_branching_which_stays_last():
    for f in (frontier.branch_and_bound_frontier, frontier.FrontierRun.__init__):
        params = inspect.signature(f).parameters
        assert list(params)[-4:] == ["strong_candidates", "strong_chunk", "strong_audit", "branching"], f
        assert (params["strong_candidates"].default, params["strong_chunk"].default, params["strong_audit"].default) == (None, 256, None)
        assert frontier.STRONG_CHUNK_DEFAULT == 256          # (the best of the chunks measured)
        assert params["branching"].default == "gnn"
    jobs = inspect.signature(frontier.JobsRun.__init__).parameters
    assert list(jobs)[-1] == "branching" and not any(p.startswith("strong") for p in jobs)
    assert "strong" in frontier.BRANCHINGS and frontier._Round.strong_on is False


BAD = [({"branching": "strong", "strong_candidates": 0}, "strong_candidates"), ({"branching": "strong", "strong_candidates": -2}, "strong_candidates"),
       ({"branching": "strong", "strong_candidates": True}, "strong_candidates"), ({"branching": "strong", "strong_candidates": 2.0}, "strong_candidates"),
       ({"branching": "strong", "strong_candidates": "8"}, "strong_candidates"),
       ({"branching": "strong", "strong_chunk": 0}, "strong_chunk"), ({"branching": "strong", "strong_chunk": None}, "strong_chunk"),
       ({"branching": "strong", "strong_chunk": True}, "strong_chunk"), ({"branching": "strong", "strong_chunk": 64.0}, "strong_chunk"),
       ({"branching": "strong", "strong_audit": ()}, "strong_audit"), ({"strong_audit": {}}, "strong_audit"), ({"strong_audit": True}, "strong_audit"),
       ({"branching": "strong", "branching_threshold": 0.2}, "branching"), ({"branching": "strong", "online_threshold": 5}, "branching"),
       ({"branching": "strong", "branching_threshold": 0.2, "online_threshold": 5}, "branching"),
       ({"strong_candidates": 8}, "strong_candidates"), ({"branching": "babsr", "strong_candidates": 8}, "strong_candidates"),
       ({"strong_chunk": 64}, "strong_chunk"), ({"branching": "babsr", "strong_chunk": 64}, "strong_chunk"),
       ({"strong_audit": [], "branching_threshold": 0.2}, "strong_audit"), ({"strong_audit": [], "branching_threshold": 0.2, "online_threshold": 3}, "strong_audit")]


@pytest.mark.parametrize("kw,name", BAD)
def test_bad_strong_arguments_are_rejected_before_a_device_is_touched(kw, name):
    with pytest.raises(ValueError, match=name):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], **kw)


@pytest.mark.parametrize("kw", [{"branching": "strong"}, {"branching": "strong", "strong_candidates": 1}, {"branching": "strong", "strong_candidates": 16},
                                {"branching": "strong", "strong_chunk": 1}, {"branching": "strong", "strong_candidates": 8, "strong_chunk": 256},
                                {"branching": "strong", "strong_audit": []}, {"strong_audit": []}, {"branching": "babsr", "strong_audit": []},
                                {"strong_audit": [], "strong_candidates": 4, "strong_chunk": 7}, {"strong_candidates": None, "strong_chunk": 256}])
def test_good_strong_arguments_reach_the_device(kw):
    """The checks pass and the first thing touched is the choice's engine: NoDevice raises there, so nothing before it refused."""
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [nn.Linear(5, 1)], K=4, **kw)
