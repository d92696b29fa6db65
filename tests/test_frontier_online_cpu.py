"""CPU: learning online inside the device frontier.  The entry points gnnb_frontier_learn / gnnb_online_step_rows
are declared, bound and exported, their kernels have one profile class each, they refuse a null handle and a K or n outside their ranges
with a message that names them; ``branch_and_bound_frontier`` rejects bad online arguments before it touches a device and
``verify_properties`` / ``verify_properties_threshold`` do not take the option.  (A handle needs a GPU to exist: the other refusals are in
tests/test_gpu_frontier_online.py.)"""
import ctypes as C

import pytest

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_frontier_learn", "gnnb_online_step_rows")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def learn(lib, h, K, online_threshold=1):
    return lib.gnnb_frontier_learn(h, K, *([None] * 5), online_threshold, *([None] * 5), None)


def step_rows(lib, h, K, n):
    return lib.gnnb_online_step_rows(h, C.byref(_lib.Batch()), K, None, n, None, None, None, None, 0, None)


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2                       # the additions are additive
    assert "#define GNNB_ABI_VERSION 2" in header


def test_every_new_kernel_has_one_profile_class_and_no_name_is_doubled(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in ("k_frontier_learn", "k_trows_gather"):
        assert classes.count(k) == 1, k
    assert len(set(classes)) == len(classes) and "" not in classes


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in (("gnnb_frontier_learn", lambda: learn(lib, None, 2)), ("gnnb_online_step_rows", lambda: step_rows(lib, None, 2, 1))):
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and b"null handle" in msg, (name, msg)


@pytest.mark.parametrize("K", [0, -3, 32768])
def test_learn_refuses_a_batch_outside_the_range_with_a_message(lib, K):
    assert learn(lib, None, K) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_learn" in msg and str(K).encode() in msg and b"null handle" not in msg, msg


@pytest.mark.parametrize("K,n", [(4, 0), (4, -1), (4, 5), (0, 1), (-2, 1)])
def test_step_rows_refuses_n_outside_the_batch_with_a_message(lib, K, n):
    assert step_rows(lib, None, K, n) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_online_step_rows" in msg and f"n = {n}".encode() in msg and f"K = {K}".encode() in msg and b"null handle" not in msg, msg


ON = {"branching_threshold": 0.5}


@pytest.mark.parametrize("kw", [{"online_threshold": 0, **ON}, {"online_threshold": -1, **ON}, {"online_threshold": 2.0, **ON}, {"online_threshold": True, **ON},
                                {"online_threshold": "5", **ON},                      # not None, not an integer >= 1
                                {"online_threshold": 5},                              # without a branching_threshold
                                {"online_threshold": 5, **ON, "kwbd_threshold": 3}, {"online_threshold": 5, **ON, "kwbd_threshold": 2 ** 31 - 1},
                                {"online_threshold": 5, **ON, "kwbd_threshold": 0}])  # a kwbd_threshold other than the default
def test_bad_online_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, **kw)
    with pytest.raises(ValueError):
        frontier.FrontierRun(NoDevice(), NoDevice(), [], K=4, **kw)


@pytest.mark.parametrize("online_threshold", [1, 5, 2 ** 30])
def test_a_choice_that_is_no_online_graphchoice_is_a_type_error(online_threshold):
    """Valid numbers, but the choice owns no lr / wd: refused before anything of it is touched (NoDevice raises on any attribute)."""
    with pytest.raises(TypeError, match="graph_score_online"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, online_threshold=online_threshold, **ON)
    with pytest.raises(TypeError, match="graph_score_online"):
        frontier.branch_and_bound_frontier(NoDevice(), object(), [], K=4, online_threshold=online_threshold, **ON, kwbd_threshold=10)


def test_off_is_accepted_by_the_argument_check_whatever_the_other_arguments():
    frontier._check_online(None, None, 3, NoDevice())
    frontier._check_online(None, 0.5, 0, NoDevice())


def test_verify_properties_do_not_take_the_option():
    with pytest.raises(TypeError):
        frontier.verify_properties(NoDevice(), [], [job()], online_threshold=5)
    with pytest.raises(TypeError):
        frontier.verify_properties_threshold(NoDevice(), [], [job()], 0.5, online_threshold=5)
