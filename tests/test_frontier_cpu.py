"""CPU: the device-resident BaB frontier's entry points (include/gnnb.h gnnb_frontier_gather / _expand / _commit, gnnb_net_eval) are
declared, bound and exported; they refuse a null handle and K < 1 before anything else, with a message; their workspace sizers return 0
for a null handle; and branch_and_bound_frontier rejects bad arguments before it touches a device.  (A handle needs a GPU to exist, so
the unbound-handle refusals are in tests/test_gpu_frontier.py.)"""
import ctypes as C

import pytest

from gnn_branching_amd import _lib, frontier

NEW = ("gnnb_frontier_gather", "gnnb_frontier_expand", "gnnb_net_eval_workspace_bytes", "gnnb_net_eval", "gnnb_frontier_commit_workspace_bytes",
       "gnnb_frontier_commit")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def calls(lib, h, K):
    """The four steps with handle ``h`` and batch size ``K``; every pointer is null or an empty struct (nothing may be dereferenced)."""
    pool, ch = _lib.Pool(), _lib.Children()
    return {"gnnb_frontier_gather": lambda: lib.gnnb_frontier_gather(h, C.byref(pool), None, K, None, None, None, None, None, None, None, None, None,
                                                                    None, None),
            "gnnb_frontier_expand": lambda: lib.gnnb_frontier_expand(h, C.byref(pool), None, None, K, None, None, None, None, None, None, None, None),
            "gnnb_net_eval": lambda: lib.gnnb_net_eval(h, None, None, None, K, None, None, 0, None),
            "gnnb_frontier_commit": lambda: lib.gnnb_frontier_commit(h, C.byref(pool), None, K, C.byref(ch), 1e-4, float("nan"), None, None, 0, None)}


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert "gnnb_k_frontier.h" in _lib.SOURCES
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in ("k_frontier_gather", "k_frontier_expand", "k_net_eval", "k_frontier_resolve", "k_frontier_decide", "k_frontier_store"):
        assert classes.count(k) == 1, k
    assert lib.gnnb_abi_version() == 2                       # the additions are additive
    assert f"#define GNNB_FRONTIER_STATE_DOUBLES {_lib.FRONTIER_STATE_DOUBLES}" in header


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in calls(lib, None, 2).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and b"null handle" in msg, (name, msg)


@pytest.mark.parametrize("K", [0, -3])
def test_a_batch_below_one_is_refused_with_a_message(lib, K):
    for name, call in calls(lib, None, K).items():
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() in msg and str(K).encode() in msg and b"null handle" not in msg, (name, msg)


def test_a_null_pool_is_refused(lib):
    assert lib.gnnb_frontier_gather(None, None, None, 1, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.gnnb_frontier_commit(None, None, None, 1, None, 1e-4, 0.0, None, None, 0, None) == -1


def test_workspace_sizers_return_zero_for_a_null_handle(lib):
    assert lib.gnnb_net_eval_workspace_bytes(None, 4) == 0
    assert lib.gnnb_frontier_commit_workspace_bytes(None, 4) == 0


class NoDevice:
    """Stands in for the GraphChoice: any attribute access means the loop went for a device."""

    def __getattr__(self, name):
        raise AssertionError(f"touched the scorer ({name}) before checking the arguments")


@pytest.mark.parametrize("kw", [{"K": 0}, {"K": -1}, {"K": 2.5}, {"K": True}, {"K": 4, "capacity": 8}, {"K": 1, "capacity": 2}, {"n_iter": -1},
                                {"max_rounds": -1}, {"eps": -1.0}, {"lr": 0.0}])
def test_bad_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], **kw)


def test_unknown_arguments_are_rejected():
    with pytest.raises(TypeError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, child_lp="dual_device")


def test_smallest_capacity_is_accepted_by_the_argument_check():
    assert frontier._check_args(4, 20, 0.1, 1e-4, 3, 9) == 9
    assert frontier._check_args(4, 20, 0.1, 1e-4, 3, None) >= 9


def test_bytes_per_open_domain():
    """DESIGN.md section 7.3's figure for cifar_base_kw: R = 3172 ReLU nodes, graph layers 3072 / 2048 / 1024 / 100 / 1."""
    assert frontier.DomainPool.bytes_per_domain([3072, 2048, 1024, 100, 1], 3172) == 3172 * 17 + 16 * 3173 + 12
