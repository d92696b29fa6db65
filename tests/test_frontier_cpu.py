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


def test_start_record_is_what_a_new_pool_holds():
    """Three +inf (global_ub, closed_lb, lowest open bound), then zeros: the first FRONTIER_STATE_DOUBLES values ``DomainPool`` starts from."""
    inf = float("inf")
    assert _lib.FRONTIER_STATE_DOUBLES == 9
    assert frontier._start_record() == [inf, inf, inf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def _inline_round(st, K, capacity, eps, decision_bound, rounds, max_rounds):
    """The rule ``branch_and_bound_frontier`` had inline before it shared ``_stop_reason`` and ``plan_round`` with ``verify_properties``."""
    global_lb, global_ub = min(st[_lib.FS_LOWEST_OPEN], st[_lib.FS_CLOSED_LB], st[_lib.FS_GLOBAL_UB]), st[_lib.FS_GLOBAL_UB]
    n_open, in_use = int(st[_lib.FS_N_OPEN]), int(st[_lib.FS_IN_USE])
    if n_open == 0:
        return "exhausted", 0, False
    if not global_ub - global_lb > eps:
        return "gap", 0, False
    if decision_bound is not None and (global_lb >= decision_bound or global_ub < decision_bound):
        return "decision", 0, False
    if rounds >= max_rounds:
        return "max_rounds", 0, False
    if n_open + min(K, n_open) > capacity:
        return "capacity", 0, False
    k = min(K, n_open)
    return None, k, in_use + k > capacity


def _record(n_open, in_use, gub=1.0, closed=float("inf"), low=-1.0):
    return [gub, closed, low, float(n_open), float(in_use), 0.0, 0.0, 0.0, 0.0]


# (record, K, capacity, eps, decision_bound, rounds, max_rounds) -> (reason, k, compact), written out by hand.  global_lb = min(low, closed,
# gub) = -1 and global_ub = 1 unless the record says otherwise.
ROUND_CASES = [
    # a plain round: fewer open domains than K, and more
    ((_record(3, 5), 4, 20, 1e-4, None, 0, 5), (None, 3, False)),
    ((_record(9, 9), 4, 20, 1e-4, None, 0, 5), (None, 4, False)),
    # each stop reason alone
    ((_record(0, 5), 4, 20, 1e-4, None, 0, 5), ("exhausted", 0, False)),
    ((_record(3, 5, gub=1.0, low=1.0 - 5e-5), 4, 20, 1e-4, None, 0, 5), ("gap", 0, False)),
    ((_record(3, 5, gub=1.0, low=0.5), 4, 20, 0.5, None, 0, 5), ("gap", 0, False)),                   # (a gap equal to eps stops)
    ((_record(3, 5, gub=1.0, low=0.25), 4, 20, 0.5, None, 0, 5), (None, 3, False)),
    ((_record(3, 5), 4, 20, 1e-4, 2.0, 0, 5), ("decision", 0, False)),                                 # global_ub below the bound
    ((_record(3, 5), 4, 20, 1e-4, -2.0, 0, 5), ("decision", 0, False)),                                # global_lb above it
    ((_record(3, 5), 4, 20, 1e-4, None, 5, 5), ("max_rounds", 0, False)),
    ((_record(18, 18), 4, 20, 1e-4, None, 0, 5), ("capacity", 0, False)),
    # in pairs: exhausted > gap > decision > max_rounds > capacity
    ((_record(0, 5, gub=1.0, low=1.0), 4, 20, 1e-4, None, 0, 5), ("exhausted", 0, False)),
    ((_record(0, 5), 4, 20, 1e-4, 2.0, 0, 5), ("exhausted", 0, False)),
    ((_record(0, 5), 4, 20, 1e-4, None, 5, 5), ("exhausted", 0, False)),
    ((_record(3, 5, gub=1.0, low=1.0), 4, 20, 1e-4, 2.0, 0, 5), ("gap", 0, False)),
    ((_record(3, 5, gub=1.0, low=1.0), 4, 20, 1e-4, None, 5, 5), ("gap", 0, False)),
    ((_record(18, 18, gub=1.0, low=1.0), 4, 20, 1e-4, None, 0, 5), ("gap", 0, False)),
    ((_record(3, 5), 4, 20, 1e-4, 2.0, 5, 5), ("decision", 0, False)),
    ((_record(18, 18), 4, 20, 1e-4, 2.0, 0, 5), ("decision", 0, False)),
    ((_record(18, 18), 4, 20, 1e-4, None, 5, 5), ("max_rounds", 0, False)),
    # the bound closed_lb or global_ub gives, not the lowest open one
    ((_record(3, 5, gub=1.0, closed=-3.0, low=-1.0), 4, 20, 1e-4, -2.0, 0, 5), (None, 3, False)),
    ((_record(3, 5, gub=1.0, closed=0.5, low=2.0), 4, 20, 1e-4, 0.5, 0, 5), ("decision", 0, False)),
    # n_open + min(K, n_open) equal to the capacity, and one above it
    ((_record(16, 16), 4, 20, 1e-4, None, 0, 5), (None, 4, False)),
    ((_record(17, 17), 4, 20, 1e-4, None, 0, 5), ("capacity", 0, False)),
    ((_record(2, 2), 4, 4, 1e-4, None, 0, 5), (None, 2, False)),                                       # (min(K, n_open) = n_open)
    ((_record(3, 3), 4, 5, 1e-4, None, 0, 5), ("capacity", 0, False)),
    # in_use + k equal to the capacity, and one above it: the compaction flag
    ((_record(3, 17), 4, 20, 1e-4, None, 0, 5), (None, 3, False)),
    ((_record(3, 18), 4, 20, 1e-4, None, 0, 5), (None, 3, True)),
    ((_record(9, 16), 4, 20, 1e-4, None, 0, 5), (None, 4, False)),
    ((_record(9, 17), 4, 20, 1e-4, None, 0, 5), (None, 4, True)),
    # no decision bound, and one equal to global_lb (>= stops)
    ((_record(3, 5), 4, 20, 1e-4, None, 0, 5), (None, 3, False)),
    ((_record(3, 5), 4, 20, 1e-4, -1.0, 0, 5), ("decision", 0, False)),
    ((_record(3, 5), 4, 20, 1e-4, 1.0, 0, 5), (None, 3, False)),                                       # (global_ub equal to it does not)
    ((_record(3, 5), 4, 20, 1e-4, 0.0, 0, 5), (None, 3, False)),
    # max_rounds = 0 stops before the first round
    ((_record(1, 1), 4, 20, 1e-4, None, 0, 0), ("max_rounds", 0, False)),
]


@pytest.mark.parametrize("args,expected", ROUND_CASES)
def test_the_one_job_loop_decides_its_round_by_the_rule_it_had_inline(args, expected):
    assert _inline_round(*args) == expected                   # the table itself, against the restated rule
    assert frontier._one_job_round(*args) == expected


def _traced(m_e, sel_rows):
    """A hand-made run of 5 parent rows after a threshold round, as ``_threshold_trace`` reads it: row i decides [0, i] (GNN), [1, 10 + i]
    (KW) and [2, 20 + i] (final); improvements i / 8 (GNN) and i / 4 (KW); pair A's child c bound -c, pair B's child c bound -c / 2."""
    import types
    import torch
    i5, i10 = torch.arange(5), torch.arange(10)
    dec = lambda layer, first: torch.stack([torch.full((5,), layer), first + i5], dim=1).to(torch.int32)      # noqa: E731
    return types.SimpleNamespace(
        P=types.SimpleNamespace(dec=dec(0, 0)), kw_dec=dec(1, 10), dec=dec(2, 20), gnn_imp=i5.double() / 8, kw_imp=i5.double() / 4,
        used_kw=torch.tensor([1, 0, 1, 0, 1], dtype=torch.int32), sel_rows=torch.tensor(sel_rows + [77] * (5 - len(sel_rows)), dtype=torch.int32),
        pair_a=(-i10.double(), (i10 % 3 == 0).to(torch.int32)), ChB=types.SimpleNamespace(bound=-i10.double() / 2, infeasible=(i10 % 4 == 1).to(torch.int32)),
        m_e=m_e, M=m_e[-1])


THRESHOLD_TRACE_CASES = {
    "one job, nobody selected": ((_traced([0], []), 2), {
        "gnn_decisions": [[0, 0], [0, 1]], "gnn_improvement": [0.0, 0.125], "kw_decisions": [[1, 10], [1, 11]], "kw_improvement": [-1.0, -1.0], "selected": [],
        "used_kw": [0, 0], "decisions": [[0, 0], [0, 1]], "gnn_child_bounds": [-0.0, -1.0, -2.0, -3.0], "gnn_child_infeasible": [1, 0, 0, 1],
        "kw_child_bounds": [], "kw_child_infeasible": []}),
    "one job, rows 0 and 2 selected": ((_traced([2], [0, 2]), 3), {
        "gnn_decisions": [[0, 0], [0, 1], [0, 2]], "gnn_improvement": [0.0, 0.125, 0.25], "kw_decisions": [[1, 10], [1, 11], [1, 12]],
        "kw_improvement": [0.0, 0.25, 0.5], "selected": [0, 2], "used_kw": [1, 0, 1], "decisions": [[2, 20], [2, 21], [2, 22]],
        "gnn_child_bounds": [-0.0, -1.0, -2.0, -3.0, -4.0, -5.0], "gnn_child_infeasible": [1, 0, 0, 1, 0, 0],
        "kw_child_bounds": [-0.0, -0.5, -1.0, -1.5], "kw_child_infeasible": [0, 1, 0, 0]}),
    # entries (rows [0, 2), m = 1) and (rows [2, 5), m = 2): entry 1's selected rows 2 and 4 count from row 2, its pair B is children 2..5
    "entry 1 of a two-entry plan": ((_traced([1, 2, 3], [1, 2, 4]), 3, 1, 2), {
        "gnn_decisions": [[0, 2], [0, 3], [0, 4]], "gnn_improvement": [0.25, 0.375, 0.5], "kw_decisions": [[1, 12], [1, 13], [1, 14]],
        "kw_improvement": [0.5, 0.75, 1.0], "selected": [0, 2], "used_kw": [1, 0, 1], "decisions": [[2, 22], [2, 23], [2, 24]],
        "gnn_child_bounds": [-4.0, -5.0, -6.0, -7.0, -8.0, -9.0], "gnn_child_infeasible": [0, 0, 1, 0, 0, 1],
        "kw_child_bounds": [-1.0, -1.5, -2.0, -2.5], "kw_child_infeasible": [0, 0, 0, 1]}),
}


@pytest.mark.parametrize("case", list(THRESHOLD_TRACE_CASES))
def test_the_threshold_trace_of_a_plan_entry_is_the_dict_written_out_by_hand(case):
    """``_threshold_trace`` serves the one-job round (entry 0, row 0) and every entry of a many-job round: the keys and values of both
    public docstrings, with "selected" counted from the entry's first row and pair B's range from the sum of the m before the entry."""
    args, expected = THRESHOLD_TRACE_CASES[case]
    assert frontier._threshold_trace(*args) == expected
