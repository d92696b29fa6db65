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


# ---- the report of a round, per plan entry -------------------------------------------------------------------------------------------------
def _launched(branching="strong", audit=None, imitate=None, last_imitation=0, witness=False):
    """A hand-made run of 5 parent rows (10 children) and 7 candidates after ``launch_round``, as the report reads it.  Row i: slot 10 + i,
    decision [0, i], table decision [1, i], parent bound -2 (row 3: 0.5); child c: bound -c / 4, upper value c / 2, live, infeasible
    only for c = 3.  Candidate q: improvement q / 8; rows 0..4 hold 2, 0, 3, 1, 1 of them (cand0 below), graph layers of 10 and 6 ReLUs.
    The step's loss i / 2, regret i / 4 and report [i, i + 1, i + 2, i + 3]; the incumbents' values 7, 8, 9 for segments 0, 1, 2."""
    import types
    import torch
    i5, i10, ns = torch.arange(5), torch.arange(10), types.SimpleNamespace
    dec = lambda layer: torch.stack([torch.full((5,), layer), i5], dim=1).to(torch.int32)      # noqa: E731
    parent = torch.tensor([-2.0, -2.0, -2.0, 0.5, -2.0], dtype=torch.float64)
    return ns(branching=branching, threshold=None, strong_audit=audit, imitate=imitate, last_imitation=last_imitation, witness_on=witness,
              eng=ns(sizes=[4, 10, 6, 1]), slots=(10 + i5).to(torch.int32), P=ns(bound=parent, dec=dec(0)), parent_bound=parent, s_dec=dec(1),
              Ch=ns(bound=-i10.double() / 4, ubv=i10.double() / 2, live=torch.ones(10, dtype=torch.int32), infeasible=(i10 == 3).to(torch.int32)),
              cand0=torch.tensor([0, 2, 2, 5, 6, 7], dtype=torch.int32), cand_entry=[0, 7], s_best=torch.tensor([0.125, -1.0, 0.5, 0.625, 0.75]).double(),
              cand_dec=torch.tensor([[0, 1], [1, 2], [0, 3], [0, 4], [1, 0], [1, 5], [0, 9]], dtype=torch.int32), s_imp=torch.arange(7).double() / 8,
              im_loss=i5.float() / 2, im_regret=i5.double() / 4, im_report=torch.stack([i5 + d for d in range(4)], dim=1).to(torch.int32),
              best_value=torch.tensor([7.0, 8.0, 9.0], dtype=torch.float64))


ONE_JOB = [(0, 0, 5)]
TWO_JOBS = [(0, 0, 2), (2, 2, 3)]                             # (segment, row0, k): the second entry starts at row 2, child 4, candidate 2
TAGS = [{"job": 5, "segment": 0, "round": 3}, {"job": 6, "segment": 2, "round": 0}]
RECORDS = [_record(3, 5), None, _record(4, 6, gub=3.0, closed=-4.0)]      # per segment: bounds (-1, 1) and (-4, 3)
ROWS = {"slots": [10, 11, 12, 13, 14], "parent_bounds": [-2.0, -2.0, -2.0, 0.5, -2.0], "decisions": [[0, 0], [0, 1], [0, 2], [0, 3], [0, 4]],
        "child_bounds": [0.0, -0.25, -0.5, -0.75, -1.0, -1.25, -1.5, -1.75, -2.0, -2.25], "child_ub": [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5],
        "live": [1] * 10, "infeasible": [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]}
CANDIDATES = {"strong_candidates": [[1, 12], [], [3, 4, 10], [15], [9]], "strong_improvement": [[0.0, 0.125], [], [0.25, 0.375, 0.5], [0.625], [0.75]]}
ENTRY_0 = {"slots": [10, 11], "parent_bounds": [-2.0, -2.0], "decisions": [[0, 0], [0, 1]], "child_bounds": [0.0, -0.25, -0.5, -0.75],
           "child_ub": [0.0, 0.5, 1.0, 1.5], "live": [1, 1, 1, 1], "infeasible": [0, 0, 0, 1], "strong_candidates": [[1, 12], []],
           "strong_improvement": [[0.0, 0.125], []]}
ENTRY_1 = {"slots": [12, 13, 14], "parent_bounds": [-2.0, 0.5, -2.0], "decisions": [[0, 2], [0, 3], [0, 4]],
           "child_bounds": [-1.0, -1.25, -1.5, -1.75, -2.0, -2.25], "child_ub": [2.0, 2.5, 3.0, 3.5, 4.0, 4.5], "live": [1] * 6, "infeasible": [0] * 6,
           "strong_candidates": [[3, 4, 10], [15], [9]], "strong_improvement": [[0.25, 0.375, 0.5], [0.625], [0.75]]}
# improvement of the committed pair: (min(lb0, 0) + min(lb1, 0) + 4) / 4 on the parent bound -2, an infeasible child counting 0; 1 for row 3
OWN = [(0 - 0.25 + 4) / 4, (-0.5 + 0 + 4) / 4, (-1 - 1.25 + 4) / 4, 1.0, (-2 - 2.25 + 4) / 4]


def _audit_rows(strong_decision_layer, tags=None):
    return [{"slot": 10 + i, "decision": [0, i], "improvement": OWN[i], "strong_decision": [strong_decision_layer, i],
             "best_improvement": [0.125, -1.0, 0.5, 0.625, 0.75][i], "candidates": CANDIDATES["strong_candidates"][i],
             "improvements": CANDIDATES["strong_improvement"][i], **(tags[i >= 2] if tags else {})} for i in range(5)]


def _report(run, entries, tags):
    """Both halves of the report over a plan's entries, as the two loops call them around ``read_state``."""
    trace = []
    made = [frontier._report_launched(run, trace, e, row0, k, tags[e]) for e, (s, row0, k) in enumerate(entries)]
    assert all(a is b for a, b in zip(made, trace)) and len(trace) == len(entries)
    values = frontier._witness_values(run)
    for (s, row0, k), t in zip(entries, trace):
        frontier._report_read(run, t, s, row0, k, RECORDS[s], values)
    return trace


def _concatenated(one, two):
    """The one-job report of rows [0, 5) is the two entries' reports joined key by key, the tags and the per-record keys aside."""
    per_record = ("global_lb", "global_ub", "witness_value")
    assert set(one) == set(two[0]) - set(TAGS[0]) == set(two[1]) - set(TAGS[1]) and not set(one) & set(TAGS[0])
    for key in set(one) - set(per_record):
        assert one[key] == two[0][key] + two[1][key], key


def test_the_report_of_a_round_is_per_entry_the_dict_written_out_by_hand():
    # 1. and 2.: "strong" mode, traced and audited: the one-job entry, then the two entries of a plan
    run = _launched(audit=[])
    one, = _report(run, ONE_JOB, [{}])
    assert one == {**ROWS, **CANDIDATES} and run.strong_audit == _audit_rows(0)
    run = _launched(audit=[])
    two = _report(run, TWO_JOBS, TAGS)
    assert two == [{**TAGS[0], **ENTRY_0}, {**TAGS[1], **ENTRY_1}] and run.strong_audit == _audit_rows(0, TAGS)
    _concatenated(one, two)
    # 3. "gnn" with an audit: the table's own decisions are read, and the trace has no strong key
    run = _launched("gnn", audit=[])
    one, = _report(run, ONE_JOB, [{}])
    assert one == ROWS and run.strong_audit == _audit_rows(1)
    run = _launched("gnn", audit=[])
    two = _report(run, TWO_JOBS, TAGS)
    assert run.strong_audit == _audit_rows(1, TAGS) and not any(key.startswith("strong") for t in two for key in t)
    _concatenated(one, two)
    run = _launched("gnn")                                    # (neither: the strong rows are not read at all)
    del run.cand0, run.s_best, run.cand_dec, run.s_imp, run.s_dec, run.parent_bound
    assert _report(run, ONE_JOB, [{}]) == [ROWS]
    # 4. a learning round that took a step, and one that took none: the bounds stay
    step = {"imitation_loss": [0.0, 0.5, 1.0, 1.5, 2.0], "imitation_regret": [0.0, 0.25, 0.5, 0.75, 1.0],
            "imitation_report": [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6], [4, 5, 6, 7]]}
    one, = _report(_launched(imitate=2, last_imitation=5), ONE_JOB, [{}])
    assert one == {**ROWS, **CANDIDATES, **step, "global_lb": -1.0, "global_ub": 1.0}
    two = _report(_launched(imitate=2, last_imitation=5), TWO_JOBS, TAGS)
    assert two[1] == {**TAGS[1], **ENTRY_1, **{key: v[2:] for key, v in step.items()}, "global_lb": -4.0, "global_ub": 3.0}
    assert (two[0]["global_lb"], two[0]["global_ub"]) == (-1.0, 1.0)
    _concatenated(one, two)
    one, = _report(_launched(imitate=2, last_imitation=0), ONE_JOB, [{}])
    assert one == {**ROWS, **CANDIDATES, "global_lb": -1.0, "global_ub": 1.0}
    two = _report(_launched(imitate=2, last_imitation=0), TWO_JOBS, TAGS)
    assert two[1] == {**TAGS[1], **ENTRY_1, "global_lb": -4.0, "global_ub": 3.0}
    _concatenated(one, two)
    # 5. a run with a witness: element 0, or element ``segment``, of the one host copy
    one, = _report(_launched("gnn", witness=True), ONE_JOB, [{}])
    assert one == {**ROWS, "global_ub": 1.0, "witness_value": 7.0}
    two = _report(_launched("gnn", witness=True), TWO_JOBS, TAGS)
    assert [(t["global_ub"], t["witness_value"]) for t in two] == [(1.0, 7.0), (3.0, 9.0)]
    _concatenated(one, two)
    # an untraced, unaudited run reads nothing: no tensor is there to be read
    import types
    bare = types.SimpleNamespace(branching="strong", strong_audit=None, cand_entry=[0, 7])
    assert frontier._report_launched(bare, None, 0, 0, 5, {}) is None


def test_the_tally_of_a_job_is_counted_per_entry():
    import types
    record = _record(3, 5)
    record[_lib.FS_KEPT], record[_lib.FS_CLOSED], record[_lib.FS_INFEASIBLE] = 3.0, 2.0, 1.0
    tally = frontier._new_tally()
    assert tally == {"rounds": 0, "domains_bounded": 1, "branches": 0, "kw_bounded": 0, "strong_bounded": 0}       # the root
    frontier._tally_entry(types.SimpleNamespace(threshold=None, m_e=[0], cand_entry=None), tally, 1, 3, record)     # (m_e is not a plan's: not read)
    assert tally == {"rounds": 1, "domains_bounded": 7, "branches": 3, "kw_bounded": 0, "strong_bounded": 0}
    frontier._tally_entry(types.SimpleNamespace(threshold=0.5, m_e=[1, 2, 3], cand_entry=None), tally, 1, 4, record)      # both children of 2 KW pairs
    assert tally == {"rounds": 2, "domains_bounded": 17, "branches": 7, "kw_bounded": 2, "strong_bounded": 0}
    frontier._tally_entry(types.SimpleNamespace(threshold=None, m_e=[0], cand_entry=[0, 4, 9]), tally, 1, 2, record)      # 5 candidates, two children each
    assert tally == {"rounds": 3, "domains_bounded": 23, "branches": 9, "kw_bounded": 2, "strong_bounded": 10}


# ---- the options of a run ------------------------------------------------------------------------------------------------------------------
def _options(choice=None, **kw):
    import types
    run = types.SimpleNamespace()
    frontier._Round._set_options(run, choice, **kw)
    return run


def test_the_option_setter_leaves_every_kind_of_run_with_every_attribute():
    """``_Round._set_options`` on a bare object with the keywords of ``FrontierRun``, ``JobsRun`` and ``StrongJobsRun``: what ``_launch``,
    ``_buffers`` and the loops read exists, off where the kind does not take it; the derived values; the engine a run takes."""
    import types
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice

    class Choice(GraphChoice):
        model = types.SimpleNamespace(engine=lambda: "the model's engine")

        def __init__(self):
            pass

        def _eng(self):
            return "the engine with its optimizer"
    upper = {"witness": None, "pgd_steps": None, "pgd_step": 1.0 / 64, "pgd_restarts": None, "pgd_seed": 0}
    jobs = {"branching_threshold": None, "kwbd_threshold": 10, "sparsest_layer": 0, "decision_threshold": 0.001, "branching": "gnn", **upper}
    strong = {**jobs, "imitate": None, "imitate_margin": 1.0, "strong_candidates": None, "strong_chunk": 256, "strong_audit": None, "branching": "strong"}
    one = {**strong, "online_threshold": None, "branching": "gnn"}
    off = {"threshold": None, "online": None, "kwbd_threshold": 10, "sparsest_layer": 0, "decision_threshold": 0.001, "witness_on": False,
           "witness_to": None, "pgd_steps": None, "pgd_step": 1.0 / 64, "restarts": 0, "pgd_seed": 0, "imitate": None, "imitate_margin": 1.0, "learns": False,
           "strong_M": 0, "strong_chunk": 256, "strong_audit": None, "round": 0, "k": 0, "strong_n": 0, "imitation_steps": 0, "imitation_rows": 0,
           "last_imitation": 0, "learning": False, "imitate_pending": False, "cand_entry": None, "im_table": None}
    assert vars(_options(**one)) == vars(_options(**jobs)) == vars(_options()) == {**off, "branching": "gnn", "strong_on": False}
    assert vars(_options(**strong)) == {**off, "branching": "strong", "strong_on": True}
    # the derived values
    audit, point = [], []
    assert _options(strong_audit=audit).strong_on and _options(strong_audit=audit).strong_audit is audit and _options(strong_audit=audit).branching == "gnn"
    assert _options(Choice(), imitate=3).strong_on and _options(Choice(), imitate=3, imitate_margin=2).imitate_margin == 2.0
    assert not _options(branching="babsr").strong_on and _options(branching="babsr", sparsest_layer=True).sparsest_layer == 1
    assert (_options(branching="strong", strong_candidates=8).strong_M, _options(branching="strong", strong_chunk=7).strong_chunk) == (8, 7)
    run = _options(witness=point, pgd_steps=4, pgd_step=1, pgd_restarts=3, pgd_seed=11)
    assert (run.witness_on, run.witness_to is point, run.pgd_steps, run.pgd_step, run.restarts, run.pgd_seed) == (True, True, 4, 1.0, 3, 11)
    assert type(run.pgd_step) is float and _options(pgd_steps=4, pgd_restarts=0).restarts == 0
    run = _options(branching_threshold=0.25, kwbd_threshold=3, sparsest_layer=1, decision_threshold=1)
    assert (run.threshold, run.kwbd_threshold, run.sparsest_layer, run.decision_threshold, run.online) == (0.25, 3, 1, 1.0, None)
    run = _options(Choice(), branching_threshold=0.25, online_threshold=5)
    assert (run.online, run.kwbd_threshold, run.learns, run.imitate) == (5, frontier.KWBD_NEVER, True, None)
    # the engine: the one with the optimizer where the parameters move
    engine_of = lambda **kw: frontier._Round._engine_of(_options(Choice(), **kw), Choice())      # noqa: E731
    assert engine_of() == engine_of(branching="strong") == engine_of(strong_audit=[]) == engine_of(branching_threshold=0.5) == "the model's engine"
    assert engine_of(imitate=1) == engine_of(imitate=2, branching="strong") == engine_of(branching_threshold=0.5, online_threshold=1) \
        == "the engine with its optimizer"
    # the checks run in the one stated order: imitate, branching, strong, witness, restarts, threshold, online
    order = [("imitate", {"imitate": 0}), ("branching", {"branching": "x"}), ("strong_chunk", {"strong_chunk": 0}), ("pgd_step", {"pgd_step": 0}),
             ("pgd_seed", {"pgd_seed": -1}), ("branching_threshold", {"branching_threshold": 2}), ("online_threshold", {"online_threshold": 0})]
    for i, (name, _) in enumerate(order):
        bad = {}
        for _, kw in order[i:]:
            bad.update(kw)
        with pytest.raises(ValueError, match=name + " = "):
            _options(**bad)
