"""CPU: online learning for every job of a many-property frontier.  gnnb_frontier_learn_jobs and its workspace
sizer are declared, bound and exported; the ABI stays 2 with ten options and the profile class list is the one it was (the two new kernels
launch under k_frontier_learn's class); the entry point refuses, with a message that names it, a null handle, a null plan, no entry and n
outside 1..32767, and the sizer returns 0 for a null handle; ``verify_properties_online`` and ``OnlineJobsRun`` have the documented
signatures, the older ones are unchanged, and bad arguments are refused before a device is touched; the restatement of the per-entry walk
and the compaction (tests/frontier_jobs_online_twin.py) on rows worked out by hand.  (A handle needs a GPU to exist: the refusals behind
it -- online_threshold < 1, a null argument, a short workspace, a call before bind -- are in tests/test_gpu_frontier_jobs_online.py.)"""
import ctypes as C
import inspect
import math

import pytest
from torch import nn

from gnn_branching_amd import _lib, frontier
from tests.frontier_jobs_online_twin import learn_jobs_reference
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job
from tests.test_frontier_shortlist_cpu import CLASSES

NEW = ("gnnb_frontier_learn_jobs_workspace_bytes", "gnnb_frontier_learn_jobs")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def learn_jobs(lib, h, n_entries, n, online_threshold=1, plan=True):
    """The entry point with handle ``h``; every pointer is null (nothing may be dereferenced)."""
    plan_s = _lib.Plan(None, None, n_entries, n, 1, 8)
    return lib.gnnb_frontier_learn_jobs(h, C.byref(plan_s) if plan else None, *([None] * 5), online_threshold, *([None] * 5), None, 0, None)


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2                       # the additions are additive
    assert "#define GNNB_ABI_VERSION 2" in header


def test_no_option_and_no_profile_class_was_added(lib):
    options = sorted(lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count()))
    assert options == sorted(_lib.OPTIONS) and len(options) == 10
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    assert classes == CLASSES and classes.count("k_frontier_learn") == 1
    assert not any(c in ("k_frontier_learn_jobs", "k_frontier_learn_compact") for c in classes)      # they launch under k_frontier_learn


def test_null_handle_is_refused_with_a_message(lib):
    assert learn_jobs(lib, None, 1, 2) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_learn_jobs" in msg and b"null handle" in msg, msg
    assert learn_jobs(lib, None, 1, 2, online_threshold=0) == -1      # the plan and the handle come first
    assert b"gnnb_frontier_learn_jobs" in lib.gnnb_last_error() and b"null handle" in lib.gnnb_last_error()


@pytest.mark.parametrize("n_entries,n", [(1, 0), (1, -3), (0, 2), (1, 32768)])
def test_no_entry_or_a_row_count_outside_the_range_is_refused_with_a_message(lib, n_entries, n):
    assert learn_jobs(lib, None, n_entries, n) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_frontier_learn_jobs" in msg and f"n = {n} ".encode() in msg and b"null handle" not in msg, msg


def test_a_null_plan_is_refused(lib):
    assert learn_jobs(lib, None, 1, 1, plan=False) == -1
    assert b"gnnb_frontier_learn_jobs: null plan" in lib.gnnb_last_error()


def test_workspace_sizer_returns_zero_for_a_null_handle(lib):
    assert lib.gnnb_frontier_learn_jobs_workspace_bytes(None, 4) == 0


# ---- signatures -----------------------------------------------------------------------------------------------------------------------
def test_the_signature_is_the_documented_one():
    sig = inspect.signature(frontier.verify_properties_online)
    assert list(sig.parameters) == ["choice", "fixed_layers", "jobs", "branching_threshold", "online_threshold", "K", "segments", "capacity", "n_iter",
                                    "lr", "eps", "max_rounds", "sparsest_layer", "decision_threshold", "repack", "log", "trace", "stats", "learned"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["K"], d["segments"], d["capacity"], d["n_iter"], d["lr"], d["eps"], d["max_rounds"]) == (16, None, None, 20, 0.1, 1e-4, 50)
    assert (d["sparsest_layer"], d["decision_threshold"], d["repack"], d["trace"], d["stats"], d["learned"]) == (0, 0.001, "host", None, None, None)
    assert d["branching_threshold"] is inspect.Parameter.empty and d["online_threshold"] is inspect.Parameter.empty
    assert "kwbd_threshold" not in sig.parameters            # the online loop has no table of inefficient KW points


def test_the_run_is_a_jobsrun_with_its_parameters_first():
    assert issubclass(frontier.OnlineJobsRun, frontier.JobsRun)
    base = list(inspect.signature(frontier.JobsRun.__init__).parameters)
    mine = list(inspect.signature(frontier.OnlineJobsRun.__init__).parameters)
    assert mine == base + ["online_threshold", "repack"]
    assert inspect.signature(frontier.OnlineJobsRun.__init__).parameters["repack"].default == "host"


def test_the_older_signatures_are_unchanged():
    assert list(inspect.signature(frontier.JobsRun.__init__).parameters) == [
        "self", "choice", "fixed_layers", "jobs", "in_shape", "K", "segments", "cap", "n_iter", "lr", "eps", "branching_threshold", "kwbd_threshold",
        "sparsest_layer", "decision_threshold", "witness", "pgd_steps", "pgd_step", "pgd_restarts", "pgd_seed", "branching"]
    assert list(inspect.signature(frontier.verify_properties_threshold).parameters) == [
        "choice", "fixed_layers", "jobs", "branching_threshold", "K", "segments", "capacity", "n_iter", "lr", "eps", "max_rounds", "kwbd_threshold",
        "sparsest_layer", "decision_threshold", "log", "trace", "stats"]
    assert list(inspect.signature(frontier.verify_properties).parameters) == ["choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr",
                                                                            "eps", "max_rounds", "log", "trace"]
    with pytest.raises(TypeError):                           # they keep refusing the option
        frontier.verify_properties(NoDevice(), [], [job()], online_threshold=5)
    with pytest.raises(TypeError):
        frontier.verify_properties_threshold(NoDevice(), [], [job()], 0.5, online_threshold=5)


# ---- arguments, before a device is touched --------------------------------------------------------------------------------------------
# tests/test_frontier_online_cpu.py's bad argument lists, for a function without a kwbd_threshold (the three lists that set one: below)
@pytest.mark.parametrize("threshold,online", [(0.5, 0), (0.5, -1), (0.5, 2.0), (0.5, True), (0.5, "5"), (0.5, None),      # not an integer >= 1
                                              (None, 5)])                                                               # without a branching_threshold
def test_bad_online_arguments_are_rejected_before_a_device_is_touched(threshold, online):
    with pytest.raises(ValueError):
        frontier.verify_properties_online(NoDevice(), [], [job(), job()], threshold, online, K=4)


@pytest.mark.parametrize("kwbd", [3, 2 ** 31 - 1, 0])
def test_a_kwbd_threshold_is_not_taken(kwbd):
    with pytest.raises(TypeError):
        frontier.verify_properties_online(NoDevice(), [], [job(), job()], 0.5, 5, K=4, kwbd_threshold=kwbd)
    with pytest.raises(ValueError, match="kwbd_threshold"):  # the run class has JobsRun's parameter: anything but the default is refused
        frontier.OnlineJobsRun(NoDevice(), [], [job(), job()], (3, 4, 4), 4, 2, 17, 20, 0.1, 1e-4, branching_threshold=0.5, kwbd_threshold=kwbd,
                               online_threshold=5)


def test_a_missing_branching_threshold_has_verify_properties_threshold_s_message():
    with pytest.raises(ValueError, match=r"branching_threshold = None: a number with 0 < branching_threshold <= 1"):
        frontier.verify_properties_online(NoDevice(), [], [job(), job()], None, 5)


@pytest.mark.parametrize("online_threshold", [1, 5, 2 ** 30])
def test_a_choice_that_is_no_online_graphchoice_is_a_type_error(online_threshold):
    """Valid numbers, but the choice owns no lr / wd: refused before anything of it is touched (NoDevice raises on any attribute)."""
    with pytest.raises(TypeError, match="graph_score_online"):
        frontier.verify_properties_online(NoDevice(), [], [job(), job()], 0.5, online_threshold, K=4)
    with pytest.raises(TypeError, match="graph_score_online"):
        frontier.verify_properties_online(object(), [], [job()], 1.0, online_threshold)


@pytest.mark.parametrize("kw", [{"K": 0}, {"K": True}, {"K": 4, "capacity": 8}, {"n_iter": -1}, {"max_rounds": -1}, {"eps": -1.0}, {"lr": 0.0},
                                {"segments": 0}, {"segments": True}, {"K": 16, "segments": 1024}])
def test_bad_jobs_arguments_come_first(kw):
    """``_check_jobs_args`` runs before the online checks: a ValueError, not the TypeError the stand-in choice would get."""
    with pytest.raises(ValueError):
        frontier.verify_properties_online(NoDevice(), [], [job(), job()], 0.5, 5, **kw)
    with pytest.raises(ValueError, match="no job"):
        frontier.verify_properties_online(NoDevice(), [], [], 0.5, 5)
    with pytest.raises(ValueError, match="property layer"):
        frontier.verify_properties_online(NoDevice(), [], [job(), job(prop=nn.Linear(5, 2))], 0.5, 5)


@pytest.mark.parametrize("threshold", [0, -0.2, 1.5, float("nan"), "0.2", True])
def test_a_bad_branching_threshold_comes_before_the_choice(threshold):
    with pytest.raises(ValueError, match="branching_threshold"):
        frontier.verify_properties_online(NoDevice(), [], [job()], threshold, 5)


def test_repack_and_learned_are_checked():
    """Behind the choice's type in the order of the checks, so the stand-in here is a real online GraphChoice class instance without a
    device: ``object.__new__`` makes one that owns nothing."""
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice
    choice = object.__new__(GraphChoice)
    with pytest.raises(ValueError, match="repack"):
        frontier.verify_properties_online(choice, [], [job()], 0.5, 5, repack="gpu")
    with pytest.raises(ValueError, match="learned"):
        frontier.verify_properties_online(choice, [], [job()], 0.5, 5, learned=[])


# ---- the walk and the compaction on rows worked out by hand ---------------------------------------------------------------------------
RELU = [4, 3]                                                 # flat indices: layer 0 -> 0..3, layer 1 -> 4..6


def rows_of(spec):
    """spec: per global row (gnn decision, kw decision, used, gnn_imp, kw_imp)."""
    return {"gnn_dec": [r[0] for r in spec], "kw_dec": [r[1] for r in spec], "used": [r[2] for r in spec], "gnn_imp": [r[3] for r in spec],
            "kw_imp": [r[4] for r in spec]}


def test_a_count_one_below_the_threshold_and_one_reaching_it():
    """online_threshold 3; node 1 has lost once (after the row: 2, no learn row), node 5 twice (after the row: 3, a learn row)."""
    rows = rows_of([([0, 1], [1, 0], 1, 0.2, 0.25), ([1, 1], [0, 3], 1, 0.2, 0.5)])
    wrong = {0: [0, 1, 0, 0, 0, 2, 0]}
    got = learn_jobs_reference(RELU, [(0, 0, 2)], rows, wrong, 3)
    assert got[:4] == ([1], [3], [1.0], [1, 1]) and got[4] == {0: [0, 2, 0, 0, 0, 3, 0]}
    assert wrong == {0: [0, 1, 0, 0, 0, 2, 0]}               # the input tables are not written


def test_two_rows_of_one_entry_naming_one_node_both_count():
    rows = rows_of([([0, 2], [1, 0], 1, 0.2, 0.25), ([0, 2], [1, 2], 1, 0.3, 0.35)])
    got = learn_jobs_reference(RELU, [(0, 0, 2)], rows, {0: [0] * 7}, 2)
    assert got[:4] == ([1], [6], [0.0], [1, 1]) and got[4][0][2] == 2      # the second row crosses the threshold the first one approached


def test_the_same_node_in_two_entries_meets_two_tables():
    """Rows 0 and 1 belong to segments 1 and 0 and both name node 2 at online_threshold 2: segment 1's table holds one earlier loss (a
    learn row), segment 0's none (no learn row).  Neither entry sees the other's count."""
    rows = rows_of([([0, 2], [1, 0], 1, 0.2, 0.25), ([0, 2], [1, 0], 1, 0.2, 0.25)])
    wrong = {0: [0] * 7, 1: [0, 0, 1, 0, 0, 0, 0]}
    got = learn_jobs_reference(RELU, [(1, 0, 1), (0, 1, 1)], rows, wrong, 2)
    assert got[:4] == ([0], [4], [0.0], [1, 0, 1]) and got[4] == {0: [0, 0, 1, 0, 0, 0, 0], 1: [0, 0, 2, 0, 0, 0, 0]}
    swapped = learn_jobs_reference(RELU, [(0, 0, 1), (1, 1, 1)], rows, wrong, 2)      # the other assignment: the learn row is GLOBAL row 1
    assert swapped[:4] == ([1], [4], [0.0], [0, 1, 1]) and swapped[4] == got[4]


def test_an_empty_entry_between_two_others():
    used = ([0, 0], [1, 1], 1, 0.2, 0.5)
    lost = ([0, 1], [1, 1], 0, 0.2, 0.1)                     # the GNN pair stayed: no count
    rows = rows_of([used, used, lost, ([0, 3], [1, 2], 1, 0.2, 0.25)])
    got = learn_jobs_reference(RELU, [(2, 0, 2), (0, 2, 1), (1, 3, 1)], rows, {s: [0] * 7 for s in range(3)}, 1)
    assert got[:4] == ([0, 1, 3], [5, 5, 6], [1.0, 1.0, 0.0], [2, 0, 1, 3])
    assert got[4] == {2: [2, 0, 0, 0, 0, 0, 0], 0: [0] * 7, 1: [0, 0, 0, 1, 0, 0, 0]}


def test_a_row_without_a_node_or_with_a_node_outside_its_layer_is_skipped():
    rows = rows_of([([-1, -1], [1, 0], 1, 0.2, 0.5), ([0, 4], [1, 0], 1, 0.2, 0.5), ([1, 3], [0, 0], 1, 0.2, 0.5), ([0, 0], [-1, -1], 1, 0.2, 0.5),
                    ([0, 0], [1, 3], 1, 0.2, 0.5), ([1, 2], [0, 0], 1, 0.2, 0.5)])
    got = learn_jobs_reference(RELU, [(0, 0, 6)], rows, {0: [0] * 7}, 1)
    assert got[:4] == ([5], [0], [1.0], [1, 1]) and got[4] == {0: [0, 0, 0, 0, 0, 0, 1]}      # one past a layer is not the next layer's first node


def test_improve_is_strictly_greater_than_a_tenth():
    """0.2 - 0.1 is 0.1 in fp64: not greater; one ulp above is."""
    assert 0.2 - 0.1 == 0.1
    rows = rows_of([([0, 0], [1, 0], 1, 0.1, 0.2), ([0, 1], [1, 0], 1, 0.1, math.nextafter(0.2, 1.0))])
    got = learn_jobs_reference(RELU, [(0, 0, 2)], rows, {0: [0] * 7}, 1)
    assert got[:4] == ([0, 1], [4, 4], [0.0, 1.0], [2, 2])
