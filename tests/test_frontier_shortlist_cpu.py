"""CPU: shortlisting the strong-branching candidates by the GNN's scores as well.  gnnb_strong_list_union and its
workspace sizer are declared, bound and exported; the ABI stays 2 with ten options and the profile class list is the one it was (the two new
kernels launch under k_strong_count's and k_strong_compact's classes); the entry point refuses, with a message that names it, a null
handle, K outside 1..32767 and a count below 1; ``frontier.Shortlist`` travels as the VALUE of ``strong_candidates`` -- no signature
changed --, its bad values are refused before a device is touched and ``Shortlist(babsr=M)`` sets a run's options exactly as
``strong_candidates=M`` does; the twin of the rule on rows worked out by hand.  (A handle needs a GPU to exist: the refusals behind it
-- a null argument, a short workspace, a call before bind -- are in tests/test_gpu_shortlist.py.)"""
import inspect

import pytest
import torch
from torch import nn

from gnn_branching_amd import _lib, frontier
from gnn_branching_amd.frontier import Shortlist
from gnn_branching_amd.graphnet.graph_conv import GraphNet
from tests.frontier_shortlist_twin import shortlist_of, union_of, union_reference
from tests.test_frontier_cpu import NoDevice, _options
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_strong_list_union_workspace_bytes", "gnnb_strong_list_union")
NAN = float("nan")
# the profile classes before this feature, in order: no class was added, none changed its number
CLASSES = ["k_embed", "k_pre", "k_pre_inp", "k_conv_fwd", "k_convT_bwd", "k_dense_agg", "k_prop", "k_node_update", "k_input_update", "k_score",
           "k_argmax", "k_gather", "k_gather_input_update", "k_classify", "k_livesum", "k_top", "k_gather_update", "k_kw_first", "k_kw_layer",
           "k_kw_flag", "k_dual_ascent", "k_frontier_gather", "k_frontier_expand", "k_net_eval", "k_frontier_resolve", "k_frontier_decide",
           "k_frontier_store", "k_frontier_pick_jobs", "k_frontier_rows_jobs", "k_frontier_decide_jobs", "k_frontier_candidates",
           "k_frontier_fallback", "k_frontier_choose", "k_frontier_choose_copy", "k_frontier_fallback_jobs", "k_frontier_select_jobs",
           "k_frontier_rows_sel", "k_frontier_choose_jobs", "k_frontier_learn", "k_trows_gather", "k_net_descend", "k_frontier_witness",
           "k_frontier_witness_jobs", "k_net_starts", "k_net_descend_tile", "k_net_starts_pick", "k_frontier_babsr_decide",
           "k_frontier_babsr_decide_jobs", "k_strong_count", "k_strong_compact", "k_strong_pick"]


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def call(lib, h, K, top_a=2, top_b=3):
    """The entry point with handle ``h``; every pointer is null (nothing may be dereferenced)."""
    return lib.gnnb_strong_list_union(h, None, None, K, None, None, top_a, None, top_b, None, None, None, None, None, None, 0, None)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2 and "GNNB_ABI_VERSION 2" in header.replace("  ", " ")
    options = [lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())]
    assert sorted(options) == sorted(_lib.OPTIONS) and len(options) == 10
    from gnn_branching_amd.engine import ScorerEngine
    assert callable(ScorerEngine.strong_list_union)
    source = open(_lib.CSRC + "/gnnb_k_strong.h").read()
    assert "void k_strong_union_count(" in source and "void k_strong_union_compact(" in source
    assert source.count("bit >>= 1") == 1                    # one bisection: the union's cuts are k_strong_count's


def test_the_profile_class_list_is_the_one_it_was(lib):
    assert [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())] == CLASSES


def test_the_workspace_sizer_returns_zero_for_a_null_handle(lib):
    assert lib.gnnb_strong_list_union_workspace_bytes(None, 4) == 0


def test_a_null_handle_is_refused_with_a_message(lib):
    assert call(lib, None, 2) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_list_union:" in msg and b"null handle" in msg, msg


@pytest.mark.parametrize("K", [0, -3, 32768])
def test_a_row_count_outside_the_range_is_refused_with_a_message(lib, K):
    assert call(lib, None, K) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_list_union:" in msg and f"K = {K} ".encode() in msg and b"null handle" not in msg, msg
    for ok in (1, 32767):                                    # the edges of the range pass this check (and stop at the null handle)
        assert call(lib, None, ok) == -1 and b"null handle" in lib.gnnb_last_error(), ok


@pytest.mark.parametrize("tops,what", [((0, 3), b"top_a = 0 "), ((-1, 3), b"top_a = -1 "), ((2, 0), b"top_b = 0 "), ((2, -5), b"top_b = -5 "),
                                       ((0, 0), b"top_a = 0 ")])
def test_a_count_below_one_is_refused_with_a_message(lib, tops, what):
    assert call(lib, None, 2, *tops) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_list_union:" in msg and what in msg and b"gnnb_strong_list" in msg and b"null handle" not in msg, msg
    assert call(lib, None, 2, 1, 1) == -1 and b"null handle" in lib.gnnb_last_error()      # 1 and 1 pass this check


# ---- the Python arguments ---------------------------------------------------------------------------------------------------------------
def test_no_signature_changed():
    """The option travels as the value of ``strong_candidates``: the parameter lists the older tests pin are the ones they were."""
    tail = ["imitate", "imitate_margin", "strong_candidates", "strong_chunk", "strong_audit", "branching"]
    for f in (frontier.branch_and_bound_frontier, frontier.FrontierRun.__init__, frontier.StrongJobsRun.__init__, frontier.verify_properties_strong):
        params = inspect.signature(f).parameters
        assert list(params)[-6:] == tail and params["strong_candidates"].default is None, f
    assert list(inspect.signature(frontier.verify_properties_strong).parameters) == [
        "choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr", "eps", "max_rounds", "log", "trace", "stats", "learned"] + tail
    assert not any(p.startswith("strong") for p in inspect.signature(frontier.JobsRun.__init__).parameters)
    assert list(inspect.signature(Shortlist.__init__).parameters) == ["self", "babsr", "gnn"]
    assert (Shortlist().babsr, Shortlist().gnn, Shortlist(3).babsr, Shortlist(gnn=2).gnn) == (None, None, 3, 2)
    assert frontier._Round.strong_G == 0 and frontier._Round.cand_src is None


class Net(GraphNet):
    """A GraphNet nothing may run: a choice with a scorer, as the checks see it."""

    def __init__(self):
        nn.Module.__init__(self)

    def engine(self):
        raise AssertionError("touched the scorer (engine) before checking the arguments")


class Scorer:
    def __init__(self):
        self.model = Net()


def online_scorer():
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice

    class Online(GraphChoice):
        def __init__(self):
            self.model = Net()

        def _eng(self):
            raise AssertionError("touched the scorer (_eng) before checking the arguments")
    return Online()


BAD = [Shortlist(), Shortlist(babsr=0), Shortlist(babsr=-2), Shortlist(babsr=True), Shortlist(babsr=2.0), Shortlist(babsr="8"), Shortlist(gnn=0),
       Shortlist(gnn=True), Shortlist(gnn=4.0), Shortlist(gnn="4"), Shortlist(babsr=8, gnn=0), Shortlist(babsr=0, gnn=4), Shortlist(babsr=[8], gnn=4)]


@pytest.mark.parametrize("value", BAD, ids=repr)
@pytest.mark.parametrize("branching", ["strong", "gnn"])
def test_a_bad_shortlist_is_refused_before_a_device_is_touched(value, branching):
    extra = {} if branching == "strong" else {"strong_audit": []}
    with pytest.raises(ValueError, match="strong_candidates = Shortlist"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], branching=branching, strong_candidates=value, **extra)
    with pytest.raises(ValueError, match="strong_candidates = Shortlist"):
        frontier.verify_properties_strong(NoDevice(), [], [job(), job()], branching=branching, strong_candidates=value, **extra)


def test_a_gnn_count_needs_a_scorer_to_run():
    for value in (Shortlist(gnn=4), Shortlist(babsr=8, gnn=4)):
        for choice in (object(), Scorer().model, type("NoModel", (), {"model": None})()):      # no model, or one that is no GraphNet
            with pytest.raises(ValueError, match="strong_candidates = Shortlist.*GraphNet"):
                frontier.branch_and_bound_frontier(None, choice, [], branching="strong", strong_candidates=value)
            with pytest.raises(ValueError, match="strong_candidates = Shortlist.*GraphNet"):
                frontier.verify_properties_strong(choice, [], [job()], strong_candidates=value)
        with pytest.raises(ValueError, match='strong_candidates = Shortlist.*"babsr"'):      # BaBSR never prepares the scorer's inputs
            frontier.branch_and_bound_frontier(None, Scorer(), [], branching="babsr", strong_audit=[], strong_candidates=value)
    # a BaBSR count alone asks nothing of the choice: the audit next to a BaBSR run takes it, as it takes an integer
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [nn.Linear(5, 1)], K=4, branching="babsr", strong_audit=[], strong_candidates=Shortlist(8))


def test_the_older_refusals_keep_their_messages():
    for bad in ("8", 2.0, True, 0):
        with pytest.raises(ValueError, match=r"strong_candidates = .*: None \(every undecided node\), or an integer >= 1"):
            frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], branching="strong", strong_candidates=bad)
    with pytest.raises(ValueError, match="strong_candidates = Shortlist.* without branching=\"strong\", a strong_audit or imitate"):
        frontier.branch_and_bound_frontier(NoDevice(), Scorer(), [], strong_candidates=Shortlist(gnn=4))


@pytest.mark.parametrize("kw", [{"branching": "strong", "strong_candidates": Shortlist(gnn=4)}, {"branching": "strong", "strong_candidates": Shortlist(8, 4)},
                                {"strong_audit": [], "strong_candidates": Shortlist(gnn=1)}, {"strong_audit": [], "strong_candidates": Shortlist(16, gnn=1)},
                                {"branching": "strong", "strong_candidates": Shortlist(babsr=8), "strong_chunk": 7}])
def test_good_shortlists_reach_the_engine(kw):
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.branch_and_bound_frontier(NoDevice(), Scorer(), [nn.Linear(5, 1)], K=4, **kw)
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.verify_properties_strong(Scorer(), [], [job(), job()], K=4, **{"branching": "gnn", **kw})
    with pytest.raises(AssertionError, match="touched the scorer"):      # a run that learns: the engine with the optimizer
        frontier.branch_and_bound_frontier(NoDevice(), online_scorer(), [nn.Linear(5, 1)], K=4, imitate=1, **{k: v for k, v in kw.items() if k != "strong_audit"})


def test_a_babsr_shortlist_sets_the_options_an_integer_sets():
    """``_Round._set_options`` on a bare object: ``Shortlist(babsr=M)`` leaves exactly the attributes ``strong_candidates=M`` leaves; a gnn
    count adds ``strong_G`` and nothing else."""
    for kw in ({"branching": "strong"}, {"strong_audit": None, "branching": "strong", "strong_chunk": 7}):
        assert vars(_options(strong_candidates=Shortlist(babsr=8), **kw)) == vars(_options(strong_candidates=8, **kw))
        assert vars(_options(strong_candidates=Shortlist(8, None), **kw))["strong_M"] == 8
    plain = vars(_options(strong_candidates=8, branching="strong"))
    assert "strong_G" not in plain and "strong_G" not in vars(_options(branching="strong"))
    both = vars(_options(Scorer(), strong_candidates=Shortlist(babsr=8, gnn=4), branching="strong"))
    assert both == {**plain, "strong_G": 4}
    alone = vars(_options(Scorer(), strong_candidates=Shortlist(gnn=4), branching="strong"))
    assert alone == {**plain, "strong_M": 0, "strong_G": 4}
    audit = []
    run = _options(Scorer(), strong_candidates=Shortlist(16, 2), strong_audit=audit)
    assert (run.branching, run.strong_on, run.strong_M, run.strong_G, run.strong_audit is audit) == ("gnn", True, 16, 2, True)
    assert frontier._shortlist_counts(None) == (0, 0) and frontier._shortlist_counts(5) == (5, 0) and frontier._shortlist_counts(Shortlist(gnn=3)) == (0, 3)


def test_the_report_holds_sources_only_in_a_run_with_a_gnn_count():
    """``_strong_rows`` on the hand-made run of tests/test_frontier_cpu.py: no "sources" without a gnn count (the dicts the older tests
    write out by hand), the union's cand_src with both counts, all 2 with the scorer's shortlist alone."""
    from tests.test_frontier_cpu import _launched
    run = _launched(audit=[])
    assert all("sources" not in r for r in frontier._strong_rows(run, 5))
    run.strong_G = 4
    assert [r["sources"] for r in frontier._strong_rows(run, 5)] == [[2, 2], [], [2, 2, 2], [2], [2]]
    run.cand_src = torch.tensor([1, 3, 2, 2, 1, 3, 3], dtype=torch.int32)
    assert [r["sources"] for r in frontier._strong_rows(run, 5)] == [[1, 3], [], [2, 2, 1], [3], [3]]
    assert [r["sources"] for r in frontier._strong_rows(run, 3, 2)] == [[2, 2, 1], [3], [3]]      # an entry of a plan: its own range
    trace = []
    t = frontier._report_launched(run, trace, 0, 0, 5, {})
    assert t["strong_sources"] == [[1, 3], [], [2, 2, 1], [3], [3]] and [a["sources"] for a in run.strong_audit] == t["strong_sources"]


# ---- the twin on rows worked out by hand ----------------------------------------------------------------------------------------------------
def test_the_twin_on_hand_worked_rows():
    relu = [4, 3]
    amb = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0])              # node 2 is decided
    a = torch.tensor([5.0, 1.0, 9.0, 1.0, 1.0, 0.0, -1.0])               # open order: 0, then the tie 1, 3, 4 in index order, 5, 6
    b = torch.tensor([0.0, -0.0, NAN, 0.0, 7.0, 7.0, 7.0])               # the NaN is at the decided node; zeros of both signs tie
    assert union_of(amb, a, 2, b, 2) == ([0, 1, 4, 5], [1, 1, 2, 2])      # disjoint: 2 + 2
    assert union_of(amb, a, 2, b, 4) == ([0, 1, 4, 5, 6], [3, 1, 2, 2, 2])      # B's fourth is the first zero, node 0: both take it
    assert union_of(amb, a, 3, b, 4) == ([0, 1, 3, 4, 5, 6], [3, 1, 1, 2, 2, 2])      # node 4 is inside A's tie run but past A's rank: B takes it
    assert union_of(amb, a, 4, b, 1) == ([0, 1, 3, 4], [1, 1, 1, 3])      # ... and here both take it
    assert union_of(amb, a, 2, a, 1) == ([0, 1], [3, 1])                  # B = A with fewer: A's list
    assert union_of(amb, a, 10, b, 2) == ([0, 1, 3, 4, 5, 6], [1, 1, 1, 3, 3, 1])      # more than there are: all of them
    assert union_of(amb, a, 10, b, 10)[1] == [3] * 6
    for bad in (3, 6):                                                    # a NaN at an undecided node of either array empties the row
        c = b.clone()
        c[bad] = NAN
        assert union_of(amb, a, 2, c, 2) == union_of(amb, c, 2, a, 2) == ([], [])
    assert union_of(torch.zeros(7), a, 2, b, 2) == ([], [])               # nothing undecided
    inf = torch.tensor([-float("inf"), 1.0, 0.0, float("inf"), 1.0, 1.0, 1.0])
    assert union_of(amb, inf, 1, inf, 5) == ([1, 3, 4, 5, 6], [2, 3, 2, 2, 2])      # +-inf are ordinary values
    # the dense lists: row 1 has a slot outside the pool of 9
    ref = union_reference(relu, amb.repeat(3, 1), a.repeat(3, 1), 2, b.repeat(3, 1), 2, [4, 9, 0], 9)
    assert ref == ([0, 4, 4, 8], [0] * 4 + [2] * 4, [4] * 4 + [0] * 4, [[0, 0], [0, 1], [1, 0], [1, 1]] * 2, [1, 1, 2, 2] * 2)
    # one list alone is gnnb_strong_list's, every source its own
    assert shortlist_of(amb, a, 2, None, None) == ([0, 1], [1, 1]) and shortlist_of(amb, None, None, b, 2) == ([4, 5], [2, 2])
    assert shortlist_of(amb, a, 2, b, 2) == union_of(amb, a, 2, b, 2)
