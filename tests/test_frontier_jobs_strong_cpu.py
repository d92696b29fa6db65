"""CPU: strong branching, its audit and the imitation step for many jobs in one pool.  gnnb_strong_rows_jobs is
declared, bound and exported, the ABI stays 2 with ten options, and NO profile class was added: the new kernel k_strong_rows_jobs launches
under k_frontier_rows_sel's, whose copy it shares.  The entry point refuses a null handle, c outside 1..32767 and segments / seg_cap below 1
with a message that names it; ``verify_properties_strong`` has the documented signature, the older loops keep theirs, ``StrongJobsRun`` is a
``JobsRun``, and bad arguments are rejected before a device is touched.  (A handle needs a GPU to exist: the other refusals are in
tests/test_gpu_frontier_jobs_strong.py.)

The BAD lists of tests/test_frontier_strong_cpu.py and tests/test_imitation_cpu.py are applied with ``branching`` defaulting to "gnn", as
those tests ran them (here the default is "strong"); their entries with a branching_threshold or an online_threshold are left out, because
the function takes neither."""
import inspect

import pytest

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job
from tests.test_frontier_strong_cpu import BAD as STRONG_BAD, NEW_KERNELS as STRONG_KERNELS
from tests.test_imitation_cpu import BAD as IMITATE_BAD

NEW = "gnnb_strong_rows_jobs"
ABSENT = ("branching_threshold", "online_threshold")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def call(lib, h, c, segments=3, seg_cap=7):
    """The entry point with handle ``h``; every pointer is null (nothing may be dereferenced)."""
    return lib.gnnb_strong_rows_jobs(h, None, c, segments, seg_cap, None, None, None, None, None, None, None, None, None)


def test_the_symbol_is_declared_bound_and_exported(lib):
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    assert NEW in {s[0] for s in _lib.SYMBOLS} and hasattr(lib, NEW) and NEW + "(" in header
    assert lib.gnnb_abi_version() == 2 and "GNNB_ABI_VERSION 2" in header.replace("  ", " ")
    names = [lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())]
    assert sorted(names) == sorted(_lib.OPTIONS) and len(names) == 10
    from gnn_branching_amd.engine import ScorerEngine
    assert callable(ScorerEngine.strong_rows_jobs)
    source = open(_lib.CSRC + "/gnnb_k_strong.h").read()
    assert "void k_strong_rows_jobs(" in source and "fr_seg_row(" in source
    assert "fr_seg_row(" in open(_lib.CSRC + "/gnnb_k_frontier.h").read()      # one body, shared with k_frontier_rows_sel


def test_the_profile_class_list_is_unchanged(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    assert tuple(classes[-3:]) == STRONG_KERNELS and len(set(classes)) == len(classes)
    assert classes.count("k_frontier_rows_sel") == 1 and "k_strong_rows_jobs" not in classes


def test_null_handle_is_refused_with_a_message(lib):
    assert call(lib, None, 2) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_rows_jobs:" in msg and b"null handle" in msg, msg


@pytest.mark.parametrize("c", [0, -3, 32768])
def test_a_candidate_count_outside_the_range_is_refused_with_a_message(lib, c):
    assert call(lib, None, c) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_rows_jobs:" in msg and f"c = {c} ".encode() in msg and b"null handle" not in msg, msg
    for ok in (1, 32767):                                    # the edges of the range pass this check (and stop at the null handle)
        assert call(lib, None, ok) == -1 and b"null handle" in lib.gnnb_last_error(), ok


@pytest.mark.parametrize("kw,what", [({"segments": 0}, b"segments = 0 "), ({"segments": -2}, b"segments = -2 "), ({"seg_cap": 0}, b"seg_cap = 0 "),
                                     ({"seg_cap": -7}, b"seg_cap = -7 ")])
def test_a_pool_without_a_segment_or_a_slot_is_refused_with_a_message(lib, kw, what):
    assert call(lib, None, 2, **kw) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_strong_rows_jobs:" in msg and what in msg and b"null handle" not in msg, msg
    assert call(lib, None, 2, 1, 1) == -1 and b"null handle" in lib.gnnb_last_error()


# ---- the Python arguments ---------------------------------------------------------------------------------------------------------------
def test_the_signature_is_the_documented_one_and_the_older_ones_stay():
    sig = inspect.signature(frontier.verify_properties_strong)
    assert list(sig.parameters) == ["choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr", "eps", "max_rounds", "log", "trace",
                                    "stats", "learned", "imitate", "imitate_margin", "strong_candidates", "strong_chunk", "strong_audit", "branching"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["K"], d["segments"], d["capacity"], d["n_iter"], d["lr"], d["eps"], d["max_rounds"]) == (16, None, None, 20, 0.1, 1e-4, 50)
    assert (d["log"], d["trace"], d["stats"], d["learned"], d["imitate"], d["imitate_margin"]) == (print, None, None, None, None, 1.0)
    assert (d["strong_candidates"], d["strong_chunk"], d["strong_audit"], d["branching"]) == (None, 256, None, "strong")
    assert issubclass(frontier.StrongJobsRun, frontier.JobsRun)
    own, base = (list(inspect.signature(c.__init__).parameters) for c in (frontier.StrongJobsRun, frontier.JobsRun))
    assert base[-1] == "branching" and not any(p.startswith(("strong", "imitate")) for p in base)
    assert own[:len(base) - 1] == base[:-1]
    assert own[len(base) - 1:] == ["imitate", "imitate_margin", "strong_candidates", "strong_chunk", "strong_audit", "branching"]
    assert own[-8:-6] == ["pgd_restarts", "pgd_seed"] and inspect.signature(frontier.StrongJobsRun.__init__).parameters["branching"].default == "strong"
    assert list(inspect.signature(frontier.FrontierRun.__init__).parameters)[-6:] == own[-6:]
    assert list(inspect.signature(frontier.verify_properties).parameters) == ["choice", "fixed_layers", "jobs", "K", "segments", "capacity", "n_iter", "lr",
                                                                            "eps", "max_rounds", "log", "trace"]
    assert list(inspect.signature(frontier.verify_properties_threshold).parameters)[:4] == ["choice", "fixed_layers", "jobs", "branching_threshold"]
    assert list(inspect.signature(frontier.verify_properties_babsr).parameters)[-5:] == ["sparsest_layer", "decision_threshold", "log", "trace", "stats"]
    assert list(inspect.signature(frontier.branch_and_bound_frontier).parameters)[-6:] == own[-6:]
    # the hook of a one-job run does nothing, and both run classes share the learning half
    assert frontier._Round._strong_chunk_rows(None, 0, 1) is None
    assert frontier.FrontierRun._imitate is frontier._Round._imitate and frontier.StrongJobsRun._strong_chunk_rows is not frontier._Round._strong_chunk_rows


def applicable(bad):
    return [({"branching": "gnn", **kw}, name) for kw, name in bad if not any(a in kw for a in ABSENT)]


def test_the_lists_of_bad_arguments_are_not_empty():
    assert len(applicable(STRONG_BAD)) >= 14 and len(applicable(IMITATE_BAD)) >= 12


@pytest.mark.parametrize("kw,name", applicable(STRONG_BAD) + applicable(IMITATE_BAD))
def test_bad_strong_and_imitate_arguments_are_rejected_before_a_device_is_touched(kw, name):
    with pytest.raises(ValueError, match=name + r"\b"):
        frontier.verify_properties_strong(NoDevice(), [], [job(), job()], **kw)


def test_gnn_without_a_table_and_babsr_name_the_function_to_call():
    with pytest.raises(ValueError, match=r"verify_properties\b"):
        frontier.verify_properties_strong(NoDevice(), [], [job()], branching="gnn")
    for kw in ({}, {"strong_audit": []}):
        with pytest.raises(ValueError, match="verify_properties_babsr"):
            frontier.verify_properties_strong(NoDevice(), [], [job()], branching="babsr", **kw)
    for bad in ("sb", None, "STRONG", 1):
        with pytest.raises(ValueError, match="branching"):
            frontier.verify_properties_strong(NoDevice(), [], [job()], branching=bad)
    with pytest.raises(ValueError, match="learned"):
        frontier.verify_properties_strong(NoDevice(), [], [job()], learned=[])


@pytest.mark.parametrize("kw", [{"K": 0}, {"K": True}, {"K": 4, "capacity": 8}, {"n_iter": -1}, {"max_rounds": -1}, {"eps": -1.0}, {"lr": 0.0},
                                {"segments": 0}, {"segments": 2.0}, {"K": 16, "segments": 1024}])
def test_bad_jobs_arguments_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.verify_properties_strong(NoDevice(), [], [job(), job()], **kw)
    with pytest.raises(ValueError, match="no job"):
        frontier.verify_properties_strong(NoDevice(), [], [])
    with pytest.raises(ValueError, match="pgd_steps"):
        frontier.verify_properties_strong(NoDevice(), [], frontier.FrontierJobs([job()], pgd_steps=-1))


@pytest.mark.parametrize("kw", [{"imitate": 1}, {"imitate": 3, "branching": "gnn"}, {"imitate": 1, "imitate_margin": 0}, {"imitate": 1, "strong_audit": []},
                                {"imitate": 2, "strong_candidates": 8, "strong_chunk": 64, "branching": "gnn"}])
def test_a_choice_that_is_no_online_graphchoice_is_a_type_error(kw):
    for choice in (NoDevice(), object()):
        with pytest.raises(TypeError, match="graph_score_online"):
            frontier.verify_properties_strong(choice, [], [job(), job()], K=4, **kw)


@pytest.mark.parametrize("kw", [{}, {"strong_candidates": 8}, {"strong_chunk": 3}, {"strong_audit": []}, {"branching": "gnn", "strong_audit": []},
                                {"branching": "gnn", "strong_audit": [], "strong_candidates": 4, "strong_chunk": 7}, {"stats": [], "learned": {}}])
def test_good_arguments_reach_the_engine(kw):
    """The checks pass and the first thing touched is the choice's engine: NoDevice raises there, so nothing before it refused."""
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.verify_properties_strong(NoDevice(), [], [job(), job()], K=4, **kw)
    with pytest.raises(AssertionError, match="touched the scorer"):
        frontier.verify_properties_strong(NoDevice(), [], frontier.FrontierJobs([job(), job()], witness=[], pgd_steps=2), K=4, **kw)
