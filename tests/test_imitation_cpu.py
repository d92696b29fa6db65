"""CPU: the imitation step.  gnnb_imitation_step_rows and gnnb_imitation_loss are declared, bound and exported, the
ABI stays 2 with ten options and the profile classes still end in the three strong kernels; the entry points refuse a null handle, a row
count outside its range and a bad margin with a message that names them; ``branch_and_bound_frontier`` and ``FrontierRun`` take ``imitate``
and ``imitate_margin`` directly in front of ``strong_candidates`` and reject bad ones before a device is touched; the twin's rule
(tests/imitation_twin.py) on hand-worked rows.  (A handle needs a GPU to exist: everything else is in tests/test_gpu_imitation.py.)"""
import inspect
import math

import numpy as np
import pytest

from gnn_branching_amd import _lib, frontier
from tests.imitation_twin import NAN, rule, rule_rows
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_strong_cpu import NEW_KERNELS as STRONG_KERNELS

NEW = ("gnnb_imitation_step_rows", "gnnb_imitation_loss")
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def step_rows(lib, h, K, n, margin=1.0):
    return lib.gnnb_imitation_step_rows(h, None, K, None, n, None, margin, None, None, None, None, 0, None)


def loss_hook(lib, h, n, margin=1.0):
    return lib.gnnb_imitation_loss(h, None, None, None, n, margin, None, None, None, None, None, None)


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2 and "GNNB_ABI_VERSION 2" in header.replace("  ", " ")
    source = open(_lib.CSRC + "/gnnb_k_train.h").read()        # (the training kernels; gnnb_train.h, which includes it, holds their host side)
    for k in ("k_tloss_table", "k_tscore_bwd_w_dense"):
        assert "void " + k + "(" in source, k
    assert "gnnb_train.h" in _lib.SOURCES and "gnnb_k_train.h" in _lib.SOURCES


def test_no_option_and_no_profile_class_was_added(lib):
    names = [lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())]
    assert sorted(names) == sorted(_lib.OPTIONS) and len(names) == 10
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    assert tuple(classes[-3:]) == STRONG_KERNELS and len(set(classes)) == len(classes)
    assert classes.count("k_trows_gather") == 1 and not any("tloss" in c or "tscore" in c for c in classes)


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in ((NEW[0], lambda: step_rows(lib, None, 4, 2)), (NEW[1], lambda: loss_hook(lib, None, 2))):
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and b"null handle" in msg, (name, msg)


@pytest.mark.parametrize("K,n", [(4, 0), (4, -1), (4, 5), (0, 1), (-2, 1)])
def test_a_row_count_outside_the_batch_is_refused_with_a_message(lib, K, n):
    assert step_rows(lib, None, K, n) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_imitation_step_rows:" in msg and f"n = {n} ".encode() in msg and f"K = {K} ".encode() in msg and b"null handle" not in msg, msg


def test_the_edges_of_the_row_range_pass_and_the_hook_refuses_no_rows(lib):
    for K, n in ((1, 1), (4, 4), (4, 1)):
        assert step_rows(lib, None, K, n) == -1 and b"null handle" in lib.gnnb_last_error(), (K, n)
    for n in (0, -3):
        assert loss_hook(lib, None, n) == -1
        msg = lib.gnnb_last_error()
        assert b"gnnb_imitation_loss:" in msg and f"n = {n} ".encode() in msg and b"null handle" not in msg, msg


@pytest.mark.parametrize("margin", [-1.0, -1e-300, NAN, -math.inf])
def test_a_negative_or_nan_margin_is_refused_with_a_message(lib, margin):
    for name, call in ((NEW[0], lambda: step_rows(lib, None, 4, 2, margin)), (NEW[1], lambda: loss_hook(lib, None, 2, margin))):
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and b"margin" in msg and b"null handle" not in msg, (name, msg)
    for ok in (0.0, 1.0, 1e30):                               # these pass the check (and stop at the null handle)
        assert step_rows(lib, None, 4, 2, ok) == -1 and b"null handle" in lib.gnnb_last_error()
        assert loss_hook(lib, None, 2, ok) == -1 and b"null handle" in lib.gnnb_last_error()


# ---- the Python arguments ---------------------------------------------------------------------------------------------------------------
def test_the_new_keywords_stand_directly_in_front_of_strong_candidates():
    for f in (frontier.branch_and_bound_frontier, frontier.FrontierRun.__init__):
        names = list(inspect.signature(f).parameters)
        params = inspect.signature(f).parameters
        assert names[-6:] == ["imitate", "imitate_margin", "strong_candidates", "strong_chunk", "strong_audit", "branching"], f
        assert params["imitate"].default is None and params["imitate_margin"].default == 1.0 == frontier.IMITATE_MARGIN_DEFAULT
    jobs = inspect.signature(frontier.JobsRun.__init__).parameters
    assert not any(p.startswith("imitate") for p in jobs)    # the jobs of a pool share one handle: out of scope
    assert frontier._Round.imitate is None and frontier._Round.learning is False


BAD = [({"imitate": 0}, "imitate"), ({"imitate": -1}, "imitate"), ({"imitate": True}, "imitate"), ({"imitate": 2.0}, "imitate"), ({"imitate": "1"}, "imitate"),
       ({"imitate": 1, "imitate_margin": -0.5}, "imitate_margin"), ({"imitate": 1, "imitate_margin": NAN}, "imitate_margin"),
       ({"imitate": 1, "imitate_margin": True}, "imitate_margin"), ({"imitate": 1, "imitate_margin": "1"}, "imitate_margin"),
       ({"imitate": 1, "imitate_margin": None}, "imitate_margin"),
       ({"imitate_margin": 0.5}, "imitate_margin"), ({"imitate_margin": 0.5, "branching": "strong"}, "imitate_margin"),
       ({"imitate": 1, "branching": "babsr"}, "imitate"), ({"imitate": 1, "branching_threshold": 0.2}, "imitate"),
       ({"imitate": 1, "branching_threshold": 0.2, "online_threshold": 5}, "imitate"), ({"imitate": 1, "online_threshold": 5}, "imitate"),
       ({"imitate": 2, "branching": "strong", "branching_threshold": 0.2}, "imitate")]


@pytest.mark.parametrize("kw,name", BAD)
def test_bad_imitate_arguments_are_rejected_before_a_device_is_touched(kw, name):
    with pytest.raises(ValueError, match=name + r"\b"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], **kw)


@pytest.mark.parametrize("kw", [{"imitate": 1}, {"imitate": 3, "branching": "strong"}, {"imitate": 1, "imitate_margin": 0}, {"imitate": 1, "imitate_margin": 2.5},
                                {"imitate": 1, "strong_audit": []}, {"imitate": 2, "strong_candidates": 8, "strong_chunk": 64},
                                {"imitate": 1, "branching": "strong", "strong_candidates": 8, "strong_audit": []}])
def test_a_choice_that_is_no_online_graphchoice_is_a_type_error(kw):
    """The value checks pass and the type check of ``choice`` refuses the stand-in, still before a device is touched."""
    for choice in (NoDevice(), object()):
        with pytest.raises(TypeError, match="graph_score_online"):
            frontier.branch_and_bound_frontier(NoDevice(), choice, [], K=4, **kw)


def test_the_strong_options_alone_are_still_refused():
    with pytest.raises(ValueError, match="strong_candidates"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], strong_candidates=8)
    with pytest.raises(ValueError, match="strong_chunk"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], strong_chunk=64)


def test_the_engine_refuses_a_bad_margin_before_anything_else():
    from gnn_branching_amd.engine import ScorerEngine
    for bad in (-1.0, NAN, True, "1", None):
        with pytest.raises(ValueError, match="margin"):
            ScorerEngine._margin(bad, "imitation_step")
    assert ScorerEngine._margin(0, "x") == 0.0 and ScorerEngine._margin(np.float32(0.5), "x") == 0.5


# ---- the rule on hand-worked rows -------------------------------------------------------------------------------------------------------
def row(R=8):
    return np.zeros(R, F32), np.ones(R, F32), np.full(R, NAN)


def test_rule_two_violators_and_one_satisfied_candidate():
    s, m, tau = row()
    tau[[1, 3, 4, 6]] = [0.5, 0.9, 0.1, 0.25]                # teacher 3
    s[[1, 3, 4, 6]] = [0.0, 0.25, -1.0, 0.5]
    # terms at margin 1: q=1: -0.25 + 0.4 = 0.15 > 0; q=4: -1.25 + 0.8 < 0; q=6: 0.25 + 0.65 = 0.9 > 0
    loss, ds, rep, regret, status = rule(s, m, tau, 1.0)
    t1 = F32(F32(0.0) - F32(0.25)) + F32(1.0 * (0.9 - 0.5))
    t6 = F32(F32(0.5) - F32(0.25)) + F32(1.0 * (0.9 - 0.25))
    assert loss == F32(float(t1) + float(t6)) and abs(float(loss) - 1.05) < 1e-6
    assert ds.tolist() == [0, 1, 0, -2, 0, 0, 1, 0] and rep == [3, 6, 4, 2] and regret == 0.9 - 0.25 and status == 0
    loss0, ds0, rep0, _, _ = rule(s, m, tau, 0.0)            # margin 0: the plain ranking hinge, only q = 6 scores above the teacher
    assert loss0 == F32(0.25) and ds0.tolist() == [0, 0, 0, -1, 0, 0, 1, 0] and rep0 == [3, 6, 4, 1]


def test_rule_a_term_of_exactly_zero_is_no_violator_and_one_ulp_above_is():
    s, m, tau = row()
    tau[[2, 5]] = [1.0, 0.5]                                  # delta = 0.5 exactly
    s[[2, 5]] = [0.5, 0.0]                                    # term = -0.5 + 0.5 = 0
    loss, ds, rep, regret, status = rule(s, m, tau, 1.0)
    assert loss == 0 and not ds.any() and rep == [2, 2, 2, 0] and regret == 0.0 and status == 0
    s[5] = np.nextafter(F32(0.0), F32(1.0))                   # the smallest subnormal: -0.5 + it rounds to -0.5, still no violator
    assert rule(s, m, tau, 1.0)[2][3] == 0
    s[2] = np.nextafter(F32(0.5), F32(0.0))                   # s[t] one ulp below 0.5: term = one ulp of 0.5 (2^-25 below, so 2^-25)
    loss, ds, rep, _, _ = rule(s, m, tau, 1.0)
    assert rep[3] == 1 and float(loss) == 2.0 ** -25 and ds.tolist() == [0, 0, -1, 0, 0, 1, 0, 0]


def test_rule_equal_maxima_take_the_lower_index_and_a_tie_with_a_higher_score_violates():
    s, m, tau = row()
    tau[[1, 4, 6]] = [0.75, 0.75, 0.2]
    s[[1, 4, 6]] = [0.1, 0.3, -5.0]
    loss, ds, rep, regret, _ = rule(s, m, tau, 1.0)           # teacher 1; q = 4: delta 0, term 0.2 > 0
    assert rep == [1, 4, 3, 1] and loss == F32(F32(0.3) - F32(0.1)) and ds.tolist() == [0, -1, 0, 0, 1, 0, 0, 0] and regret == 0.0
    s[4] = 0.1                                                # the tie in s too: term 0, no violator; the pick is the lower index
    loss, ds, rep, _, _ = rule(s, m, tau, 1.0)
    assert rep == [1, 1, 3, 0] and loss == 0 and not ds.any()


def test_rule_one_candidate_none_and_the_refusals():
    s, m, tau = row()
    loss, ds, rep, regret, status = rule(s, m, tau, 1.0)
    assert math.isnan(loss) and not ds.any() and rep == [-1, -1, 0, 0] and math.isnan(regret) and status == 0
    tau[3] = 0.4
    loss, ds, rep, regret, status = rule(s, m, tau, 1.0)
    assert loss == 0 and not ds.any() and rep == [3, 3, 1, 0] and regret == 0.0 and status == 0
    for bad in ("decided", "+inf", "-inf"):
        s2, m2, tau2 = s.copy(), m.copy(), tau.copy()
        tau2[5] = {"decided": 0.2, "+inf": math.inf, "-inf": -math.inf}[bad]
        if bad == "decided":
            m2[5], s2[5] = 0.0, -np.inf
        loss, ds, rep, regret, status = rule(s2, m2, tau2, 1.0)
        assert math.isnan(loss) and not ds.any() and rep == [-1, -1, 0, 0] and math.isnan(regret) and status == 8, bad


def test_rule_rows_ors_the_status_and_keeps_the_rows_apart():
    s, m, tau = (np.stack([a, a]) for a in row())
    tau[0, [1, 2]] = [0.3, 0.6]
    tau[1, 4] = math.inf
    loss, ds, rep, regret, status = rule_rows(s, m, tau, 2.0)
    assert status == 8 and math.isnan(loss[1]) and loss[0] == F32(2.0 * (0.6 - 0.3)) and rep.tolist() == [[2, 1, 2, 1], [-1, -1, 0, 0]]
    assert ds[0].tolist() == [0, 1, -1, 0, 0, 0, 0, 0] and not ds[1].any()
