"""CPU: the replay buffer.  gnnb_replay_push, gnnb_replay_sample and gnnb_replay_bytes are declared, bound and
exported; the ABI stays 2 with ten options and the profile classes are the ones before; the entry points refuse every value outside its
range with a message that names them and the value, the null handle last; ``Replay`` rides on ``imitate`` and is checked before a device
is touched, and the four pinned parameter lists are what they were; the sampler's keys (csrc/gnnb_k_replay.h, compiled with g++ through
csrc/gnnb_replay_test.cpp) equal the numpy restatement of tests/replay_twin.py, whose draws are distinct, in range, a function of
(filled, n, seed, draw) alone and uniform; the push rule on hand-made tables.  (A handle needs a GPU: the rest is tests/test_gpu_replay.py.)"""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from gnn_branching_amd import _lib, frontier
from gnn_branching_amd.frontier import Replay, ReplayBuffer
from tests import replay_twin as twin
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_shortlist_cpu import CLASSES

NEW = ("gnnb_replay_push", "gnnb_replay_sample", "gnnb_replay_bytes")
NAN, INF = float("nan"), float("inf")
SAMPLE_CASES = [(1, 1), (2, 2), (5, 3), (5, 5), (300, 256), (65536, 256)]      # (filled, n)


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def push(lib, h, K, n, Cap):
    return lib.gnnb_replay_push(h, None, K, None, None, n, None, Cap, None, None, None, None)


def sample(lib, h, Cap, n):
    return lib.gnnb_replay_sample(h, None, Cap, n, 0, 0, None, None)


# ---- the library's surface --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2 and "GNNB_ABI_VERSION 2" in header.replace("  ", " ")
    assert "gnnb_k_replay.h" in _lib.SOURCES
    source = open(_lib.CSRC + "/gnnb_k_replay.h").read()
    for k in ("k_replay_rank", "k_replay_store", "k_replay_sample"):
        assert "void " + k + "(" in source, k
    assert "atomic" not in source.replace("No atomics", "")


def test_no_option_and_no_profile_class_was_added(lib):
    names = [lib.gnnb_option_name(i).decode() for i in range(lib.gnnb_option_count())]
    assert sorted(names) == sorted(_lib.OPTIONS) and len(names) == 10
    assert [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())] == CLASSES
    assert not any("replay" in c for c in CLASSES)


def test_one_list_of_step_tensors_serves_the_gather_the_store_and_the_size(lib):
    """The tensors a step reads are listed by ONE function (gnnb_step.h, with the step; gnnb.hip includes it); the gather (step_rows), the
    push and gnnb_replay_bytes (gnnb.hip) call it."""
    assert "gnnb_step.h" in _lib.SOURCES
    src = open(_lib.CSRC + "/gnnb_step.h").read() + open(_lib.CSRC + "/gnnb.hip").read()
    assert src.count("static std::vector<StepTensor> step_tensors(") == 1 and src.count(" : step_tensors(h, ") == 3
    body = src[src.index("static int step_rows("):src.index('extern "C" int gnnb_online_step_rows(')]
    assert "step_tensors(h, in->n_primal)" in body and "in->dual[" not in body and "in->primal[" not in body


@pytest.mark.parametrize("Cap", [0, -1, 65537, 1 << 30])
def test_a_capacity_outside_its_range_is_refused_with_a_message(lib, Cap):
    for name, call in ((NEW[0], lambda: push(lib, None, 4, 2, Cap)), (NEW[1], lambda: sample(lib, None, Cap, 2))):
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert (name + ":").encode() in msg and f"C = {Cap} ".encode() in msg and b"null handle" not in msg, (name, msg)
    assert lib.gnnb_replay_bytes(None, Cap) == 0


@pytest.mark.parametrize("K,n,Cap", [(4, 0, 8), (4, -1, 8), (4, 5, 8), (0, 1, 8), (-2, 1, 8), (8, 5, 4), (65536, 3, 2)])
def test_a_row_count_outside_the_batch_or_the_buffer_is_refused_with_a_message(lib, K, n, Cap):
    assert push(lib, None, K, n, Cap) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_replay_push:" in msg and f"n = {n} ".encode() in msg and f"K = {K} ".encode() in msg and f"C = {Cap} ".encode() in msg, msg
    assert b"null handle" not in msg


@pytest.mark.parametrize("n", [0, -1, 257, 1 << 20])
def test_a_draw_outside_its_range_is_refused_with_a_message(lib, n):
    assert sample(lib, None, 1024, n) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_replay_sample:" in msg and f"n = {n} ".encode() in msg and b"null handle" not in msg, msg


def test_the_edges_of_the_ranges_pass_and_the_null_handle_comes_last(lib):
    for K, n, Cap in ((1, 1, 1), (4, 4, 4), (4, 1, 65536), (65536, 65536, 65536)):
        assert push(lib, None, K, n, Cap) == -1 and b"gnnb_replay_push: null handle" in lib.gnnb_last_error(), (K, n, Cap)
    for Cap, n in ((1, 1), (1, 256), (65536, 256)):
        assert sample(lib, None, Cap, n) == -1 and b"gnnb_replay_sample: null handle" in lib.gnnb_last_error(), (Cap, n)
    assert lib.gnnb_replay_bytes(None, 4) == 0


# ---- the Python arguments ---------------------------------------------------------------------------------------------------------------
PINNED = {
    "branch_and_bound_frontier": ['lp', 'choice', 'layers', 'K', 'n_iter', 'lr', 'eps', 'max_rounds', 'decision_bound', 'capacity', 'log', 'trace',
                                  'branching_threshold', 'kwbd_threshold', 'sparsest_layer', 'decision_threshold', 'stats', 'online_threshold', 'witness',
                                  'pgd_steps', 'pgd_step', 'pgd_restarts', 'pgd_seed', 'repack', 'imitate', 'imitate_margin', 'strong_candidates',
                                  'strong_chunk', 'strong_audit', 'branching'],
    "FrontierRun": ['self', 'lp', 'choice', 'layers', 'K', 'n_iter', 'lr', 'eps', 'decision_bound', 'capacity', 'branching_threshold', 'kwbd_threshold',
                    'sparsest_layer', 'decision_threshold', 'online_threshold', 'max_rounds', 'witness', 'pgd_steps', 'pgd_step', 'pgd_restarts', 'pgd_seed',
                    'repack', 'imitate', 'imitate_margin', 'strong_candidates', 'strong_chunk', 'strong_audit', 'branching'],
    "StrongJobsRun": ['self', 'choice', 'fixed_layers', 'jobs', 'in_shape', 'K', 'segments', 'cap', 'n_iter', 'lr', 'eps', 'branching_threshold',
                      'kwbd_threshold', 'sparsest_layer', 'decision_threshold', 'witness', 'pgd_steps', 'pgd_step', 'pgd_restarts', 'pgd_seed', 'imitate',
                      'imitate_margin', 'strong_candidates', 'strong_chunk', 'strong_audit', 'branching'],
    "verify_properties_strong": ['choice', 'fixed_layers', 'jobs', 'K', 'segments', 'capacity', 'n_iter', 'lr', 'eps', 'max_rounds', 'log', 'trace', 'stats',
                                 'learned', 'imitate', 'imitate_margin', 'strong_candidates', 'strong_chunk', 'strong_audit', 'branching'],
}


def test_the_four_pinned_parameter_lists_are_unchanged():
    fns = {"branch_and_bound_frontier": frontier.branch_and_bound_frontier, "FrontierRun": frontier.FrontierRun.__init__,
           "StrongJobsRun": frontier.StrongJobsRun.__init__, "verify_properties_strong": frontier.verify_properties_strong}
    for name, f in fns.items():
        params = inspect.signature(f).parameters
        assert list(params) == PINNED[name], name
        assert params["imitate"].default is None
    assert frontier._Round.replay is None


def test_replay_keeps_what_it_is_given_and_has_the_issues_defaults():
    r = Replay(3)
    assert (r.every, r.buffer, r.capacity, r.batch, r.steps, r.seed) == (3, None, 1024, 8, 1, 0)
    assert list(inspect.signature(Replay.__init__).parameters) == ["self", "every", "buffer", "capacity", "batch", "steps", "seed"]
    for m in ("push", "read_state", "sample", "step", "evaluate", "split", "save", "load"):
        assert callable(getattr(ReplayBuffer, m)), m
    assert list(inspect.signature(ReplayBuffer.step).parameters)[:5] == ["self", "n", "margin", "seed", "draw"]
    assert list(inspect.signature(ReplayBuffer.push).parameters) == ["self", "batch", "K", "rows", "n", "table", "status"]


BAD = [Replay(0), Replay(-1), Replay(True), Replay(2.0), Replay("1"), Replay(None), Replay(1, capacity=0), Replay(1, capacity=2.5),
       Replay(1, capacity=True), Replay(1, capacity=65537), Replay(1, batch=0), Replay(1, batch=True), Replay(1, batch=1.0), Replay(1, batch=257),
       Replay(1, capacity=4, batch=5), Replay(1, steps=-1), Replay(1, steps=True), Replay(1, steps=1.5), Replay(1, steps=None), Replay(1, seed=-1),
       Replay(1, seed=2 ** 64), Replay(1, seed=0.5), Replay(1, buffer=object()), Replay(1, buffer=[]), Replay(1, buffer=8)]


@pytest.mark.parametrize("r", BAD, ids=[repr(r) for r in BAD])
@pytest.mark.parametrize("branching", ["gnn", "strong"])
def test_a_bad_replay_is_a_value_error_that_names_imitate_before_a_device_is_touched(r, branching):
    with pytest.raises(ValueError, match=r"imitate\b"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, imitate=r, branching=branching)
    with pytest.raises(ValueError, match=r"imitate\b"):
        frontier.StrongJobsRun(NoDevice(), [], [], (3, 8, 8), 4, 2, 64, 20, 0.1, 1e-4, imitate=r, branching=branching)


@pytest.mark.parametrize("kw", [{"branching": "babsr"}, {"branching_threshold": 0.2}, {"online_threshold": 5, "branching_threshold": 0.2}])
def test_a_replay_is_refused_where_an_integer_is(kw):
    for r in (Replay(1), Replay(1, steps=0)):
        with pytest.raises(ValueError, match=r"imitate\b"):
            frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], imitate=r, **kw)


@pytest.mark.parametrize("r", [Replay(1), Replay(2, capacity=16, batch=2, steps=2), Replay(1, capacity=256, batch=256, steps=3, seed=2 ** 64 - 1)])
def test_steps_with_a_choice_that_is_no_online_graphchoice_is_still_the_type_error(r):
    for choice in (NoDevice(), object()):
        with pytest.raises(TypeError, match="graph_score_online"):
            frontier.branch_and_bound_frontier(NoDevice(), choice, [], K=4, imitate=r)


def test_an_integer_imitate_is_checked_as_before():
    for bad in (0, -1, True, 2.0, "1"):
        with pytest.raises(ValueError, match=r"imitate\b"):
            frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], imitate=bad)
    with pytest.raises(TypeError, match="graph_score_online"):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, imitate=1)


def test_a_buffer_needs_a_capacity_in_range_and_a_bound_engine():
    class Unbound:
        sizes = None
    for bad in (0, -1, 65537, True, 2.5, "8", None):
        with pytest.raises(ValueError, match="capacity"):
            ReplayBuffer(NoDevice(), bad)
    with pytest.raises(ValueError, match="no network bound"):
        ReplayBuffer(Unbound(), 8)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("replay") / "libgnnb_replay_test.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(_lib.CSRC, "gnnb_replay_test.cpp")])
    lib = C.CDLL(so)
    lib.gnnb_rt_keys.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.gnnb_rt_sample.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    return lib


SEEDS = [(0, 0), (1, 0), (0, 1), (12345, 678), (2 ** 64 - 1, 2 ** 64 - 1), (0x9E3779B97F4A7C15, 2 ** 63)]


def test_the_headers_keys_equal_the_restatement(shim):
    assert shim.gnnb_rt_max_sample() == 256 == frontier.REPLAY_BATCH_MAX and shim.gnnb_rt_max_capacity() == 65536 == frontier.REPLAY_CAPACITY_MAX
    for seed, draw in SEEDS:
        for filled in (1, 5, 300):
            got = np.zeros(filled, np.uint64)
            shim.gnnb_rt_keys(filled, seed, draw, got.ctypes.data)
            assert got.tolist() == twin.keys(filled, seed, draw).tolist(), (seed, draw, filled)
            assert len(set(got.tolist())) == filled              # distinct: the order never needs its second component


@pytest.mark.parametrize("filled,n", SAMPLE_CASES)
def test_the_headers_draw_equals_the_restatement(shim, filled, n):
    for seed, draw in SEEDS[:4]:
        got = np.full(n, -7, np.int32)
        shim.gnnb_rt_sample(filled, n, seed, draw, got.ctypes.data)
        assert got.tolist() == twin.sample(filled, n, seed, draw), (seed, draw)


@pytest.mark.parametrize("filled,n", SAMPLE_CASES + [(0, 4), (3, 8)])
def test_a_draw_is_distinct_in_range_sorted_by_key_and_a_function_of_its_four_arguments(filled, n):
    idx = twin.sample(filled, n, 7, 3)
    m = min(n, filled)
    assert len(idx) == n and idx[m:] == [-1] * (n - m) and len(set(idx[:m])) == m and all(0 <= j < filled for j in idx[:m])
    k = twin.keys(filled, 7, 3)
    picked = [int(k[j]) for j in idx[:m]]
    assert picked == sorted(picked) and (m == filled or max(picked) < min(int(k[j]) for j in set(range(filled)) - set(idx[:m])))
    assert idx == twin.sample(filled, n, 7, 3)
    if filled >= 300:                                            # another seed or draw is another draw; a smaller n is a prefix
        assert idx != twin.sample(filled, n, 8, 3) and idx != twin.sample(filled, n, 7, 4)
        assert twin.sample(filled, n // 2, 7, 3) == idx[:n // 2]


def test_the_draws_are_uniform_over_the_slots():
    """4096 draws of 16 from 64: a slot is in a draw with probability 1/4, so its count is Binomial(4096, 1/4): mean 1024, standard
    deviation sqrt(4096 * 0.25 * 0.75) = 27.7.  Every count within 6 of them."""
    counts = np.zeros(64, np.int64)
    for draw in range(4096):
        counts[twin.sample(64, 16, 2024, draw)] += 1
    sd = (4096 * 0.25 * 0.75) ** 0.5
    print("slot counts: min", counts.min(), "max", counts.max(), "6 sd", 6 * sd)
    assert counts.sum() == 4096 * 16 and np.abs(counts - 1024).max() <= 6 * sd


# ---- the push rule ----------------------------------------------------------------------------------------------------------------------
def hand_table():
    """K = 6, R = 5: rows with 0, 1, 2 and all candidates, one at a decided node, one with tau = +inf."""
    tab = np.full((6, 5), NAN)
    mask = np.ones((6, 5), np.float32)
    tab[1, 2] = 0.5
    tab[2, [0, 4]] = [0.1, 0.2]
    tab[3] = [0.3, 0.1, 0.0, -0.2, 0.9]
    tab[4, [1, 3]] = [0.2, 0.4]
    mask[4, 3] = 0.0
    tab[5, [0, 1, 2]] = [0.1, INF, 0.3]
    return tab, mask


def test_the_rule_of_a_row():
    tab, mask = hand_table()
    assert [twin.row_class(list(tab[r]), list(mask[r])) for r in range(6)] == ["silent", "silent", "stored", "stored", "refused", "refused"]
    assert twin.row_class([NAN, -INF, 0.1], [1, 1, 1]) == "refused" and twin.row_class([0.0, 0.0], [1, 1]) == "stored"
    assert twin.row_class([0.5, NAN], [0, 1]) == "refused"       # one candidate, at a decided node: the refusal comes first


def test_the_ring_order_the_counts_and_the_status():
    tab, mask = hand_table()
    slots, state, status = twin.push(tab, mask, [0, 1, 2, 3], 6, 4, [0, 0, 0, 0])
    assert (slots, state, status) == ([-1, -1, 0, 1], [2, 2, 2, 2], 0)
    slots, state, status = twin.push(tab, mask, [3, 4, 2, 6, 3, -1], 6, 4, state)      # wraps: head 2 + 3 stored -> 1, full
    assert (slots, state, status) == ([2, -1, 3, -1, 0, -1], [1, 4, 3, 3], 8)
    slots, state, status = twin.push(tab, mask, [5], 6, 4, state)
    assert (slots, state, status) == ([-1], [1, 4, 0, 1], 8)
    slots, state, status = twin.push(tab, mask, [2], 6, 1, [0, 0, 0, 0])               # C = 1: every stored row lands in slot 0
    assert (slots, state) == ([0], [0, 1, 1, 0])


def test_the_python_ring_follows_both_rules():
    tab, mask = hand_table()
    ring = twin.Ring(4)
    assert ring.push(list("abcdef"), tab, mask) == 8 and ring.state == [2, 2, 2, 4]
    assert [s and s[0] for s in ring.slots] == ["c", "d", None, None]
    idx, pairs = ring.draw(2, 5, 0)
    assert sorted(idx) == [0, 1] and [p[0] for p in pairs] == ["cd"[j] for j in idx]
