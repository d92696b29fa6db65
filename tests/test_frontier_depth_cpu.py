"""CPU: the host side of ``split_depth`` -- ``frontier.round_depth`` over a grid against its restatement, with
the three boundaries; every refusal of ``frontier._check_split_depth`` by message, through the public function (the option travels on
the root's description, ``lp.split_depth``: the parameter lists of ``branch_and_bound_frontier`` and ``FrontierRun`` are pinned) before a
device is touched; the null-handle and range refusals of the two entry points; and the twins of tests/frontier_depth_twin.py checked against
hand-written examples, so that the GPU tests compare against something that has itself been checked."""
import ctypes as C
import inspect
import itertools
import types

import pytest
import torch

from gnn_branching_amd import _lib, frontier
from tests import frontier_depth_twin as T

INF = float("inf")
SIZES = [6, 4, 3, 1]                 # a toy network: graph layers 0..L+1, two ReLU layers, R = 7


class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"touched the scorer ({name}) before checking the arguments")


def root(split_depth):
    """Stands in for the LayerGraphLP: the option and nothing else -- a run that reads more of it went past the checks."""
    return types.SimpleNamespace(split_depth=split_depth)


# ---- round_depth ----------------------------------------------------------------------------------------------------------------------
def test_round_depth_over_a_grid_against_the_restatement():
    n = 0
    for K, D in itertools.product((1, 2, 3, 4, 16, 64), range(1, 9)):
        for k in sorted({1, 2, 3, K // 2, K - 1, K} - {0}):
            if k > K:
                continue
            for n_open, cap in itertools.product((k, k + 1, 2 * K, 5 * K), (2 * K + 1, 4 * K + 1, 1024)):
                if n_open > cap:
                    continue
                d = frontier.round_depth(k, K, D, n_open, cap)
                assert d == T.depth_of_round(k, K, D, n_open, cap), (k, K, D, n_open, cap)
                assert 0 <= d <= D
                if d:                                             # it fits, and the next depth does not (or is above D)
                    assert k << d <= 2 * K and n_open + ((1 << d) - 1) * k <= cap
                    assert d == D or k << (d + 1) > 2 * K or n_open + ((1 << (d + 1)) - 1) * k > cap
                else:
                    assert n_open + k > cap or 2 * k > 2 * K
                n += 1
    assert n > 1000


def test_round_depth_boundaries():
    # exactly 2K child rows: k 2^d = 2K fits, one parent more does not
    assert frontier.round_depth(2, 8, 8, 2, 1024) == 3 and 2 << 3 == 16
    assert frontier.round_depth(3, 8, 8, 3, 1024) == 2                      # 3 * 8 = 24 > 16
    assert frontier.round_depth(1, 64, 8, 1, 1024) == 7 and frontier.round_depth(1, 128, 8, 1, 1024) == 8
    # exactly cap: n_open + (2^d - 1) k = cap fits, one slot fewer drops a depth
    assert frontier.round_depth(2, 8, 8, 10, 10 + 7 * 2) == 3
    assert frontier.round_depth(2, 8, 8, 10, 10 + 7 * 2 - 1) == 2
    # nothing fits: not even one more slot per parent -> the "capacity" stop
    assert frontier.round_depth(2, 8, 8, 10, 11) == 0 and frontier.round_depth(2, 8, 8, 10, 12) == 1
    # a full round is depth 1 whatever D and the room
    for K, D in itertools.product((1, 2, 5, 16, 64), range(1, 9)):
        assert frontier.round_depth(K, K, D, K, 1 << 20) == 1


def test_one_job_round_depth():
    S = _lib
    st = [1.0, INF, -1.0, 10.0, 14.0, 0.0, 0.0, 0.0, 0.0]         # 10 open domains in 14 slots
    assert frontier._one_job_round_depth(st, 8, 3, 100, 1e-4, None, 0, 5) == (None, 8, False, 1)
    st[S.FS_N_OPEN] = 2.0
    assert frontier._one_job_round_depth(st, 8, 8, 100, 1e-4, None, 0, 5) == (None, 2, False, 3)
    assert frontier._one_job_round_depth(st, 8, 8, 27, 1e-4, None, 0, 5) == (None, 2, True, 3)      # 14 + 14 > 27: compact, then 2 + 14 <= 27
    assert frontier._one_job_round_depth(st, 8, 8, 15, 1e-4, None, 0, 5) == (None, 2, True, 2)      # 2 + 14 > 15: depth 2, 14 + 6 > 15
    assert frontier._one_job_round_depth(st, 8, 8, 3, 1e-4, None, 0, 5) == ("capacity", 0, False, 0)
    assert frontier._one_job_round_depth(st, 8, 8, 100, 1e-4, None, 5, 5)[0] == "max_rounds"
    assert frontier._one_job_round_depth(st, 8, 8, 100, 1e-4, -2.0, 0, 5)[0] == "decision"
    # D = 1 is today's round on every record
    for n_open, in_use, cap in itertools.product((1, 3, 8, 20), (20, 30), (21, 24, 28, 40)):
        st[S.FS_N_OPEN], st[S.FS_IN_USE] = float(n_open), float(in_use)
        assert frontier._one_job_round_depth(st, 8, 1, cap, 1e-4, None, 0, 5)[:3] == frontier._one_job_round(st, 8, cap, 1e-4, None, 0, 5)


# ---- the option ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 9, -1, 2.0, "2", True, False])
def test_a_bad_split_depth_is_refused(value):
    with pytest.raises(ValueError, match=r"split_depth = .*1\.\.8"):
        frontier._check_split_depth(value)
    with pytest.raises(ValueError, match="split_depth"):
        frontier.branch_and_bound_frontier(root(value), NoDevice(), [], K=4)
    from gnn_branching_amd import lp_producer
    with pytest.raises(ValueError, match="split_depth"):          # the root's description refuses it first
        lp_producer.LayerGraphLP([], None, None, split_depth=value)


def test_good_values_pass():
    for d in [None] + list(range(1, 9)):
        frontier._check_split_depth(d)
    frontier._check_split_depth(None, branching="babsr", branching_threshold=0.2, imitate=1)     # off: nothing to refuse
    frontier._check_split_depth(2, strong_candidates=None)


REFUSED = [({"branching": "babsr"}, r"split_depth with branching='babsr'"),
           ({"branching": "strong"}, r"split_depth with branching='strong'"),
           ({"branching_threshold": 0.2}, "split_depth takes no branching_threshold"),
           ({"branching_threshold": 0.2, "online_threshold": 5}, "split_depth takes no branching_threshold"),
           ({"online_threshold": 5}, "split_depth takes no online_threshold"),
           ({"imitate": 1}, "split_depth takes no imitate"),
           ({"imitate": frontier.Replay(every=1)}, "split_depth takes no imitate"),
           ({"strong_audit": []}, "split_depth takes no strong_audit"),
           ({"strong_candidates": frontier.Shortlist(gnn=2)}, "split_depth takes no Shortlist"),
           ({"strong_candidates": frontier.Shortlist(babsr=4, gnn=2)}, "split_depth takes no Shortlist")]


@pytest.mark.parametrize("kw,message", REFUSED)
def test_every_refused_combination_names_split_depth(kw, message):
    with pytest.raises(ValueError, match=message):
        frontier._check_split_depth(2, **kw)


@pytest.mark.parametrize("kw,message", [r for r in REFUSED if set(r[0]) <= {"branching", "branching_threshold", "strong_audit"}])
def test_the_public_function_refuses_before_a_device_is_touched(kw, message):
    """The run reads the root's option behind its own options' checks (a root is not touched before them), so this covers the
    combinations those checks pass with a stand-in scorer: an online run, imitate and a Shortlist need a real one to get that far."""
    with pytest.raises(ValueError, match=message):
        frontier.branch_and_bound_frontier(root(2), NoDevice(), [], K=4, **kw)
    with pytest.raises(ValueError, match=message):
        frontier.FrontierRun(root(2), NoDevice(), [], K=4, **kw)


def test_a_root_without_the_option_is_a_run_without_it():
    """``None`` and a root that has never heard of the option pass the check and reach the next thing the constructor reads."""
    for lp in (root(None), types.SimpleNamespace()):
        with pytest.raises(IndexError):                           # layers[-1] of no layers: past every option check
            frontier.FrontierRun(lp, NoDevice(), [], K=4)
    assert frontier._Round.split_depth is None and frontier._Round.depth == 0
    assert inspect.signature(frontier.FrontierRun.launch_round).parameters["depth"].default == 0


def test_the_many_job_functions_do_not_take_the_option():
    for f in (frontier.verify_properties, frontier.verify_properties_threshold, frontier.verify_properties_babsr, frontier.verify_properties_strong,
              frontier.verify_properties_online, frontier.FrontierJobs.__init__, frontier.FrontierJob.__init__):
        assert "split_depth" not in inspect.signature(f).parameters, f.__name__


# ---- the entry points, as far as they go without a handle ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_the_entry_points_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in ("gnnb_frontier_expand_depth", "gnnb_frontier_commit_depth", "gnnb_frontier_commit_depth_workspace_bytes"):
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2


@pytest.mark.parametrize("K,depth", [(2, 1), (0, 1), (2, 0), (2, 9), (32767, 2)])
def test_refusals_without_a_handle_carry_the_entry_point_s_name(lib, K, depth):
    pool, ch = _lib.Pool(), _lib.Children()
    calls = {"gnnb_frontier_expand_depth": lambda: lib.gnnb_frontier_expand_depth(None, C.byref(pool), None, K, depth, None, None, None, None, None, None,
                                                                                  None, None, None, None),
             "gnnb_frontier_commit_depth": lambda: lib.gnnb_frontier_commit_depth(None, C.byref(pool), None, K, depth, C.byref(ch), 1e-4, float("nan"), None,
                                                                                  None, 0, None)}
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in lib.gnnb_last_error(), (name, lib.gnnb_last_error())
    assert lib.gnnb_frontier_commit_depth_workspace_bytes(None, K, depth) == 0


# ---- the twins against hand-written examples ---------------------------------------------------------------------------------------------
def toy_pool(cap, seed):
    g = torch.Generator().manual_seed(seed)
    R = sum(SIZES[1:-1])
    return {"mask": torch.full((cap, R), -1, dtype=torch.int8), "lb": [torch.randn(cap, s, generator=g, dtype=torch.float64) for s in SIZES[1:]],
            "ub": [torch.randn(cap, s, generator=g, dtype=torch.float64) for s in SIZES[1:]], "alpha": torch.randn(cap, R, generator=g, dtype=torch.float64),
            "beta": torch.randn(cap, R, generator=g, dtype=torch.float64), "bound": torch.randn(cap, generator=g, dtype=torch.float64),
            "open": torch.ones(cap, dtype=torch.int32)}


def rows(n):
    R = sum(SIZES[1:-1])
    return {"mask": torch.full((n, R), 77, dtype=torch.int8), "plb": [torch.full((n, s), float("nan"), dtype=torch.float64) for s in SIZES[1:]],
            "pub": [torch.full((n, s), float("nan"), dtype=torch.float64) for s in SIZES[1:]], "alpha": torch.full((n, R), float("nan"), dtype=torch.float64),
            "beta": torch.full((n, R), float("nan"), dtype=torch.float64), "split": torch.full((n,), 77, dtype=torch.int32),
            "live": torch.full((n,), 77, dtype=torch.int32)}


@pytest.mark.parametrize("m", [1, 2, 3])
def test_a_parent_s_live_masks_enumerate_every_assignment_of_its_nodes(m):
    """depth 3, one parent with m listed nodes: 2^m live rows, pairwise distinct, every assignment of the m nodes once, nothing else
    touched; the other 8 - 2^m rows dead with the parent's mask."""
    pool, out = toy_pool(3, 1), rows(8)
    pool["mask"][2, 0] = 1                                        # a decided node of the parent stays as it is
    nodes = [[0, 1], [0, 3], [1, 2]][:m]                          # flat 1, 3, 6: ascending
    flat = [1, 3, 6][:m]
    T.expand(pool, [2], 3, [0, m], nodes, SIZES, out)
    live = out["live"].tolist()
    assert live == [1] * 2 ** m + [0] * (8 - 2 ** m)
    seen = set()
    for j in range(8):
        row = out["mask"][j]
        others = [r for r in range(7) if r not in flat]
        assert torch.equal(row[others], pool["mask"][2][others])
        assert torch.equal(out["alpha"][j], pool["alpha"][2]) and torch.equal(out["plb"][1][j], pool["lb"][1][2])
        if live[j]:
            bits = tuple(int(row[r]) for r in flat)
            assert all(b in (0, 1) for b in bits) and bits == tuple((j >> b) & 1 for b in range(m))
            seen.add(bits)
            assert int(out["split"][j]) == 0
        else:
            assert torch.equal(row, pool["mask"][2]) and int(out["split"][j]) == len(SIZES) - 3
    assert seen == set(itertools.product((0, 1), repeat=m))


def test_expand_twin_dead_parents_and_split_layer():
    """K = 5 at depth 2: no nodes, more nodes than the depth, a slot outside the pool, a node that is none, one node in the last layer."""
    pool, out = toy_pool(4, 2), rows(21)
    cand0 = [0, 0, 3, 4, 5, 6]
    cand_dec = [[0, 0], [0, 1], [1, 0], [0, 2], [1, 3], [1, 1]]   # [1, 3]: layer 1 has 3 nodes
    T.expand(pool, [0, 1, 9, 2, 3], 2, cand0, cand_dec, SIZES, out)
    assert out["live"].tolist() == [0] * 16 + [1, 1, 0, 0] + [77]
    assert out["split"].tolist() == [1] * 8 + [-1] * 4 + [1] * 4 + [1, 1, 1, 1] + [77]
    assert bool((out["mask"][8:12] == 77).all()) and bool(torch.isnan(out["alpha"][8:12]).all())      # the slot outside: nothing written
    for c, s in [(0, 0), (3, 0), (4, 1), (7, 1), (12, 2), (15, 2), (18, 3), (19, 3)]:
        assert torch.equal(out["mask"][c], pool["mask"][s]), c
    assert int(out["mask"][16, 5]) == 0 and int(out["mask"][17, 5]) == 1 and bool((out["mask"][20] == 77).all())


def test_top_nodes_order():
    scores = torch.tensor([0.5, 0.9, -0.0, 0.9, 0.0, float("nan"), 0.2])
    und = torch.tensor([1, 1, 1, 1, 1, 0, 0], dtype=torch.bool)
    assert T.top_nodes(scores, und, 1, SIZES) == [[0, 1]]                        # equal scores: the lowest index
    assert T.top_nodes(scores, und, 3, SIZES) == [[0, 0], [0, 1], [0, 3]]        # emitted in ascending flat index
    assert T.top_nodes(scores, und, 4, SIZES) == [[0, 0], [0, 1], [0, 2], [0, 3]]      # -0.0 == 0.0: flat 2 before flat 4
    assert T.top_nodes(scores, und, 8, SIZES) == [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0]]
    und[5] = True
    assert T.top_nodes(scores, und, 2, SIZES) == []                              # a NaN at an undecided node


def two_children_example():
    """K = 2 parents in slots [3, 1] of a pool of 6 with 4 slots in use, slot 0 open besides; children: 0 kept, 1 kept, 2 kept, 3 closed
    by its bound.  global_ub becomes 0.5."""
    pool = toy_pool(6, 3)
    pool["open"] = torch.tensor([1, 1, 0, 1, 0, 0], dtype=torch.int32)
    pool["bound"][0] = -0.25
    R = sum(SIZES[1:-1])
    g = torch.Generator().manual_seed(4)
    ch = {"mask": torch.full((4, R), -1, dtype=torch.int8), "lb": [-torch.rand(4, s, generator=g, dtype=torch.float64) - 0.1 for s in SIZES[1:]],
          "ub": [torch.rand(4, s, generator=g, dtype=torch.float64) + 0.1 for s in SIZES[1:]], "infeasible": torch.zeros(4, dtype=torch.int32),
          "live": torch.ones(4, dtype=torch.int32), "bound": torch.tensor([-1.0, -2.0, -3.0, 0.75], dtype=torch.float64),
          "ub_value": torch.tensor([0.9, 0.5, 0.8, 0.95], dtype=torch.float64), "alpha": torch.rand(4, R, generator=g, dtype=torch.float64),
          "beta": torch.rand(4, R, generator=g, dtype=torch.float64)}
    ch["lb"][0][1, 2] = 0.5                                       # child 1: node 2 resolves to passing
    return pool, ch


def test_commit_twin_at_two_children_reproduces_a_hand_written_example():
    pool, ch = two_children_example()
    state = [1.0, INF, INF, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]
    got = T.commit(pool, state, [3, 1], 2, ch, 1e-4, None, SIZES)
    # ranks 0, 1 take the parents' slots in the order of `slots`; rank 2 >= K lands above in_use, in slot 4
    assert got == [0.5, 0.75, -3.0, 4.0, 5.0, 3.0, 1.0, 0.0, 0.0]
    assert pool["open"].tolist() == [1, 1, 0, 1, 1, 0]
    assert [float(pool["bound"][s]) for s in (3, 1, 4)] == [-1.0, -2.0, -3.0]
    assert int(pool["mask"][1, 2]) == 1 and bool((pool["mask"][3] == -1).all())
    assert torch.equal(pool["alpha"][4], ch["alpha"][2]) and torch.equal(pool["lb"][1][1], ch["lb"][1][1])


def test_commit_twin_drops_a_child_that_finds_no_slot_and_closes_a_parent_without_children():
    pool, ch = two_children_example()
    small = {k: ([t[:5] for t in v] if isinstance(v, list) else v[:5]) for k, v in pool.items()}      # a pool of 5: slot 4 is the last
    ch["bound"][3] = -4.0                                         # all four kept: ranks 2, 3 -> slots 4 and 5, and 5 is not there
    got = T.commit(small, [1.0, INF, INF, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0], [3, 1], 2, ch, 1e-4, None, SIZES)
    assert got == [0.5, -4.0, -3.0, 4.0, 5.0, 3.0, 1.0, 0.0, 1.0]
    pool, ch = two_children_example()
    ch["live"][2] = ch["live"][3] = 0                             # parent 1 (slot 1) has no live child: closed at its own bound
    want_closed = float(pool["bound"][1])
    got = T.commit(pool, [1.0, INF, INF, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0], [3, 1], 2, ch, 1e-4, None, SIZES)
    assert got[T.FS_CLOSED_LB] == want_closed and got[T.FS_KEPT] == 2.0 and got[T.FS_CLOSED] == 1.0 and got[T.FS_N_OPEN] == 3.0 and got[T.FS_IN_USE] == 4.0


def test_commit_twin_with_four_children_per_parent():
    """C = 4, K = 1: parent in slot 2, in_use 3; children kept, dead, kept, kept -> ranks 0, 1, 2 -> slots 2, 3, 4."""
    pool, ch = two_children_example()
    ch["live"][1] = 0
    got = T.commit(pool, [1.0, INF, INF, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0], [2], 4, ch, 1e-4, 0.8, SIZES)
    assert got[T.FS_GLOBAL_UB] == 0.8 and got[T.FS_KEPT] == 3.0 and got[T.FS_IN_USE] == 5.0 and got[T.FS_N_OPEN] == 5.0
    assert [float(pool["bound"][s]) for s in (2, 3, 4)] == [-1.0, -3.0, 0.75]
