"""Shortlisting the strong-branching candidates by the GNN's scores as well, on the MI355X (DESIGN.md section 7.14;
gnn_branching_amd/frontier.py ``Shortlist``; csrc/gnnb_k_strong.h k_strong_union_count, k_strong_union_compact).  Every comparison is
exact -- integers, Python floats of the same fp64 values, fp32 bits for losses and parameters -- but global_ub, within 1e-9 max(1, |ub|),
as in the files these tests stand beside.

1. gnnb_strong_list_union against its restatement (tests/frontier_shortlist_twin.py) on crafted rows of kwg_rect;
2. ``Shortlist(babsr=M)`` is the run ``strong_candidates=M``;
3. a "strong" run over the scorer's shortlist, and over the union, against the host loop;
4. an audited "gnn" run is the run, its sources are the twin's and the committed decision is always a candidate;
5. a "gnn" run that learns: the report's pick is the committed decision, and the run equals the host loop of
   tests/test_gpu_imitation.py fed the audit's tables;
6. what crosses the link; 7. who launches what; 8. many jobs; 9. the limits that need a handle."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib
from gnn_branching_amd.frontier import DomainPool, FrontierJob, FrontierRun, Shortlist, branch_and_bound_frontier, verify_properties_strong
from tests.frontier_shortlist_twin import shortlist_twin, union_reference
from tests.frontier_strong_twin import NAN, list_reference, node_of, offsets, same
from tests.frontier_twin import EPS_BAB, LR, N_ITER, bind, engine, masked, toy   # noqa: F401  (engine: the module's fixture)
from tests.test_gpu_frontier_babsr import FORWARD_CLASSES

pytestmark = pytest.mark.gpu

I32, F64, F32 = torch.int32, torch.float64, torch.float32
S = _lib
NET = "kwg_rect"                    # R = 2904: ReLU layers of 1920, 960 and 24 nodes
INF = float("inf")
CAP = 9                             # the crafted pool's slots
PROP, EPS_SMALL = (2, 6), 0.005
KINDS = ["same", "tie", "zeros", "inf", "nan_decided", "nan_a", "nan_b", "no_open", "bad_slot", "disjoint"]
SLOT = {kind: (CAP if kind == "bad_slot" else i % CAP) for i, kind in enumerate(KINDS)}
TIE = [1790, 1791, 1792, 1793, 1919, 1920]      # A's tie of six: across the tile boundary 1791 | 1792 and the layer boundary 1919 | 1920


def quiet(s):
    pass


def close_ub(a, b):
    return a == b or abs(a - b) <= 1e-9 * max(1.0, abs(b))


# ---- 1. the list ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(engine):
    """One row per kind of KINDS on one pattern of undecided nodes (so the rows share ``count``), as CPU tensors amb / A / B (10, R)."""
    relu = bind(engine, NET)
    off, R, K = offsets(relu), sum(relu), len(KINDS)
    assert relu[0] == 1920 and TIE[1] % 256 == 255 and TIE[2] % 256 == 0 and TIE[4] == off[1] - 1 and TIE[5] == off[1]
    g = torch.Generator().manual_seed(23)
    pattern = (torch.rand(R, generator=g) < 0.5).float()
    pattern[TIE] = 1.0
    pattern[[0, R - 1]] = 1.0
    pattern[[1, R - 2]] = 0.0
    amb = pattern.repeat(K, 1)
    A = torch.rand(K, R, generator=g) * 0.1 + 0.01
    B = torch.rand(K, R, generator=g) * 0.1 + 0.01          # independent of A: two top lists overlap in part
    open_ = [r for r in range(R) if pattern[r] != 0]
    rest = [r for r in open_ if r not in TIE]
    for i, kind in enumerate(KINDS):
        if kind == "same":
            B[i] = A[i]
        elif kind == "tie":
            # A: 253 scores above the tie of six, so that 255, 256, 257 take 2, 3, 4 of it (258: across the layer boundary).  B: ties on
            # other nodes (ten at 0.8, a tie of four at 0.6 that a count of 14 cuts after two); B ranks TIE[0] first -- a node both take
            # -- and TIE[3] second: inside A's tie run but past A's rank for 255 and 256
            A[i, rest[5::5][:253]] = 0.9
            A[i, TIE] = 0.5
            B[i, rest[2::5][:10]] = 0.8
            B[i, rest[3::5][100:104]] = 0.6
            B[i, TIE[0]], B[i, TIE[3]] = 0.96, 0.95
        elif kind == "zeros":                              # the maxima of both: 300 zeros of both signs, on sets that overlap in part
            A[i], B[i] = -A[i], -B[i]
            za, zb = open_[3::4][:300], open_[1::3][:300]
            A[i, za[0::2]], A[i, za[1::2]] = -0.0, 0.0
            B[i, zb[0::2]], B[i, zb[1::2]] = 0.0, -0.0
        elif kind == "inf":
            A[i, rest[7::9][:20]], A[i, rest[2::9][:20]] = INF, -INF
            B[i, rest[7::9][10:30]], B[i, rest[4::9][:20]] = INF, -INF
        elif kind == "nan_decided":
            A[i, [1, R - 2]] = NAN
            B[i, 1] = NAN
        elif kind == "nan_a":
            A[i, open_[len(open_) // 2]] = NAN
        elif kind == "nan_b":
            B[i, open_[len(open_) // 3]] = NAN
        elif kind == "no_open":
            amb[i] = 0.0
        elif kind == "disjoint":                           # A's best 300 and B's best 300 share no node
            A[i, open_[0::4][:300]] += 0.5
            B[i, open_[1::4][:300]] += 0.5
    assert len(rest[5::5]) >= 253 and len(open_[1::3]) >= 300 and len(open_[1::4]) >= 300
    return relu, amb, A, B, len(open_)


def union_on_device(engine, pool, crafted, idx, top_a, top_b, pad=1, b_is_a=False):
    """gnnb_strong_list_union on the rows ``idx``; ``pad`` rows and list entries more in every array, poisoned, which must stay as they
    were.  Returns (cand0, cand_row, cand_slot, cand_dec, cand_src) as lists."""
    relu, amb, A, B, _ = crafted
    dev, K, R = engine.device, len(idx), sum(relu)
    cap = K * min(R, top_a + top_b)
    rows = lambda t: torch.cat([t[idx], torch.full((pad, R), 3.0)]).contiguous().to(dev)      # noqa: E731
    cand0 = torch.full((K + 1 + pad,), -7, dtype=I32, device=dev)
    lists = [torch.full(s, -7, dtype=I32, device=dev) for s in ((cap + pad,), (cap + pad,), (cap + pad, 2), (cap + pad,))]
    slots = torch.tensor([SLOT[KINDS[i]] for i in idx], dtype=I32).to(dev)
    engine.strong_list_union(pool, slots, rows(amb), rows(A), top_a, rows(A if b_is_a else B), top_b, cand0, *lists)
    cand0, row, slot, dec, src = (t.cpu().tolist() for t in (cand0, *lists))
    n = cand0[K]
    assert 0 <= n <= cap and cand0[K + 1:] == [-7] * pad
    assert row[n:] == slot[n:] == src[n:] == [-7] * (cap + pad - n) and dec[n:] == [[-7, -7]] * (cap + pad - n)
    return cand0[:K + 1], row[:n], slot[:n], dec[:n], src[:n]


def reference(crafted, idx, top_a, top_b, b_is_a=False):
    relu, amb, A, B, _ = crafted
    return union_reference(relu, amb[idx], A[idx], top_a, (A if b_is_a else B)[idx], top_b, [SLOT[KINDS[i]] for i in idx], CAP)


GROUPS = [[i] for i in range(len(KINDS))] + [[1, 8, 7, 5, 0], [9, 6, 2, 8, 3]]      # K = 1; K = 5 with a padding row, and with nothing undecided


@pytest.mark.parametrize("which", ["1", "255", "256", "257", "count-1", "count", "count+5"])
def test_the_union_against_its_restatement(which, crafted, engine):
    """Every kind of row alone and two groups of five, with each count in turn as top_a against a few top_b and as top_b against them."""
    count = crafted[4]
    top = eval(which, {"count": count})
    pool = DomainPool(engine, CAP)
    for top_a, top_b in [(top, 1), (top, 14), (top, 257), (top, count + 5), (1, top), (258, top), (count - 1, top)]:
        for idx in GROUPS:
            want, got = reference(crafted, idx, top_a, top_b), union_on_device(engine, pool, crafted, idx, top_a, top_b)
            assert got[0] == want[0], (top_a, top_b, idx, got[0], want[0])
            assert got[1:] == want[1:], (top_a, top_b, idx)
            counts = [b - a for a, b in zip(want[0], want[0][1:])]
            for i, c in zip(idx, counts):                   # the reference's own outcome, per kind
                kind = KINDS[i]
                if kind in ("no_open", "bad_slot", "nan_a", "nan_b"):
                    assert c == 0, (kind, c)
                else:
                    assert max(min(top_a, count), min(top_b, count)) <= c <= min(count, top_a + top_b), (kind, c)
                if kind == "same":
                    assert c == min(count, max(top_a, top_b))      # full overlap: the larger list
                if kind == "disjoint" and max(top_a, top_b) <= 300:
                    assert c == top_a + top_b               # no node in both
                if top_a + top_b >= 2 * count and kind not in ("no_open", "bad_slot", "nan_a", "nan_b"):
                    assert c == count                       # more asked for than there are


def test_the_crafted_ties_are_cut_where_they_were_built_to_be(crafted):
    """The host rule alone, on the "tie" row: A's counts 255..258 take 2..5 nodes of its tie in index order -- over the tile boundary,
    then over the layer boundary --; B takes TIE[0], which A takes too, and TIE[3], which lies inside A's tie run past A's rank; B's own
    cut at 14 falls into its tie of four on other nodes; the zeros of both signs are taken in index order."""
    relu, amb, A, B, count = crafted
    i = KINDS.index("tie")
    tie = [node_of(relu, r) for r in TIE]
    assert tie[3][0] == 0 and tie[4] == [0, 1919] and tie[5] == [1, 0]
    for top_a, n_ties in ((255, 2), (256, 3), (257, 4), (258, 5)):
        cand0, _, _, dec, src = reference(crafted, [i], top_a, 14)
        in_tie = [(d, s) for d, s in zip(dec, src) if d in tie]
        taken_by_a = [d for d, s in in_tie if s & 1]
        assert taken_by_a == tie[:n_ties], top_a
        assert (tie[0], 3) in in_tie                        # a node both take
        assert ((tie[3], 2) in in_tie) == (n_ties < 4) and ((tie[3], 3) in in_tie) == (n_ties >= 4)      # past A's rank: B's alone
        b_only = list_reference(relu, amb[[i]], B[[i]], 14, [0], CAP)[3]
        fours = [node_of(relu, r) for r in range(sum(relu)) if B[i, r] == 0.6]
        assert len(fours) == 4 and [d for d in b_only if d in fours] == fours[:2] and not set(map(tuple, fours)) & set(map(tuple, tie))
    z = KINDS.index("zeros")
    _, _, _, dec, src = reference(crafted, [z], 255, 257)
    za = [r for r in range(sum(relu)) if amb[z, r] != 0 and A[z, r] == 0][:255]
    zb = [r for r in range(sum(relu)) if amb[z, r] != 0 and B[z, r] == 0][:257]
    assert dec == [node_of(relu, r) for r in sorted(set(za) | set(zb))] and {1, 2, 3} == set(src)
    assert {float(np.copysign(1.0, float(A[z, r]))) for r in za} == {1.0, -1.0}


@pytest.mark.parametrize("top_a,top_b", [(1, 1), (256, 255), (257, 257), ("count", 14), ("count+5", "count+5")])
def test_b_equal_to_a_is_the_list_of_a(top_a, top_b, crafted, engine):
    """B = A with top_b <= top_a: gnnb_strong_list(A, top_a) entry for entry, the first top_b of the order in both sets."""
    relu, amb, A, B, count = crafted
    top_a, top_b = (eval(str(t), {"count": count}) for t in (top_a, top_b))
    dev, R = engine.device, sum(relu)
    pool = DomainPool(engine, CAP)
    for idx in GROUPS:
        K = len(idx)
        got = union_on_device(engine, pool, crafted, idx, top_a, top_b, b_is_a=True)
        cap = K * min(R, top_a)
        cand0 = torch.zeros(K + 1, dtype=I32, device=dev)
        lists = [torch.zeros(s, dtype=I32, device=dev) for s in ((cap,), (cap,), (cap, 2))]
        slots = torch.tensor([SLOT[KINDS[i]] for i in idx], dtype=I32).to(dev)
        engine.strong_list(pool, slots, amb[idx].contiguous().to(dev), A[idx].contiguous().to(dev), top_a, cand0, *lists)
        cand0 = cand0.cpu().tolist()
        n = cand0[K]
        assert got[0] == cand0 and [got[1], got[2], got[3]] == [t[:n].cpu().tolist() for t in lists], idx
        assert set(got[4]) <= {1, 3}
        for a, b in zip(cand0, cand0[1:]):
            assert got[4][a:b].count(3) == min(top_b, b - a)


def test_a_row_gets_the_same_entries_wherever_it_stands(crafted, engine):
    """The same row at position 0 of one batch and at position 3 of another, and alone: the same candidates and sources."""
    pool = DomainPool(engine, CAP)
    for i in (KINDS.index("tie"), KINDS.index("zeros"), KINDS.index("disjoint")):
        others = [j for j in range(len(KINDS)) if j != i]
        out = []
        for idx, pos in (([i], 0), ([i] + others[:2], 0), (others[2:5] + [i] + others[5:6], 3), (others[:7] + [i], 7)):
            cand0, row, slot, dec, src = union_on_device(engine, pool, crafted, idx, 256, 257)
            a, b = cand0[pos], cand0[pos + 1]
            assert row[a:b] == [pos] * (b - a) and slot[a:b] == [SLOT[KINDS[i]]] * (b - a)
            out.append((dec[a:b], src[a:b]))
        assert all(o == out[0] for o in out) and len(out[0][0]) >= 257


# ---- 2. Shortlist(babsr=M) is strong_candidates=M -------------------------------------------------------------------------------------------
def profiled(choice_of=toy, rounds=2, K=3, **kw):
    """(result, trace, launch names in order, launch counts) of a run on toy_kw with the launches recorded (gnnb_profile_trace)."""
    lp, choice, _ = choice_of()
    eng = choice.model.engine()
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.profile_trace()
        trace = []
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=quiet, trace=trace, **kw)
        counts = eng.profile_read()
        names = [name for name, _ in eng.profile_trace(1 << 16)]
    finally:
        eng.profile_enable(False)
    return res, trace, names, counts


@pytest.mark.parametrize("kw", [{"branching": "strong"}, {"branching": "gnn", "audit": True}, {"branching": "babsr", "audit": True}])
def test_a_babsr_shortlist_is_the_run_with_an_integer(kw):
    """The same result, trace, audit and launch trace."""
    out = []
    for value in (8, Shortlist(babsr=8), Shortlist(8, None)):
        audit = [] if kw.get("audit") else None
        res, trace, names, _ = profiled(branching=kw["branching"], strong_candidates=value, strong_chunk=5, strong_audit=audit)
        out.append([list(res), trace, audit, names])
    assert same(out[0][:3], out[1][:3]) and same(out[0][:3], out[2][:3]) and out[0][3] == out[1][3] == out[2][3]
    assert len(out[0][3]) > 10 and out[0][3].count("k_strong_count") == out[0][3].count("k_strong_compact") == out[0][0][2] >= 1
    assert all("sources" not in a for a in out[1][2] or []) and all("strong_sources" not in t for t in out[1][1])


# ---- 3. "strong" over the scorer's shortlist and over the union, against the host loop ------------------------------------------------------
FORMS = {"gnn": Shortlist(gnn=4), "union": Shortlist(babsr=8, gnn=4)}
ROUNDS = 3


@lru_cache(None)
def twin_of(form, K, rounds, commit, small=False):
    s = FORMS[form]
    return shortlist_twin(K, rounds, babsr=s.babsr, gnn=s.gnn, commit=commit, **({"prop": PROP, "eps": EPS_SMALL} if small else {}))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("form", ["gnn", "union"])
def test_a_strong_run_over_a_shortlist_equals_the_host_loop(form, K):
    """Decisions, candidates, sources, improvements, parents' and children's bounds per round, and global_lb after every round (runs of
    1, 2 and 3 rounds: a run repeats itself), against ``shortlist_twin``."""
    twin = twin_of(form, K, ROUNDS, "strong")
    lp, choice, _ = toy()
    runs = []
    for r in range(1, ROUNDS + 1):
        trace, stats = [], {}
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=r, log=quiet, trace=trace, stats=stats,
                                        strong_candidates=FORMS[form], strong_chunk=5, branching="strong")
        runs.append((res, trace, stats))
    res, trace, stats = runs[-1]
    print("twin", twin, "frontier", res, stats)
    assert twin["branches"] >= 3 and len(trace) == len(twin["decisions"]) == ROUNDS
    assert [t["decisions"] for t in trace] == twin["decisions"] == twin["strong_decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]
    assert [t["parent_bounds"] for t in trace] == twin["parent_bounds"]
    assert [t["strong_candidates"] for t in trace] == twin["candidates"] and [t["strong_sources"] for t in trace] == twin["sources"]
    assert same([t["strong_improvement"] for t in trace], twin["improvements"])
    assert [run[0][0] for run in runs] == twin["global_lb"] and close_ub(res[1], twin["global_ub"])
    assert all(same(run[1], trace[:r + 1]) for r, run in enumerate(runs))
    assert stats["branches"] == twin["branches"] and stats["strong_bounded"] == 2 * sum(len(c) for t in trace for c in t["strong_candidates"])
    # the twin's own outcome: the lists are what the form says they are
    srcs = [s for t in twin["sources"] for row in t for s in row]
    counts = [len(row) for t in twin["candidates"] for row in t]
    assert (set(srcs) == {2} and all(c == 4 for c in counts)) if form == "gnn" else (set(srcs) <= {1, 2, 3} and all(8 <= c <= 12 for c in counts))
    for t in twin["sources"]:
        for row in t:
            assert form == "gnn" or (sum(1 for s in row if s & 1), sum(1 for s in row if s & 2)) == (8, 4)


# ---- 4. the audit of a "gnn" run --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["gnn", "union"])
def test_an_audited_gnn_run_is_the_run_and_labels_every_committed_decision(form):
    lp, choice, root_mask = toy(False, PROP, EPS_SMALL)
    relu = [int(m.numel()) for m in root_mask]
    out = []
    for audit in (None, []):
        trace, stats = [], {}
        extra = {} if audit is None else {"strong_audit": audit, "strong_candidates": FORMS[form], "strong_chunk": 7}
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=quiet, trace=trace, stats=stats,
                                        **extra)
        out.append((res, trace, {k: v for k, v in stats.items() if k != "strong_bounded"}))
    assert same(list(out[0]), list(out[1])) and len(out[0][1]) == 2       # results, trace (decisions, bounds) and stats
    twin = twin_of(form, 2, 2, "gnn", small=True)
    trace = out[1][1]
    assert [t["decisions"] for t in trace] == twin["decisions"] == twin["gnn_decisions"]
    rows = [(r, i) for r, t in enumerate(trace) for i in range(len(t["slots"]))]
    assert len(audit) == len(rows) >= 2
    off = offsets(relu)
    for a, (r, i) in zip(audit, rows):
        print(form, "round", r, "row", i, {k: a[k] for k in ("slot", "decision", "improvement", "strong_decision", "best_improvement", "candidates", "sources")})
        assert a["candidates"] == twin["candidates"][r][i] and a["sources"] == twin["sources"][r][i]
        assert same(a["improvements"], twin["improvements"][r][i]) and a["strong_decision"] == twin["strong_decisions"][r][i]
        assert a["decision"] == trace[r]["decisions"][i]
        flat = off[a["decision"][0]] + a["decision"][1]
        assert flat in a["candidates"]                      # the committed decision has a label
        q = a["candidates"].index(flat)
        assert a["sources"][q] & 2                          # ... because the scorer's own shortlist holds its arg-max
        assert a["improvements"][q] == a["improvement"]     # its children as candidates are the round's children
        assert a["best_improvement"] >= a["improvement"]


# ---- 5. a "gnn" run that learns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_a_learning_gnn_run_reports_the_decision_it_made_and_equals_the_host_loop(K):
    """``imitate=1`` with ``Shortlist(babsr=8, gnn=2)``: on every learn row the report's pick is the committed decision, so its regret is
    that of the split that was made; losses, reports, regrets, bounds and the final parameters are those of the host loop of
    tests/test_gpu_imitation.py (``ScorerEngine.imitation_step`` on the parents' own forward arguments) fed the audit's tables."""
    from gnn_branching_amd.engine import state_blob
    from tests.test_gpu_imitation import FR_MARGIN, FR_ROUNDS, bits, host_loop, same_or_nan
    lp, choice, root_mask = toy(online=True)
    off = offsets([int(m.numel()) for m in root_mask])
    trace, audit, stats = [], [], {}
    glb, gub, rounds, bounded, reason = branch_and_bound_frontier(
        lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=FR_ROUNDS, log=quiet, trace=trace, stats=stats,
        strong_candidates=Shortlist(babsr=8, gnn=2), strong_audit=audit, imitate=1, imitate_margin=FR_MARGIN["gnn"])
    rows, tables = iter(audit), []
    for t in trace:
        tables.append([next(rows) for _ in t["slots"]])
    host = host_loop(K, FR_ROUNDS, 1, "gnn", tables, FR_MARGIN["gnn"])
    print("host", {k: v for k, v in host.items() if not k.startswith("weights")}, "frontier", (glb, gub, rounds, bounded, reason), stats)
    assert len(trace) == len(host["decisions"]) >= 2 and any(v > 0 for l in host["loss"] for v in l), "no step of the host loop carried a gradient"
    assert [t["decisions"] for t in trace] == host["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == host["child_bounds"]
    for r, t in enumerate(trace):
        assert "imitation_loss" in t and host["loss"][r]
        assert t["global_lb"] == host["global_lb"][r] and close_ub(t["global_ub"], host["global_ub"][r])
        np.testing.assert_array_equal(bits(t["imitation_loss"]), bits(host["loss"][r]))
        assert t["imitation_report"] == host["report"][r] and same_or_nan(t["imitation_regret"], host["regret"][r])
        for i, (rep, dec, a) in enumerate(zip(t["imitation_report"], t["decisions"], tables[r])):
            flat = off[dec[0]] + dec[1]
            assert rep[1] == flat, (r, i, rep, dec)         # pick IS the committed decision
            assert flat in a["candidates"] and rep[2] <= len(a["candidates"]) <= 10
            assert rep[0] == off[a["strong_decision"][0]] + a["strong_decision"][1]      # the teacher: the table's decision
            want = a["best_improvement"] - a["improvements"][a["candidates"].index(flat)]      # the regret of the split that was made
            assert t["imitation_regret"][i] == want or (want != want and t["imitation_regret"][i] != t["imitation_regret"][i]), (r, i)
    assert glb == host["global_lb"][-1] and close_ub(gub, host["global_ub"][-1])
    assert stats["imitation_steps"] == host["steps"] == len(trace) and stats["imitation_rows"] == host["rows"]
    got_w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(got_w), bits(host["weights"]))
    assert (bits(host["weights"]) != bits(host["weights_start"])).any()
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(got_w))


# ---- 6. what crosses the link ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branching,value,imitate", [("strong", Shortlist(gnn=4), None), ("strong", Shortlist(8, 4), None), ("gnn", Shortlist(8, 2), 1),
                                                     ("strong", Shortlist(8, 2), 1), ("strong", Shortlist(gnn=3), 1)])
def test_a_round_copies_nothing_but_the_candidate_count_and_the_state_record(branching, value, imitate):
    """One round under torch.cuda.set_sync_debug_mode("error"): the read of cand0[K] and the read of the state record are the two
    exemptions a strong round already has; the forward in front of the list, the union and a learning round's step add none."""
    from tests.test_gpu_frontier_online import sync_mode_is_live
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy(online=imitate is not None)
    extra = {} if imitate is None else {"imitate": imitate}
    run = FrontierRun(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, strong_candidates=value, strong_chunk=3, branching=branching, **extra)
    st = run.root()
    if not sync_mode_is_live(run):
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
    before = torch.cuda.get_sync_debug_mode()
    reads, read_candidates = [], run.read_candidates

    def exempt_read(n):
        with pytest.raises(RuntimeError):                  # the mode is live: the read is a synchronising copy
            read_candidates(n)
        torch.cuda.set_sync_debug_mode(before)             # the explicit exemption
        try:
            reads.append(read_candidates(n))
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return reads[-1]
    run.read_candidates = exempt_read
    try:
        torch.cuda.set_sync_debug_mode("error")
        run.launch_round(1, int(st[S.FS_IN_USE]))
        with pytest.raises(RuntimeError):
            run.read_state()                                # the state record: a synchronising copy
        torch.cuda.set_sync_debug_mode(before)
        st = run.pool.state.cpu().tolist()                  # ... exempted by hand
        if imitate is not None:
            assert run.imitate_pending and run.learning
            torch.cuda.set_sync_debug_mode("error")
            run._imitate()                                  # no read of its own
            torch.cuda.set_sync_debug_mode(before)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    M, G = value.babsr or 0, value.gnn
    assert len(reads) == 1 and max(M, G) <= reads[0] <= M + G and run.strong_bounded == 2 * reads[0]
    assert run.imitation_steps == (0 if imitate is None else 1)
    run.check_status()


# ---- 7. who launches what -------------------------------------------------------------------------------------------------------------------
def test_a_strong_run_without_a_gnn_count_launches_no_forward_kernel():
    res, _, names, counts = profiled(branching="strong", strong_candidates=Shortlist(babsr=4), strong_chunk=3)
    assert res[2] >= 1 and names.count("k_strong_count") == res[2]
    for k in FORWARD_CLASSES:
        assert k not in names and counts[k][1] == 0, k


def test_a_gnn_count_adds_the_forward_and_the_union_its_launches():
    """Per round: one gnnb_forward in front of the list in "strong" mode; the union launches three kernels under k_strong_count's class
    and one under k_strong_compact's, the scorer's list alone k_strong_count's one."""
    rounds = {}
    for form, per_round in (("gnn", 1), ("union", 3)):
        res, _, names, counts = profiled(branching="strong", strong_candidates=FORMS[form], strong_chunk=3)
        rounds[form] = res[2]
        assert res[2] >= 1 and names.count("k_frontier_gather") == res[2]
        assert names.count("k_strong_count") == per_round * res[2] and names.count("k_strong_compact") == names.count("k_strong_pick") == res[2]
        assert any(k in names for k in FORWARD_CLASSES)
        first = min(names.index(k) for k in FORWARD_CLASSES if k in names)
        assert names.index("k_frontier_gather") < first < names.index("k_strong_count")      # gather, forward, list
    # "gnn" mode scores its parents anyway: the union next to it adds no forward launch
    _, _, plain, _ = profiled(branching="gnn")
    _, _, audited, _ = profiled(branching="gnn", strong_candidates=FORMS["union"], strong_audit=[])
    for k in FORWARD_CLASSES:
        assert plain.count(k) == audited.count(k), k


def test_a_learning_strong_round_runs_its_scorer_ascent_once():
    """One round (scored by the opening parameters either way): a learning round of a run with a gnn count launches the k_dual_ascent
    class exactly as often as the same round without ``imitate`` -- the ascent in front of the forward is the one the step reads."""
    online = lambda: toy(online=True)      # noqa: E731
    _, _, plain, _ = profiled(online, rounds=1, branching="strong", strong_candidates=FORMS["union"])
    _, _, learning, _ = profiled(online, rounds=1, branching="strong", strong_candidates=FORMS["union"], imitate=1)
    assert plain.count("k_dual_ascent") == learning.count("k_dual_ascent") >= 3 and learning.count("k_trows_gather") == 1
    _, _, babsr_only, _ = profiled(online, rounds=1, branching="strong", strong_candidates=8, imitate=1)
    _, _, babsr_plain, _ = profiled(online, rounds=1, branching="strong", strong_candidates=8)
    assert babsr_only.count("k_dual_ascent") == babsr_plain.count("k_dual_ascent") + 1      # (without a gnn count the learning round adds it)


# ---- 8. many jobs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branching", ["strong", "gnn"])
def test_every_job_of_a_pool_gets_the_result_it_gets_alone(branching):
    """Two jobs in one pool with ``Shortlist(babsr=8, gnn=4)``, no ``imitate``: results, stats, decisions, bounds, candidates and sources
    are those of the one-job runs."""
    from tests.test_gpu_frontier_jobs import JOBS, toy_jobs
    choice, lps = toy_jobs()
    K, cap, rounds, value = 2, 9, 3, Shortlist(babsr=8, gnn=4)
    alone = []
    for lp, (_, _, _, db) in list(zip(lps, JOBS))[:2]:
        trace, stats, audit = [], {}, []
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, decision_bound=db, capacity=cap,
                                        log=quiet, trace=trace, stats=stats, strong_candidates=value, strong_chunk=5, strong_audit=audit, branching=branching)
        alone.append((res, trace, stats, audit))
    jobs = [FrontierJob(lps[j].input_lb, lps[j].input_ub, lps[j].layers[-1], JOBS[j][3]) for j in range(2)]
    trace, stats, audit = [], [], []
    got = verify_properties_strong(choice, lps[0].layers[:-1], jobs, K=K, segments=2, capacity=cap, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds,
                                   log=quiet, trace=trace, stats=stats, strong_candidates=value, strong_chunk=5, strong_audit=audit, branching=branching)
    assert len(got) == 2 and sum(res[2] for res, _, _, _ in alone) >= 3
    for j, ((res, one, one_stats, one_audit), g) in enumerate(zip(alone, got)):
        print("job", j, "alone", res, one_stats, "together", g, stats[j])
        assert g[0] == res[0] and close_ub(g[1], res[1]) and tuple(g[2:]) == tuple(res[2:]), (j, g, res)
        assert stats[j] == {k: one_stats[k] for k in ("branches", "domains_bounded", "strong_bounded")}
        mine = sorted((t for t in trace if t["job"] == j), key=lambda t: t["round"])
        assert len(mine) == len(one)
        for a, b in zip(mine, one):
            assert a["decisions"] == b["decisions"] and a["parent_bounds"] == b["parent_bounds"]
            assert masked(a["child_bounds"], a["infeasible"], a["live"]) == masked(b["child_bounds"], b["infeasible"], b["live"])
            if branching == "strong":
                assert a["strong_candidates"] == b["strong_candidates"] and a["strong_sources"] == b["strong_sources"]
                assert same(a["strong_improvement"], b["strong_improvement"])
        rows = sorted((a for a in audit if a["job"] == j), key=lambda a: a["round"])      # (stable: a round's rows keep their order)
        assert len(rows) == len(one_audit) >= 1
        for a, b in zip(rows, one_audit):
            assert a["candidates"] == b["candidates"] and a["sources"] == b["sources"] and same(a["improvements"], b["improvements"])
            assert a["decision"] == b["decision"] and a["strong_decision"] == b["strong_decision"]


# ---- 9. the limits that need a handle -------------------------------------------------------------------------------------------------------
def test_limits(engine):
    """An unbound handle is GNNB_E_STATE; a null array GNNB_E_INVALID; a workspace one byte short GNNB_E_NOMEM, and nothing was written."""
    from gnn_branching_amd.engine import ScorerEngine
    relu = bind(engine, NET)
    dev, K, R = engine.device, 2, sum(relu)
    fresh = ScorerEngine(None)
    one = torch.zeros(64, dtype=F64, device=dev)
    p = one.data_ptr()
    empty = _lib.Pool(p, None, None, p, p, p, p, 4, 5)
    assert fresh.lib.gnnb_strong_list_union(fresh.h, C.byref(empty), p, 1, p, p, 1, p, 1, p, p, p, p, p, p, 64, None) == -3
    assert b"gnnb_strong_list_union: call gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_strong_list_union_workspace_bytes(fresh.h, 4) == 0
    lib, h = engine.lib, engine.h
    need = lib.gnnb_strong_list_union_workspace_bytes(h, K)
    assert need > lib.gnnb_strong_list_workspace_bytes(h, K) > 0 and lib.gnnb_strong_list_workspace_bytes(h, K) == K * 16      # the older size stays
    pool = DomainPool(engine, CAP)
    st, keep = engine._pool(pool)
    amb = torch.ones(K, R, dtype=F32, device=dev)
    sa, sb = torch.rand(K, R, device=dev), torch.rand(K, R, device=dev)
    slots = torch.tensor([0, 1], dtype=I32).to(dev)
    cand0 = torch.full((K + 1,), -7, dtype=I32, device=dev)
    lists = [torch.full(s, -7, dtype=I32, device=dev) for s in ((K * 7,), (K * 7,), (K * 7, 2), (K * 7,))]
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def args(a=amb.data_ptr(), b=sb.data_ptr(), src=lists[3].data_ptr(), w=need, pool_=C.byref(st)):
        return (h, pool_, slots.data_ptr(), K, a, sa.data_ptr(), 3, b, 4, cand0.data_ptr(), *(t.data_ptr() for t in lists[:3]), src, ws.data_ptr(), w, None)
    assert lib.gnnb_strong_list_union(*args(w=need - 1)) == -4
    assert b"gnnb_strong_list_union: workspace" in lib.gnnb_last_error()
    for bad in ({"a": None}, {"b": None}, {"src": None}):
        assert lib.gnnb_strong_list_union(*args(**bad)) == -1, bad
        assert b"gnnb_strong_list_union: null argument" in lib.gnnb_last_error()
    assert lib.gnnb_strong_list_union(*args(pool_=None)) == -1
    torch.cuda.synchronize()
    assert cand0.cpu().tolist() == [-7] * (K + 1) and all(int((t != -7).sum()) == 0 for t in lists)
    with pytest.raises(ValueError, match="scores_b"):        # the Python wrapper checks rows and dtypes
        engine.strong_list_union(pool, slots, amb, sa, 3, sb.double(), 4, cand0, *lists)
    with pytest.raises(ValueError, match="cand_src"):
        engine.strong_list_union(pool, slots, amb, sa, 3, sb, 4, cand0, *lists[:3], lists[3][:6])
    engine.strong_list_union(pool, slots, amb, sa, 3, sb, 4, cand0, *lists, workspace=ws)
    got = cand0.cpu().tolist()
    assert got[0] == 0 and 4 <= got[1] <= 7 and 4 <= got[2] - got[1] <= 7
