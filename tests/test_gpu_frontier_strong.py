"""Strong branching inside the device-resident frontier, on the MI355X (gnn_branching_amd/frontier.py
``branching="strong"`` and ``strong_audit``; csrc/gnnb_k_strong.h).  Every comparison is exact unless it says otherwise.

1. gnnb_strong_list against its restatement (tests/frontier_strong_twin.py) on crafted rows of kwg_rect;
2. gnnb_strong_pick against its restatement on crafted child arrays;
3. the improvements of all candidates of toy_kw's root and of its two children against the host twin, for four chunk sizes;
4. branch_and_bound_frontier(branching="strong") against the host loop;
5. ``strong_audit`` next to a "gnn" and a "babsr" run changes nothing and finds no committed decision better than the best;
6. a strong round copies nothing but the number of candidates and the state record;
7. the other modes launch none of the new kernels, a strong run none of the forward's;
8. the limits that need a handle."""
import math

import pytest
import torch

from gnn_branching_amd import _lib
from gnn_branching_amd.frontier import DomainPool, FrontierRun, branch_and_bound_frontier
from tests.frontier_strong_twin import NAN, list_reference, node_of, offsets, pick_reference, same, strong_twin
from tests.frontier_twin import EPS_BAB, LR, N_ITER, bind, engine, masked, toy   # noqa: F401  (engine: the module's fixture)
from tests.test_gpu_frontier_babsr import FORWARD_CLASSES

pytestmark = pytest.mark.gpu

I32, F64, F32 = torch.int32, torch.float64, torch.float32
S = _lib
NET = "kwg_rect"                    # ReLU layers of 1920, 960 and 24 nodes: two wider than a workgroup's 256 threads and no multiple of them, one narrower
INF = float("inf")
STRONG_CLASSES = ("k_strong_count", "k_strong_compact", "k_strong_pick")
KINDS = ["equal", "tie_cut", "zeros", "inf", "nan_decided", "nan_open", "no_open", "bad_slot"]
CAP = 9                             # the crafted pool's slots
SLOTS = [4, 0, 7, 2, 8, 1, 5, CAP]  # distinct; the last one lies outside the pool
PROP, EPS_SMALL = (2, 6), 0.005


def quiet(s):
    pass


# ---- 1. the list ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(engine):
    """One row per kind of KINDS on one pattern of undecided nodes (so the rows share ``count``), as CPU tensors amb / scores (8, R)."""
    relu = bind(engine, NET)
    assert len(relu) >= 3 and min(relu) < 256 and any(r > 256 and r % 256 for r in relu), relu
    off, R, K = offsets(relu), sum(relu), len(KINDS)
    g = torch.Generator().manual_seed(11)
    pattern = (torch.rand(R, generator=g) < 0.5).float()
    edge = list(range(off[1] - 3, off[1] + 3))              # six nodes across the boundary of layers 0 and 1
    pattern[edge] = 1.0
    pattern[[0, R - 1]] = 1.0
    pattern[[1, R - 2]] = 0.0
    amb = pattern.repeat(K, 1)
    scores = torch.rand(K, R, generator=g) * 0.1 + 0.01     # (two of them may be equal: then the index decides, on both sides)
    open_ = [r for r in range(R) if pattern[r] != 0]
    rest = [r for r in open_ if r not in edge]
    for i, kind in enumerate(KINDS):
        if kind == "equal":
            scores[i] = 0.25
        elif kind == "tie_cut":                            # 253 scores above a tie of six across the layer boundary: 255, 256, 257 cut the tie
            scores[i, rest[5::5][:253]] = 0.9
            scores[i, edge] = 0.5
        elif kind == "zeros":                              # the maxima: 300 zeros of both signs; as values they are equal and the index decides
            scores[i] = -scores[i]
            z = open_[3::4][:300]
            scores[i, z[0::2]] = -0.0
            scores[i, z[1::2]] = 0.0
        elif kind == "inf":
            scores[i, rest[7::9][:20]] = INF
            scores[i, rest[2::9][:20]] = -INF
        elif kind == "nan_decided":
            scores[i, [1, R - 2]] = NAN
        elif kind == "nan_open":
            scores[i, open_[len(open_) // 2]] = NAN
        elif kind == "no_open":
            amb[i] = 0.0
    assert len(rest[5::5]) >= 253 and len(open_[3::4]) >= 300
    return relu, amb, scores, len(open_)


def list_on_device(engine, pool, amb, scores, idx, top_m, R, pad=1):
    """gnnb_strong_list on the rows ``idx``; ``pad`` rows and list entries more in every array, which must stay as they were."""
    dev, K = engine.device, len(idx)
    cap = K * (min(R, top_m) if top_m else R)
    rows = lambda t: torch.cat([t[idx], torch.full((pad, R), 3.0)]).contiguous().to(dev)      # noqa: E731
    cand0 = torch.full((K + 1 + pad,), -7, dtype=I32, device=dev)
    cand_row, cand_slot, cand_dec = (torch.full(s, -7, dtype=I32, device=dev) for s in ((cap + pad,), (cap + pad,), (cap + pad, 2)))
    slots = torch.tensor([SLOTS[i] for i in idx], dtype=I32).to(dev)
    engine.strong_list(pool, slots, rows(amb), rows(scores) if top_m else None, top_m, cand0, cand_row, cand_slot, cand_dec)
    cand0, cand_row, cand_slot, cand_dec = (t.cpu().tolist() for t in (cand0, cand_row, cand_slot, cand_dec))
    n = cand0[K]
    assert cand0[K + 1:] == [-7] * pad
    assert cand_row[n:] == [-7] * (cap + pad - n) and cand_slot[n:] == [-7] * (cap + pad - n) and cand_dec[n:] == [[-7, -7]] * (cap + pad - n)
    return cand0[:K + 1], cand_row[:n], cand_slot[:n], cand_dec[:n]


@pytest.mark.parametrize("which", ["0", "1", "255", "256", "257", "count-1", "count", "count+5"])
def test_the_list_against_its_restatement(which, crafted, engine):
    """Every kind of row alone (K = 1) and two groups of five rows that cover all kinds, with a padding row that must stay untouched."""
    relu, amb, scores, count = crafted
    top_m = eval(which, {"count": count})
    R = sum(relu)
    pool = DomainPool(engine, CAP)
    groups = [[i] for i in range(len(KINDS))] + [[0, 1, 2, 3, 4], [7, 6, 5, 4, 3]]
    for idx in groups:
        want = list_reference(relu, amb[idx], scores[idx], top_m, [SLOTS[i] for i in idx], CAP)
        got = list_on_device(engine, pool, amb, scores, idx, top_m, R)
        assert got[0] == want[0], (which, idx, got[0], want[0])
        assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (which, idx)
        counts = [b - a for a, b in zip(want[0], want[0][1:])]
        for i, c in zip(idx, counts):                       # the reference's own outcome, per kind
            kind = KINDS[i]
            full = count if top_m == 0 else min(count, top_m)
            assert c == (0 if kind in ("no_open", "bad_slot") or (kind == "nan_open" and top_m) else full), (kind, c)


def test_the_crafted_ties_are_cut_where_they_were_built_to_be(crafted):
    """The host rule alone: 255, 256 and 257 candidates take 2, 3 and 4 nodes of the tie across the layer boundary, in index order; the
    zeros of both signs are taken in index order whatever their sign."""
    relu, amb, scores, count = crafted
    off = offsets(relu)
    edge = [node_of(relu, r) for r in range(off[1] - 3, off[1] + 3)]
    assert edge[2][0] == 0 and edge[3] == [1, 0]
    for top_m, n_ties in ((255, 2), (256, 3), (257, 4)):
        decs = list_reference(relu, amb[[1]], scores[[1]], top_m, [0], CAP)[3]
        assert [d for d in decs if d in edge] == edge[:n_ties], top_m
        z = list_reference(relu, amb[[2]], scores[[2]], top_m, [0], CAP)[3]
        zeros = [r for r in range(sum(relu)) if amb[2, r] != 0 and scores[2, r] == 0]
        assert z == [node_of(relu, r) for r in zeros[:top_m]] and len(zeros) == 300
        assert {math.copysign(1.0, float(scores[2, r])) for r in zeros[:top_m]} == {1.0, -1.0}


# ---- 2. the pick ------------------------------------------------------------------------------------------------------------------------
def crafted_children(relu):
    """Six parent rows: (parent bound, [(live0, live1, inf0, inf1, lb0, lb1)] per candidate)."""
    g = torch.Generator().manual_seed(3)
    many = [(1, 1, 0, 0, -float(a), -float(b)) for a, b in torch.rand(600, 2, generator=g, dtype=F64)]
    for q in (300, 44, 45):                                 # equal maxima: one thread's second and first candidates, and its neighbour's
        many[q] = (1, 1, 0, 0, 0.25, 0.5)
    return [(-1.0, [(1, 1, 0, 0, -0.5, -0.7), (1, 1, 1, 0, 0.0, -0.9), (1, 1, 1, 1, 0.0, 0.0), (1, 1, 0, 0, 0.5, 0.25), (1, 1, 0, 1, -0.3, -5.0)]),
            (-1.0, []),
            (-2.0, [(1, 1, 0, 0, NAN, -0.5), (1, 0, 0, 0, -0.1, -0.1), (1, 1, 0, 0, -1.9, -1.95), (0, 1, 0, 0, 0.0, 0.0), (1, 1, 0, 0, -1.5, NAN)]),
            (0.5, [(1, 1, 0, 0, 0.6, 0.7), (1, 1, 1, 0, 0.0, 0.9), (1, 1, 0, 0, 0.8, 0.9)]),
            (-1.0, [(0, 0, 0, 0, -0.5, -0.5), (1, 1, 0, 0, NAN, NAN), (1, 0, 1, 1, 0.0, 0.0)]),
            (-3.0, many)]


@pytest.mark.parametrize("with_table", [False, True])
def test_the_pick_against_its_restatement(with_table, engine):
    relu = bind(engine, NET)
    dev, R = engine.device, sum(relu)
    rows = crafted_children(relu)
    K = len(rows)
    pool = DomainPool(engine, CAP)
    slots = SLOTS[:K]
    bounds = torch.full((CAP,), 9.0, dtype=F64)
    bounds[slots] = torch.tensor([b for b, _ in rows], dtype=F64)
    pool.bound.copy_(bounds)
    cand0, cand_dec, live, infeasible, bound = [0], [], [], [], []
    for i, (_, cands) in enumerate(rows):
        step = max(1, (R - 1) // max(1, len(cands)))         # distinct nodes of all three layers, ascending
        for q, (l0, l1, i0, i1, b0, b1) in enumerate(cands):
            cand_dec.append(node_of(relu, (7 * i + q * step) % R))
            live += [l0, l1]
            infeasible += [i0, i1]
            bound += [b0, b1]
        cand0.append(len(cand_dec))
    n = cand0[-1]
    want_dec, want_best, want_imp, want_table = pick_reference(relu, cand0, cand_dec, live, infeasible, bound, [b for b, _ in rows])
    # the reference's own outcome: the first of equal maxima, NaN and dead rows below every number, rows without a number undecided
    assert want_dec[0] == cand_dec[2] and want_best[0] == 1.0 and want_imp[1] < 1.0 and want_imp[3] == 1.0 and want_imp[4] < 1.0
    assert want_dec[1] == [-1, -1] and math.isnan(want_best[1])
    assert want_dec[2] == cand_dec[cand0[2] + 2] and [math.isnan(v) for v in want_imp[cand0[2]:cand0[3]]] == [True, True, False, True, True]
    assert want_dec[3] == cand_dec[cand0[3]] and want_imp[cand0[3]:cand0[4]] == [1.0] * 3
    assert want_dec[4] == [-1, -1] and math.isnan(want_best[4])
    assert want_dec[5] == cand_dec[cand0[5] + 44] and want_imp[cand0[5] + 44] == want_imp[cand0[5] + 300] == want_imp[cand0[5] + 45] == 1.0
    t = lambda v, d, pad: torch.cat([torch.tensor(v, dtype=d).reshape(-1), torch.full((pad,), -7, dtype=d)]).to(dev)      # noqa: E731
    dec, best, imp = (torch.full(s, -7, dtype=d, device=dev) for s, d in (((K + 1, 2), I32), ((K + 1,), F64), ((n + 1,), F64)))
    table = torch.full((K + 1, R), -7.0, dtype=F64, device=dev) if with_table else None
    engine.strong_pick(pool, torch.tensor(slots, dtype=I32).to(dev), t(cand0, I32, 0), t(cand_dec, I32, 2).reshape(-1, 2), n, t(live, I32, 2),
                       t(infeasible, I32, 2), t(bound, F64, 2), dec, best, imp, table)
    dec, best, imp = dec.cpu().tolist(), best.cpu().tolist(), imp.cpu().tolist()
    assert dec[K:] == [[-7, -7]] and best[K:] == [-7.0] and imp[n:] == [-7.0]      # rows from K on, entries from n on are not written
    assert dec[:K] == want_dec
    assert same(best[:K], want_best), (best[:K], want_best)
    assert same(imp[:n], want_imp)
    if with_table:
        table = table.cpu()
        assert table[K].tolist() == [-7.0] * R
        assert same(table[:K].tolist(), want_table)
        assert int(torch.isnan(table[1]).sum()) == R and int((~torch.isnan(table[5])).sum()) == 600


def test_a_slot_outside_the_pool_gets_no_decision(engine):
    relu = bind(engine, NET)
    dev = engine.device
    pool = DomainPool(engine, CAP)
    pool.bound.fill_(-1.0)
    cand0 = torch.tensor([0, 2, 2], dtype=I32).to(dev)     # (a list no gnnb_strong_list writes: the pick checks the slot itself)
    cand_dec = torch.tensor([[0, 1], [0, 2]], dtype=I32).to(dev)
    live, infeasible, bound = torch.ones(4, dtype=I32, device=dev), torch.zeros(4, dtype=I32, device=dev), torch.full((4,), -0.5, dtype=F64, device=dev)
    dec, best, imp = torch.full((2, 2), -7, dtype=I32, device=dev), torch.full((2,), -7.0, dtype=F64, device=dev), torch.full((2,), -7.0, dtype=F64, device=dev)
    engine.strong_pick(pool, torch.tensor([CAP, -1], dtype=I32).to(dev), cand0, cand_dec, 2, live, infeasible, bound, dec, best, imp)
    assert dec.cpu().tolist() == [[-1, -1], [-1, -1]] and all(math.isnan(v) for v in best.cpu().tolist())


# ---- 3. the scores end to end -----------------------------------------------------------------------------------------------------------------
_shared = {}


def audited(chunk, branching="babsr"):
    """Two rounds with K = 2 at the small box with every undecided node a candidate, audited: on this problem BaBSR's split of the root
    leaves both children open (the best split closes one), so round 2 has two parents and a chunk can span their boundary."""
    lp, choice, _ = toy(False, PROP, EPS_SMALL)
    trace, audit, stats = [], [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=quiet, trace=trace, stats=stats,
                                    strong_chunk=chunk, strong_audit=audit, branching=branching)
    return res, trace, audit, stats


def small_twin(commit):
    if "twin" not in _shared:
        _shared["twin"] = strong_twin(2, 2, top_m=0, prop=PROP, eps=EPS_SMALL, commit=commit)
    return _shared["twin"]


@pytest.mark.parametrize("chunk", [1, 5, 7, 64])
def test_every_candidate_improvement_equals_the_twin_for_every_chunk(chunk):
    """The table of toy_kw's root (one parent) and of its two children (K = 2): candidates, improvements, best and the table's decision
    against the host twin that commits the same BaBSR decisions; the same for every chunk size."""
    res, trace, audit, stats = audited(chunk)
    twin = small_twin([t["decisions"] for t in trace])
    counts = [len(a["candidates"]) for a in audit]
    root_lb = trace[0]["parent_bounds"][0]
    print("chunk", chunk, "root bound", root_lb, "candidates", counts, "best", [a["best_improvement"] for a in audit])
    assert root_lb < 0 and 16 <= counts[0] <= 64            # the test's own condition: a root with a table worth the name
    assert len(counts) == 3 and counts[1] % 7 != 0          # round 2 has two parents and the chunk of 7 spans their boundary
    assert stats["strong_bounded"] == 2 * sum(counts)
    rows = iter(audit)
    for r, t in enumerate(trace):
        assert t["decisions"] == twin["decisions"][r] and masked(t["child_bounds"], t["infeasible"], t["live"]) == twin["child_bounds"][r]
        for i in range(len(t["slots"])):
            a = next(rows)
            assert a["candidates"] == twin["candidates"][r][i], (r, i)
            assert same(a["improvements"], twin["improvements"][r][i]), (r, i, a["improvements"], twin["improvements"][r][i])
            assert a["strong_decision"] == twin["strong_decisions"][r][i] and same(a["best_improvement"], twin["best"][r][i])
    if "first" not in _shared:
        _shared["first"] = (res, trace, audit)
    assert same([res, trace, audit], list(_shared["first"]))      # identical for every chunk


def test_a_strong_run_over_all_candidates_equals_the_twin():
    """branching="strong" with strong_candidates=None at the small box: the winners' children, bounded again with the round's children,
    carry the bounds they had as candidates, so the best improvement follows from the committed pair and the parent's bound."""
    from gnn_branching_amd.bab_caller import gnn_improvement
    lp, choice, _ = toy(False, PROP, EPS_SMALL)
    twin = strong_twin(2, 2, top_m=0, prop=PROP, eps=EPS_SMALL)
    trace, audit = [], []
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=quiet, trace=trace, strong_audit=audit,
                                    branching="strong")
    assert [t["decisions"] for t in trace] == twin["decisions"] and len(trace) == 2
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]
    assert [t["strong_candidates"] for t in trace] == twin["candidates"] and same([t["strong_improvement"] for t in trace], twin["improvements"])
    assert res[0] == twin["global_lb"]
    rows = iter(audit)
    for r, t in enumerate(trace):
        for i in range(len(t["slots"])):
            a = next(rows)
            lb0, lb1 = twin["child_bounds"][r][2 * i:2 * i + 2]
            assert a["decision"] == a["strong_decision"] == t["decisions"][i]
            assert a["best_improvement"] == a["improvement"] == twin["best"][r][i] == gnn_improvement(lb0, lb1, twin["parent_bounds"][r][i])


# ---- 4. the loop against the host twin ------------------------------------------------------------------------------------------------------
def strong_run(K, rounds, **kw):
    lp, choice, _ = toy()
    trace, stats = [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=quiet, trace=trace, stats=stats,
                                    branching="strong", **kw)
    return res, trace, stats


@pytest.mark.parametrize("K,rounds", [(1, 3), (3, 3)])
def test_the_loop_equals_the_host_loop_of_the_existing_pieces(K, rounds):
    twin = strong_twin(K, rounds, top_m=8)
    res, trace, stats = strong_run(K, rounds, strong_candidates=8)
    glb, gub, n_rounds, bounded, reason = res
    print("twin", twin, "frontier", res, stats)
    assert twin["branches"] >= 3
    assert [t["decisions"] for t in trace] == twin["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]   # bit for bit: Python floats of the same fp64 values
    assert glb == twin["global_lb"]
    assert abs(gub - twin["global_ub"]) <= 1e-9 * max(1.0, abs(twin["global_ub"]))
    assert [t["strong_candidates"] for t in trace] == twin["candidates"]
    assert same([t["strong_improvement"] for t in trace], twin["improvements"])
    assert [t["parent_bounds"] for t in trace] == twin["parent_bounds"]
    assert bounded == 1 + sum(len(t["live"]) for t in trace)                                               # domains_bounded keeps its meaning
    assert stats["branches"] == twin["branches"] and stats["domains_bounded"] == bounded
    assert stats["strong_bounded"] == 2 * sum(len(c) for t in trace for c in t["strong_candidates"])
    assert all(len(c) <= 8 for t in trace for c in t["strong_candidates"])


# ---- 5. the audit -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branching", ["gnn", "babsr"])
def test_an_audited_run_is_the_run_and_no_decision_beats_the_best(branching):
    lp, choice, _ = toy(False, PROP, EPS_SMALL)
    out = []
    for audit in (None, []):
        trace, stats = [], {}
        extra = {} if audit is None else {"strong_audit": audit}
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=quiet, trace=trace, stats=stats,
                                        branching=branching, **extra)
        out.append((res, trace, {k: v for k, v in stats.items() if k != "strong_bounded"}))
    assert same(list(out[0]), list(out[1])) and len(out[0][1]) == 2       # results, trace (decisions, bounds) and stats
    assert "strong_bounded" not in out[0][2] and stats["strong_bounded"] == 2 * sum(len(a["candidates"]) for a in audit)
    rows = [(r, i) for r, t in enumerate(out[1][1]) for i in range(len(t["slots"]))]
    assert len(audit) == len(rows) >= 2                     # (the GNN's split of the root closes a child: its round 2 has one parent)
    for a, (r, i) in zip(audit, rows):
        t = out[1][1][r]
        print(branching, "round", r, "row", i, {k: a[k] for k in ("slot", "decision", "improvement", "strong_decision", "best_improvement")})
        assert a["slot"] == t["slots"][i] and a["decision"] == t["decisions"][i]
        flat = offsets([int(m.numel()) for m in toy(False, PROP, EPS_SMALL)[2]])[a["decision"][0]] + a["decision"][1]
        assert flat in a["candidates"]                      # every undecided node is a candidate
        assert a["improvements"][a["candidates"].index(flat)] == a["improvement"]      # its children as candidates are the round's children
        assert a["best_improvement"] >= a["improvement"]
        assert a["best_improvement"] == max(a["improvements"])
        assert a["strong_decision"] == node_of([int(m.numel()) for m in toy(False, PROP, EPS_SMALL)[2]], a["candidates"][a["improvements"].index(a["best_improvement"])])


# ---- 6. what crosses the link -------------------------------------------------------------------------------------------------------------------
def test_a_strong_round_copies_nothing_but_the_candidate_count_and_the_state_record():
    """One round under torch.cuda.set_sync_debug_mode("error"): the read of cand0[K] (4 bytes, between the list and its chunks) and the read
    of the state record are the two exemptions."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy()
    run = FrontierRun(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, strong_candidates=8, strong_chunk=3, branching="strong")
    st = run.root()
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
        try:
            run.pool.state.cpu()
            live = False
        except RuntimeError:
            live = True
        finally:
            torch.cuda.set_sync_debug_mode(before)
        if not live:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
        torch.cuda.set_sync_debug_mode("error")
        run.launch_round(1, int(st[S.FS_IN_USE]))
        with pytest.raises(RuntimeError):
            run.read_state()
        torch.cuda.set_sync_debug_mode(before)
        st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert reads == [8] and run.strong_bounded == 16       # three chunks of at most three candidates were bounded under the mode
    run.check_status()


# ---- 7. who launches what -----------------------------------------------------------------------------------------------------------------------
def profiled(**kw):
    lp, choice, _ = toy()
    eng = choice.model.engine()
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.profile_trace()
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=3, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=2, log=quiet, **kw)
        counts = eng.profile_read()
        names = [name for name, _ in eng.profile_trace(1 << 16)]
    finally:
        eng.profile_enable(False)
    return res, counts, names


@pytest.mark.parametrize("branching", ["gnn", "babsr"])
def test_the_other_modes_launch_none_of_the_new_kernels(branching):
    res, counts, names = profiled(branching=branching)
    assert res[2] >= 1 and "k_frontier_gather" in names
    for k in STRONG_CLASSES:
        assert k not in names and counts[k][1] == 0, k


def test_a_strong_run_launches_no_forward_kernel():
    res, counts, names = profiled(branching="strong", strong_candidates=4, strong_chunk=3)
    rounds = res[2]
    assert rounds >= 1
    for k in STRONG_CLASSES:
        assert names.count(k) == rounds == names.count("k_frontier_gather"), k
    for k in FORWARD_CLASSES:
        assert k not in names and counts[k][1] == 0, k
    assert "k_net_eval" in names and names.count("k_net_eval") == rounds + 1       # the root and the winners' children: no candidate is evaluated
    assert "k_frontier_babsr_decide" not in names and "k_frontier_fallback" not in names


# ---- 8. the limits that need a handle -------------------------------------------------------------------------------------------------------------
def test_limits(engine):
    """An unbound handle is GNNB_E_STATE; a null array GNNB_E_INVALID; a workspace one byte short GNNB_E_NOMEM, and nothing was written."""
    import ctypes as C
    from gnn_branching_amd.engine import ScorerEngine
    relu = bind(engine, NET)
    dev, K, R = engine.device, 2, sum(relu)
    fresh = ScorerEngine(None)
    one = torch.zeros(64, dtype=F64, device=dev)
    p = one.data_ptr()
    empty = _lib.Pool(p, None, None, p, p, p, p, 4, 5)
    assert fresh.lib.gnnb_strong_list(fresh.h, C.byref(empty), p, 1, p, None, 0, p, p, p, p, p, 64, None) == -3
    assert b"gnnb_strong_list: call gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_strong_pick(fresh.h, C.byref(empty), p, 1, p, p, p, p, p, p, p, p, None, None) == -3
    assert b"gnnb_strong_pick: call gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_strong_list_workspace_bytes(fresh.h, 4) == 0
    lib, h = engine.lib, engine.h
    need = lib.gnnb_strong_list_workspace_bytes(h, K)
    assert need > 0
    pool = DomainPool(engine, CAP)
    st, keep = engine._pool(pool)
    amb = torch.ones(K, R, dtype=F32, device=dev)
    slots = torch.tensor([0, 1], dtype=I32).to(dev)
    cand0 = torch.full((K + 1,), -7, dtype=I32, device=dev)
    lists = [torch.full(s, -7, dtype=I32, device=dev) for s in ((K * R,), (K * R,), (K * R, 2))]
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = lambda a, w: (h, C.byref(st), slots.data_ptr(), K, a, None, 0, cand0.data_ptr(), *(t.data_ptr() for t in lists), ws.data_ptr(), w, None)      # noqa: E731
    assert lib.gnnb_strong_list(*args(amb.data_ptr(), need - 1)) == -4
    assert b"gnnb_strong_list: workspace" in lib.gnnb_last_error()
    assert lib.gnnb_strong_list(*args(None, need)) == -1
    assert b"gnnb_strong_list: null argument" in lib.gnnb_last_error()
    assert lib.gnnb_strong_list(h, None, slots.data_ptr(), K, amb.data_ptr(), None, 0, cand0.data_ptr(), *(t.data_ptr() for t in lists), ws.data_ptr(), need,
                                None) == -1
    assert lib.gnnb_strong_pick(h, C.byref(st), slots.data_ptr(), K, cand0.data_ptr(), lists[2].data_ptr(), None, p, p, p, p, p, None, None) == -1
    assert b"gnnb_strong_pick: null argument" in lib.gnnb_last_error()
    torch.cuda.synchronize()
    assert cand0.cpu().tolist() == [-7] * (K + 1) and all(int((t != -7).sum()) == 0 for t in lists)
    with pytest.raises(ValueError, match="scorer_mask"):     # the Python wrapper checks rows and dtypes
        engine.strong_list(pool, slots, amb.double(), None, 0, cand0, *lists)
    with pytest.raises(ValueError, match="cand_dec"):
        engine.strong_list(pool, slots, amb, None, 0, cand0, lists[0], lists[1], lists[2][:R])
    engine.strong_list(pool, slots, amb, None, 0, cand0, *lists, workspace=ws)
    assert cand0.cpu().tolist() == [0, R, 2 * R]
    assert lists[0].cpu().tolist() == [0] * R + [1] * R and lists[2][R - 1].cpu().tolist() == [len(relu) - 1, relu[-1] - 1]
