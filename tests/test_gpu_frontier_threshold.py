"""The BaBSR fall-back below a branching threshold inside the device-resident frontier, on the MI355X (DESIGN.md section 7.5;
gnn_branching_amd/frontier.py; csrc/gnnb_k_frontier.h):

1. gnnb_frontier_fallback against a Python restatement made of plnn.kw_score_conv.decide and bab_caller.gnn_improvement, exact, on
   synthetic rows that take every branch of the rule;
2. gnnb_frontier_choose against bab_caller.resolve_branching and torch indexing, exact;
3. branch_and_bound_frontier(branching_threshold=...) on toy_kw against a host loop made of public pieces (tests/frontier_twin.py: lp.solve_many(lp="dual_device"),
   GraphChoice.decision / decision_many, BatchedGraphChoice.kw_decision_many = BabsrScorer on the same engine + decide, resolve_branching):
   K = 1 and K = 4 at threshold 1.0, K = 4 at a threshold between two of the twin's own improvements, kwbd_threshold = 0 against the
   plain run, soundness, and what crosses the link in a round."""
import math
import types

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, lp_producer
from gnn_branching_amd.bab_caller import gnn_improvement, resolve_branching
from gnn_branching_amd.frontier import DomainPool, FrontierRun, branch_and_bound_frontier
from gnn_branching_amd.plnn.kw_score_conv import decide
from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, bind, engine, masked, toy, twin   # noqa: F401  (engine: the module's fixture)
from tests.test_dual_ascent_cpu import toy_kw_domains
from tests.test_gpu_kw_geometry import Net

pytestmark = pytest.mark.gpu

S = _lib


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


# ---- 1. gnnb_frontier_fallback ----------------------------------------------------------------------------------------
BT, KWBD, DTHR, SPARSEST = 0.6, 3, 0.001, 0
# the kinds of row, in an order that carries the intercept counter through 0, 1, 2 and its resets, with rows that must leave it alone
# (NaN, dead, bound >= 0, above the threshold) in between
SEQ = ["icp0", "icp0", "icp0", "icp0", "score", "icp0", "icp_late", "icp0", "icp0", "nan", "icp0", "sparsest_max", "popped", "tie_layer",
       "tie_across_hi", "tie_across_lo", "bound_pos", "infeasible", "dead", "above", "ineff_at", "ineff_below", "no_open", "icp0", "dead",
       "icp0", "bound_pos", "icp0", "both_infeasible"]


def synthetic_rows(relu, K, seed):
    """K parent rows of the kinds of SEQ (cyclic).  Returns a dict of CPU tensors: scores / intercepts / amb (K, R), pair A's live /
    infeasible / bound (2K), the parents' bounds (K) and the ineff table (R)."""
    g = torch.Generator().manual_seed(seed)
    L, R = len(relu), sum(relu)
    off = [0] + list(np.cumsum(relu))
    hi, lo = L - 1, L - 2                                  # the two layers of the across-layer ties (lo may be the sparsest layer 0)
    tl = tie_layer_of(relu)
    scores = torch.rand(K, R, generator=g) * 5e-4          # all at or below decision_threshold
    icps = -torch.rand(K, R, generator=g) * 5e-5           # all above -1e-4
    amb = (torch.rand(K, R, generator=g) < 0.5).float()
    amb[:, [o for o in off[:-1]]] = 0.0                    # the first undecided node of a layer is not node 0 ...
    amb[:, [o + 2 for o in off[:-1]]] = 1.0                # ... but node 1 or 2
    live = torch.ones(2 * K, dtype=torch.int32)
    infeasible = torch.zeros(2 * K, dtype=torch.int32)
    parent = -(torch.rand(K, generator=g, dtype=torch.float64) + 0.5)
    shrink = torch.rand(2 * K, generator=g, dtype=torch.float64) * 0.15
    bound = parent.repeat_interleave(2) * (1.0 - shrink)   # improvements around 0.075; with one infeasible child below 0.575: below BT
    ineff = torch.zeros(R, dtype=torch.int32)
    ineff[off[hi] + 7], ineff[off[hi] + 8] = KWBD, KWBD - 1
    kinds = [SEQ[i % len(SEQ)] for i in range(K)]
    for i, kind in enumerate(kinds):
        if kind == "score":
            scores[i, off[hi] + 11] = 0.5
        elif kind == "icp0":
            icps[i, off[0] + 5] = -0.5
            icps[i, off[0] + 9] = -0.5                     # (an equal minimum later in the layer: the first one counts)
            if relu[0] > 300:
                icps[i, off[0] + 261] = -0.5               # (and one a thread stride behind the first)
        elif kind == "icp_late":
            icps[i, off[0] + 5] = -0.5
            icps[i, off[1] + 4] = -0.25
        elif kind == "nan":
            scores[i, off[hi] + 1] = float("nan")
            icps[i, off[0] + 5] = -0.5
        elif kind == "sparsest_max":
            scores[i, off[SPARSEST] + 2] = 0.7
        elif kind == "popped":
            amb[i, off[hi]:off[hi + 1]] = 0.0              # the layer popped first has no undecided node
        elif kind == "tie_layer":                          # equal maxima in one layer: neighbours, and (a wide layer) one thread stride apart
            for j in ([270, 14, 15, 526] if relu[tl] > 600 else [14, 13, 21]):
                scores[i, off[tl] + j] = 0.25
        elif kind == "tie_across_hi":                      # equal maxima in two layers: the tuple (value, index) with the larger index wins
            scores[i, off[lo] + 3], scores[i, off[hi] + 6] = 0.125, 0.125
        elif kind == "tie_across_lo":
            scores[i, off[lo] + 6], scores[i, off[hi] + 3] = 0.125, 0.125
        elif kind == "bound_pos":
            parent[i] = 0.25 if i % 2 else 0.0
            scores[i, off[hi] + 11] = 0.5
        elif kind == "infeasible":
            infeasible[2 * i], bound[2 * i] = 1, -7.0
            scores[i, off[hi] + 12] = 0.5
        elif kind == "both_infeasible":
            infeasible[2 * i], infeasible[2 * i + 1] = 1, 1
        elif kind == "dead":
            live[2 * i], live[2 * i + 1] = 0, 0
            bound[2 * i], bound[2 * i + 1] = float("nan"), float("nan")
            scores[i, off[hi] + 11] = 0.5
        elif kind == "above":                              # improvement 0.625
            bound[2 * i], bound[2 * i + 1] = parent[i] * 0.25, parent[i] * 0.5
            scores[i, off[hi] + 11] = 0.5
        elif kind == "ineff_at":
            scores[i, off[hi] + 7] = 0.5
        elif kind == "ineff_below":
            scores[i, off[hi] + 8] = 0.5
        elif kind == "no_open":
            amb[i] = 0.0
            scores[i, off[hi] + 11] = 0.5
    return {"scores": scores, "icps": icps, "amb": amb, "live": live, "infeasible": infeasible, "bound": bound, "parent": parent, "ineff": ineff,
            "kinds": kinds}


def tie_layer_of(relu):
    """The widest ReLU layer that is not the sparsest one: where the equal maxima inside a layer go."""
    return max((l for l in range(len(relu)) if l != SPARSEST), key=lambda l: relu[l])


def fallback_reference(relu, rows, idx, icp):
    """The rule of a threshold round (steps 2 - 4) for the rows ``idx`` of ``rows``, restated with decide and gnn_improvement.  Returns
    (improvements, KW decisions, selected [(position, decision)], icp after, icp before every row)."""
    off = [0] + list(np.cumsum(relu))
    order = lp_producer._random_order(len(relu), SPARSEST)
    imps, kws, sel, before = [], [], [], []
    for pos, i in enumerate(idx):
        before.append(icp)
        kws.append([-1, -1])
        if not rows["live"][2 * i]:
            imps.append(float("nan"))
            continue
        b = float(rows["parent"][i])
        lbs = [INF if rows["infeasible"][c] else float(rows["bound"][c]) for c in (2 * i, 2 * i + 1)]
        imps.append(gnn_improvement(lbs[0], lbs[1], b) if b < 0 else 1.0)
        if not imps[-1] < BT:
            continue
        s, t, m = (list(torch.split(rows[k][i], relu)) for k in ("scores", "icps", "amb"))
        if bool(torch.isnan(rows["scores"][i]).any()) or bool(torch.isnan(rows["icps"][i]).any()) or not bool((rows["amb"][i] != 0).any()):
            continue                                       # the documented deviation: no KW decision, the counter stays
        try:
            d, icp = decide(s, t, m, icp, order, SPARSEST, DTHR)
        except IndexError:                                 # random_order ran out
            continue
        kws[-1] = [int(d[0]), int(d[1])]
        if int(rows["ineff"][off[d[0]] + d[1]]) < KWBD:
            sel.append((pos, kws[-1]))
    return imps, kws, sel, icp, before


def run_fallback(engine, rows, idx, icp0, seed):
    """gnnb_frontier_fallback on the rows ``idx``; the parents sit in random distinct slots of a pool with a few slots more."""
    dev, K, R = engine.device, len(idx), engine.R
    pool = DomainPool(engine, K + 3)
    slots = torch.randperm(K + 3, generator=torch.Generator().manual_seed(seed))[:K].to(torch.int32)
    pb = torch.full((K + 3,), -9.0, dtype=torch.float64)
    pb[slots.long()] = rows["parent"][idx]
    pool.bound.copy_(pb)
    pool.open.fill_(1)
    ch = torch.tensor([c for i in idx for c in (2 * i, 2 * i + 1)])
    i32 = torch.int32
    out = {"imp": torch.full((K,), -5.0, dtype=torch.float64, device=dev), "kw": torch.full((K, 2), -7, dtype=i32, device=dev),
           "sel_rows": torch.full((K,), -7, dtype=i32, device=dev), "sel_slots": torch.full((K,), -7, dtype=i32, device=dev),
           "sel_dec": torch.full((K, 2), -7, dtype=i32, device=dev), "m": torch.full((1,), -7, dtype=i32, device=dev),
           "icp": torch.tensor([icp0], dtype=i32).to(dev), "ineff": rows["ineff"].to(dev)}
    engine.frontier_fallback(pool, slots.to(dev), rows["live"][ch].contiguous().to(dev), rows["infeasible"][ch].contiguous().to(dev),
                             rows["bound"][ch].contiguous().to(dev), rows["scores"][idx].contiguous().to(dev), rows["icps"][idx].contiguous().to(dev),
                             rows["amb"][idx].contiguous().to(dev), out["icp"], out["ineff"], out["imp"], out["kw"], out["sel_rows"], out["sel_slots"],
                             out["sel_dec"], out["m"], BT, KWBD, SPARSEST, DTHR)
    got = {k: v.cpu() for k, v in out.items()}
    got["slots"] = slots
    return got


def assert_fallback(got, want, rows, what):
    imps, kws, sel, icp, _ = want
    m = int(got["m"][0])
    print(what, "m", m, "icp", int(got["icp"][0]), "kw", got["kw"].tolist()[:32], "improvements", got["imp"].tolist()[:8])
    assert all(same_float(a, b) for a, b in zip(got["imp"].tolist(), imps)), (what, got["imp"].tolist(), imps)
    assert got["kw"].tolist() == kws, what
    assert m == len(sel) and int(got["icp"][0]) == icp, (what, m, len(sel), int(got["icp"][0]), icp)
    assert got["sel_rows"][:m].tolist() == [p for p, _ in sel] and got["sel_dec"][:m].tolist() == [d for _, d in sel], what
    assert got["sel_slots"][:m].tolist() == [int(got["slots"][p]) for p, _ in sel], what
    assert torch.equal(got["ineff"], rows["ineff"]), what  # read, never written


@pytest.mark.parametrize("K", [1, 3, 130])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect", "toy_kw"])
def test_fallback_against_the_restatement(name, K, engine):
    """Every branch of the rule (the kinds of SEQ), compared exactly: improvements as Python floats; decisions, selection, m and the
    intercept counter as integers.  K = 130: more rows than a workgroup has waves, every kind four times and the counter carried through
    them.  Then the rows of the first cycle alone (K = 1 calls) from the counter the restatement had before them: the same row results."""
    relu = bind(engine, name)
    rows = synthetic_rows(relu, K, 50 + K)
    idx = list(range(K))
    for icp0 in ((0, 1) if K > 1 else (0, 1, 2)):
        want = fallback_reference(relu, rows, idx, icp0)
        got = run_fallback(engine, rows, idx, icp0, 7 + icp0)
        assert_fallback(got, want, rows, (name, K, icp0))
    kinds_hit = {k: 0 for k in SEQ}
    for i, (kind, kw) in enumerate(zip(rows["kinds"], want[1])):
        kinds_hit[kind] += kw != [-1, -1]
    if K == 130:                                           # the restatement took the branches the rows were built for
        assert all(kinds_hit[k] > 0 for k in ("score", "icp0", "icp_late", "sparsest_max", "popped", "tie_layer", "tie_across_hi", "tie_across_lo",
                                               "infeasible", "ineff_at", "ineff_below"))
        assert all(kinds_hit[k] == 0 for k in ("nan", "dead", "bound_pos", "above", "no_open", "both_infeasible"))
        hi, tl = len(relu) - 1, tie_layer_of(relu)
        by_kind = {kind: kw for kind, kw in zip(rows["kinds"][:len(SEQ)], want[1][:len(SEQ)])}
        assert by_kind["tie_layer"] == [tl, 14 if relu[tl] > 600 else 13] and by_kind["tie_across_hi"] == [hi, 6]
        assert [0, 5] in [kw for kw, kind in zip(want[1], rows["kinds"]) if kind == "icp0"]       # the first of the equal minima
        assert by_kind["popped"][0] == hi - 1 and by_kind["sparsest_max"][0] == hi and by_kind["icp_late"] == [1, 4]
        assert 2 in want[4] and any(a == 2 and kw[0] == hi for a, kw, kind in zip(want[4], want[1], rows["kinds"]) if kind == "icp0")
        sel_pos = {p for p, _ in want[2]}
        assert all((rows["kinds"][p] != "ineff_at") for p in sel_pos) and any(rows["kinds"][p] == "ineff_below" for p in sel_pos)
        imps, kws, _, _, before = want
        for i in range(len(SEQ)):
            alone = run_fallback(engine, rows, [i], before[i], 90 + i)
            assert same_float(float(alone["imp"][0]), imps[i]) and alone["kw"].tolist() == [kws[i]], (name, i, rows["kinds"][i])
            assert int(alone["icp"][0]) == (before[i + 1] if i + 1 < K else want[3]), (name, i)


# ---- 2. gnnb_frontier_choose ------------------------------------------------------------------------------------------
def child_rows(sizes, R, n, seed):
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    return types.SimpleNamespace(
        mask=torch.randint(-1, 2, (n, R), generator=g).to(torch.int8), lb=[torch.randn(n, s, generator=g, dtype=f64) for s in sizes[1:]],
        ub=[torch.randn(n, s, generator=g, dtype=f64) for s in sizes[1:]], infeasible=torch.zeros(n, dtype=torch.int32),
        bound=-torch.rand(n, generator=g, dtype=f64) - 0.1, alpha=torch.rand(n, R, generator=g, dtype=f64), beta=torch.rand(n, R, generator=g, dtype=f64),
        ubv=torch.randn(n, generator=g, dtype=f64), live=torch.ones(n, dtype=torch.int32))


FIELDS = ("mask", "infeasible", "bound", "alpha", "beta", "ubv", "live")


def to_dev(ns, dev):
    return types.SimpleNamespace(**{k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in vars(ns).items()})


def tensors(ns):
    return [getattr(ns, f) for f in FIELDS] + list(ns.lb) + list(ns.ub)


# per selected parent: the outcome its pair B is built for, and the node its KW decision names
CHOOSE_CASES = {
    "none_selected": (5, []),
    "three_outcomes": (5, [(0, "ineff", (0, 3)), (2, "used", (1, 4)), (3, "neither", (0, 5))]),
    "all_selected_two_name_one_node": (5, [(0, "ineff", (1, 2)), (1, "used", (0, 1)), (2, "ineff", (1, 2)), (3, "equal", (0, 6)), (4, "used_infeasible", (1, 2))]),
}


@pytest.mark.parametrize("case", list(CHOOSE_CASES))
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_choose_against_resolve_branching_and_torch_indexing(name, case, engine):
    """The three outcomes of resolve_branching, two parents naming one node (both count), m = 0 and m = K; the unselected rows of pair A,
    a row past 2K and the whole pair B bit-identical afterwards; the outputs start poisoned (NaN / -7) and are written for every row."""
    relu = bind(engine, name)
    sizes, R, dev = engine.sizes, engine.R, engine.device
    off = [0] + list(np.cumsum(relu))
    K, sel = CHOOSE_CASES[case]
    m = len(sel)
    A, B = child_rows(sizes, R, 2 * K + 1, 3), child_rows(sizes, R, 2 * max(m, 1), 4)
    pool = DomainPool(engine, K + 2)
    g = torch.Generator().manual_seed(5)
    slots = torch.randperm(K + 2, generator=g)[:K].to(torch.int32)
    parent = -(torch.rand(K, generator=g, dtype=torch.float64) + 0.5)
    pb = torch.full((K + 2,), -9.0, dtype=torch.float64)
    pb[slots.long()] = parent
    pool.bound.copy_(pb)
    gnn_imp = torch.rand(K, generator=g, dtype=torch.float64) * 0.1 + 0.06     # in [0.06, 0.16)
    gnn_dec = torch.tensor([[len(relu) - 1, i] for i in range(K)], dtype=torch.int32)
    for j, (row, outcome, _) in enumerate(sel):            # pair B's bounds from the improvement wanted: lb0 = lb1 = (1 - imp) * parent
        p, gi = float(parent[row]), float(gnn_imp[row])
        imp = {"ineff": 0.03, "used": gi + 0.2, "neither": (0.05 + gi) / 2, "equal": None, "used_infeasible": None}[outcome]
        if outcome == "equal":                             # the improvement of pair A's own formula: not greater, so pair A stays
            B.bound[2 * j], B.bound[2 * j + 1] = p * 0.9, p * 0.9
            gnn_imp[row] = gnn_improvement(p * 0.9, p * 0.9, p)
        elif outcome == "used_infeasible":                 # an infeasible child counts as +inf: improvement 0.5 + ...
            B.infeasible[2 * j], B.bound[2 * j], B.bound[2 * j + 1] = 1, -7.0, p * 0.9
        else:
            B.bound[2 * j], B.bound[2 * j + 1] = p * (1 - imp), p * (1 - imp)
    sel_rows = torch.tensor([r for r, _, _ in sel] + [0] * (K - m), dtype=torch.int32)
    sel_slots = torch.tensor([int(slots[r]) for r, _, _ in sel] + [0] * (K - m), dtype=torch.int32)
    sel_dec = torch.tensor([list(d) for _, _, d in sel] + [[0, 0]] * (K - m), dtype=torch.int32)
    ineff0 = torch.zeros(R, dtype=torch.int32)
    ineff0[off[1] + 2] = 4
    # the restatement
    table = {f"{l}-{i}": int(ineff0[off[l] + i]) for l in range(len(relu)) for i in (1, 2, 3, 4, 5, 6)}
    want_dec, want_used, want_kw = gnn_dec.tolist(), [0] * K, [-1.0] * K
    want_A = types.SimpleNamespace(**{k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in vars(A).items()})
    for j, (row, outcome, d) in enumerate(sel):
        lbs = [INF if B.infeasible[c] else float(B.bound[c]) for c in (2 * j, 2 * j + 1)]
        want_kw[row] = gnn_improvement(lbs[0], lbs[1], float(parent[row]))
        dec, used = resolve_branching(gnn_dec[row].tolist(), float(gnn_imp[row]), list(d), want_kw[row], table)
        want_dec[row], want_used[row] = [int(dec[0]), int(dec[1])], int(used)
        assert used == outcome.startswith("used"), (outcome, want_kw[row], float(gnn_imp[row]))
        if used:
            for a, b in zip(tensors(want_A), tensors(B)):
                a[2 * row], a[2 * row + 1] = b[2 * j], b[2 * j + 1]
    want_ineff = ineff0.clone()
    for key, v in table.items():
        l, i = (int(x) for x in key.split("-"))
        want_ineff[off[l] + i] = v
    if case == "all_selected_two_name_one_node":
        assert int(want_ineff[off[1] + 2]) == 6            # both parents counted
    # the device
    dA, dB = to_dev(A, dev), to_dev(B, dev)
    ineff = ineff0.to(dev)
    kw_imp = torch.full((K + 1,), float("nan"), dtype=torch.float64, device=dev)
    used_kw, dec_out = torch.full((K + 1,), -7, dtype=torch.int32, device=dev), torch.full((K + 1, 2), -7, dtype=torch.int32, device=dev)
    engine.frontier_choose(pool, K, m, sel_rows.to(dev), sel_slots.to(dev), sel_dec.to(dev), gnn_dec.to(dev), gnn_imp.to(dev), dA, dB, ineff, kw_imp,
                           used_kw, dec_out)
    print(case, "kw_improvement", kw_imp.tolist(), "used", used_kw.tolist(), "decisions", dec_out.tolist())
    assert kw_imp[:K].cpu().tolist() == want_kw and used_kw[:K].cpu().tolist() == want_used and dec_out[:K].cpu().tolist() == want_dec
    assert math.isnan(float(kw_imp[K])) and int(used_kw[K]) == -7 and dec_out[K].tolist() == [-7, -7]
    assert torch.equal(ineff.cpu(), want_ineff)
    for got, want in zip(tensors(dA), tensors(want_A)):    # chosen rows replaced, every other row (the one past 2K too) as it was
        assert torch.equal(got.cpu(), want)
    for got, want in zip(tensors(dB), tensors(B)):
        assert torch.equal(got.cpu(), want)


def test_limits(engine):
    """An unbound handle is GNNB_E_STATE, m > K GNNB_E_INVALID, kwg_over (a 4097-node layer) is refused before a launch, a workspace one
    byte short is GNNB_E_NOMEM -- each with a message that names the entry point."""
    import ctypes as C
    from gnn_branching_amd.engine import ScorerEngine
    fresh = ScorerEngine(None)
    pool_s, fb, ch = _lib.Pool(), _lib.Fallback(), _lib.Children()
    assert fresh.lib.gnnb_frontier_fallback(fresh.h, C.byref(pool_s), None, 1, C.byref(fb), *([None] * 6), None, 0, None) == -3
    assert b"gnnb_frontier_fallback" in fresh.lib.gnnb_last_error() and b"gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_choose(fresh.h, C.byref(pool_s), 1, 0, *([None] * 5), C.byref(ch), C.byref(ch), *([None] * 4), None) == -3
    assert b"gnnb_frontier_choose" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_fallback_workspace_bytes(fresh.h, 1) == 0

    relu = bind(engine, "kwg_mlp")
    sizes, R, dev = engine.sizes, engine.R, engine.device
    rows = synthetic_rows(relu, 2, 1)
    pool = DomainPool(engine, 3)
    A, B = to_dev(child_rows(sizes, R, 4, 3), dev), to_dev(child_rows(sizes, R, 4, 4), dev)
    i2, d2 = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 2, dtype=torch.int32, device=dev)
    f2, ineff = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    st, _keep = engine._pool(pool)
    pa, _ka = engine._children(A, 4, "a")
    assert engine.lib.gnnb_frontier_choose(engine.h, C.byref(st), 2, 3, i2.data_ptr(), i2.data_ptr(), d2.data_ptr(), d2.data_ptr(), f2.data_ptr(), C.byref(pa),
                                           C.byref(pa), ineff.data_ptr(), f2.data_ptr(), i2.data_ptr(), d2.data_ptr(), None) == -1
    assert b"gnnb_frontier_choose: m = 3" in engine.lib.gnnb_last_error()
    need = engine.lib.gnnb_frontier_fallback_workspace_bytes(engine.h, 2)
    assert need > 0
    dv = {k: v.to(dev) for k, v in rows.items() if torch.is_tensor(v)}
    args = (pool, i2.clone(), dv["live"], dv["infeasible"], dv["bound"], dv["scores"], dv["icps"], dv["amb"], torch.zeros(1, dtype=torch.int32, device=dev), ineff,
            f2.clone(), d2.clone(), i2.clone(), i2.clone(), d2.clone(), torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback failed \(-4\)"):
        engine.frontier_fallback(*args, BT, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    for bad in ({"branching_threshold": 0.0}, {"branching_threshold": 1.5}, {"branching_threshold": 0.2, "kwbd_threshold": -1}):
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback failed \(-1\).*branching_threshold"):
            engine.frontier_fallback(*args, **bad)
    engine.frontier_fallback(*args, BT)                     # the handle stays usable

    over = Net("kwg_over")
    engine.bind(over.fixed, tuple(over.shape))
    R = engine.R
    pool = DomainPool(engine, 3)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)     # noqa: E731
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback failed \(-1\).*4097 nodes"):
        engine.frontier_fallback(pool, z(1, dt=torch.int32), z(2, dt=torch.int32), z(2, dt=torch.int32), z(2, dt=torch.float64), z(1, R), z(1, R), z(1, R),
                                 z(1, dt=torch.int32), z(R, dt=torch.int32), z(1, dt=torch.float64), z(1, 2, dt=torch.int32), z(1, dt=torch.int32),
                                 z(1, dt=torch.int32), z(1, 2, dt=torch.int32), z(1, dt=torch.int32), BT, workspace=z(64, dt=torch.uint8))
    C2 = to_dev(child_rows(engine.sizes, R, 2, 3), dev)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_choose failed \(-1\).*4097 nodes"):
        engine.frontier_choose(pool, 1, 0, z(1, dt=torch.int32), z(1, dt=torch.int32), z(1, 2, dt=torch.int32), z(1, 2, dt=torch.int32),
                               z(1, dt=torch.float64), C2, C2, z(R, dt=torch.int32), z(1, dt=torch.float64), z(1, dt=torch.int32), z(1, 2, dt=torch.int32))


# ---- 3. the loop on toy_kw against a host loop of public pieces -------------------------------------------------------
_shared = {}


def frontier_run(K, rounds, threshold, kwbd=10):
    lp, choice, _ = toy()
    trace, stats = [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace,
                                    branching_threshold=threshold, kwbd_threshold=kwbd, stats=stats)
    return res, trace, stats


def runs(K, rounds, threshold):
    key = (K, rounds, threshold)
    if key not in _shared:
        _shared[key] = (twin(K, rounds, threshold, sides=threshold < 1.0), frontier_run(K, rounds, threshold))
    return _shared[key]


def assert_same_run(twin, run):
    (glb, gub, rounds, bounded, reason), trace, stats = run
    print("twin", twin, "frontier", (glb, gub, rounds, bounded, reason), stats)
    for t in trace:
        print("round", {k: t[k] for k in ("gnn_decisions", "gnn_improvement", "kw_decisions", "kw_improvement", "selected", "used_kw", "decisions")})
    assert len(trace) == len(twin["decisions"])
    for key in ("decisions", "gnn_decisions", "kw_decisions", "used_kw", "selected"):
        assert [t[key] for t in trace] == twin[key], key
    assert [t["gnn_improvement"] for t in trace] == twin["gnn_improvement"]               # Python floats of the same fp64 values
    assert [t["kw_improvement"] for t in trace] == twin["kw_improvement"]
    assert [masked(t["gnn_child_bounds"], t["gnn_child_infeasible"], t["live"]) for t in trace] == twin["gnn_child_bounds"]
    assert [masked(t["kw_child_bounds"], t["kw_child_infeasible"]) for t in trace] == twin["kw_child_bounds"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]
    assert glb == twin["global_lb"]
    assert abs(gub - twin["global_ub"]) <= 1e-9 * max(1.0, abs(twin["global_ub"]))
    n_sel = sum(len(s) for s in twin["selected"])
    assert stats == {"branches": sum(len(d) for d in twin["decisions"]), "kw_bounded": n_sel, "kw_used": sum(sum(u) for u in twin["used_kw"]),
                     "domains_bounded": bounded}
    assert bounded == 1 + sum(len(t["live"]) for t in trace) + 2 * n_sel


def test_k1_at_threshold_one_equals_the_host_loop():
    """K = 1, 4 rounds, branching_threshold = 1.0: every parent with a negative bound asks BaBSR."""
    twin, run = runs(1, 4, 1.0)
    assert len(twin["decisions"]) >= 3 and twin["asked"] >= 3
    assert_same_run(twin, run)


def test_k4_at_threshold_one_equals_the_host_loop():
    twin, run = runs(4, 3, 1.0)
    assert len(twin["decisions"]) >= 3 and twin["asked"] >= 3
    assert_same_run(twin, run)


def middle_threshold():
    """The midpoint between two adjacent sorted GNN improvements of the twin's own threshold-1.0 run at K = 4 (the middle pair): derived
    from the twin, never from the code under test.  On toy_kw's property (2, 6) at eps 0.04."""
    twin, _ = runs(4, 3, 1.0)
    v = sorted(x for r in twin["gnn_improvement"] for x in r if x < 1.0)
    assert len(v) >= 2, v
    i = len(v) // 2
    return (v[i - 1] + v[i]) / 2


def test_k4_at_a_middle_threshold_equals_the_host_loop():
    """K = 4 at a threshold that parts the twin's parents: some ask BaBSR, some do not (the twin asserts both, and that no improvement lies
    within 1e-9 of the threshold)."""
    thr = middle_threshold()
    print("middle threshold", thr)
    assert 0 < thr < 1
    twin, run = runs(4, 3, thr)
    assert_same_run(twin, run)
    asked = [kw != [-1, -1] for t in run[1] for kw in t["kw_decisions"]]
    assert any(asked) and not all(asked)


def test_kwbd_threshold_zero_selects_nobody_and_equals_the_plain_run():
    """kwbd_threshold = 0: no count is below it, so no parent is ever selected and no second pair is bounded -- the run is the
    branching_threshold=None run bit for bit (decisions, bounds, result) while its trace still shows the KW decisions."""
    lp, choice, _ = toy()
    plain_trace = []
    plain = branch_and_bound_frontier(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=3, log=lambda s: None, trace=plain_trace)
    res, trace, stats = frontier_run(4, 3, 1.0, kwbd=0)
    assert res == plain and len(trace) == len(plain_trace) >= 1
    for a, b in zip(trace, plain_trace):
        for key in b:
            assert a[key] == b[key], key
        assert a["selected"] == [] and a["used_kw"] == [0] * len(a["slots"]) and a["gnn_decisions"] == a["decisions"] and a["kw_child_bounds"] == []
    assert any(kw != [-1, -1] for t in trace for kw in t["kw_decisions"])
    assert stats["kw_bounded"] == 0 and stats["kw_used"] == 0 and stats["domains_bounded"] == plain[3]


@pytest.mark.parametrize("K,rounds", [(1, 4), (4, 3)])
def test_soundness(K, rounds):
    """As tests/test_gpu_frontier.py test_soundness: global_lb <= global_ub, and global_lb at most the network's minimum over 256 sampled
    points of the box + 1e-5."""
    _, ((glb, gub, *_), _, _) = runs(K, rounds, 1.0)
    lp0, _ = toy_kw_domains()
    assert glb <= gub
    with torch.no_grad():
        x = lp0.input_lb.float() + (lp0.input_ub - lp0.input_lb).float() * torch.rand((256,) + lp0.shapes[0], generator=torch.Generator().manual_seed(0))
        for l in lp0.layers:
            x = l(x)
    assert glb <= float(x.min()) + 1e-5


def test_a_threshold_round_copies_nothing_but_m_and_the_state_record():
    """Two rounds under torch.cuda.set_sync_debug_mode("error"): the read of m (4 bytes, between the round's halves) and the read of the
    state record are the two exemptions."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy()
    run = FrontierRun(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, branching_threshold=1.0)
    st = run.root()
    before = torch.cuda.get_sync_debug_mode()
    reads, read_selected = [], run.read_selected

    def exempt_read_of_m():
        with pytest.raises(RuntimeError):                  # the mode is live: the read of m is a synchronising copy
            read_selected()
        torch.cuda.set_sync_debug_mode(before)             # the explicit exemption
        try:
            reads.append(read_selected())
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return reads[-1]
    run.read_selected = exempt_read_of_m
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
        for _ in range(2):
            n_open, in_use = int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
            assert n_open >= 1
            torch.cuda.set_sync_debug_mode("error")
            run.launch_round(min(4, n_open), in_use)
            with pytest.raises(RuntimeError):
                run.read_state()
            torch.cuda.set_sync_debug_mode(before)
            st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert len(reads) == 2 and max(reads) >= 1             # a second pair was bounded under the mode
    run.check_status()
