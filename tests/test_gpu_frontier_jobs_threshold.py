"""The BaBSR fall-back for every job of a multi-property frontier, on the MI355X (gnn_branching_amd/frontier.py
verify_properties_threshold; csrc/gnnb_k_frontier.h k_frontier_fallback_jobs / _select_jobs / _rows_sel / _choose_jobs).  Every
comparison is exact.

1. gnnb_frontier_fallback_jobs against the existing gnnb_frontier_fallback called once per entry on that entry's rows with that segment's
   counter and table, and against torch indexing for pair B's boxes and property rows;
2. gnnb_frontier_choose_jobs against the existing gnnb_frontier_choose called once per entry on views;
3. the defining property: every job of ``verify_properties_threshold`` gets the result, the stats and the per-round trace
   ``branch_and_bound_frontier(branching_threshold=T)`` gives it alone;
4. a reused segment starts clean; 5. kwbd_threshold = 0 equals ``verify_properties``; 6. what crosses the link in a round; 7. the limits."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib
from gnn_branching_amd.frontier import DomainPool, FrontierJob, JobsRun, branch_and_bound_frontier, plan_round, verify_properties, verify_properties_threshold
from tests.test_gpu_frontier import engine   # noqa: F401  (the module's fixture)
from tests.test_gpu_frontier_jobs import EPS_BAB, JOBS, LR, N_ITER, sent, toy_jobs
from tests.test_gpu_frontier_threshold import BT, DTHR, KWBD, SEQ, SPARSEST, bind, child_rows, same_float, synthetic_rows, tensors, to_dev
from tests.test_gpu_kw_geometry import Net

pytestmark = pytest.mark.gpu

S = _lib
I32, F64, F32 = torch.int32, torch.float64, torch.float32


def same_floats(a, b):
    return len(a) == len(b) and all(same_float(x, y) for x, y in zip(a, b))


# ---- 1. gnnb_frontier_fallback_jobs ---------------------------------------------------------------------------------------------------
class FallbackCase:
    """The arguments of one gnnb_frontier_fallback_jobs call: ``spec`` = [(segment, rows of ``rows`` (tests/test_gpu_frontier_threshold.py
    synthetic_rows))] in plan order.  A segment's parents sit in random distinct slots of it that depend on the segment alone, its counter
    starts at icp0[segment], its table is ineff0[segment]; the per-segment boxes and property rows are random."""

    def __init__(self, engine, nseg, cap, spec, rows, icp0, ineff0):
        dev, R, N0, NL = engine.device, engine.R, engine.sizes[0], engine.sizes[-2]
        self.engine, self.nseg, self.cap, self.spec, self.dev = engine, nseg, cap, spec, dev
        self.entries, row0 = [], 0
        for seg, idx in spec:
            self.entries.append((seg, row0, len(idx)))
            row0 += len(idx)
        n = self.n = row0
        idx = [i for _, ix in spec for i in ix]
        ch = [c for i in idx for c in (2 * i, 2 * i + 1)]
        slots = torch.cat([torch.randperm(cap, generator=torch.Generator().manual_seed(900 + seg))[:len(ix)] + seg * cap for seg, ix in spec]).to(I32)
        self.pool = DomainPool(engine, nseg * cap)
        pb = torch.full((nseg * cap,), -9.0, dtype=F64)
        pb[slots.long()] = rows["parent"][idx]
        self.pool.bound.copy_(pb)
        self.pool.open.fill_(1)
        self.slots = slots.to(dev)
        self.live, self.infeasible, self.bound = (rows[k][ch].contiguous().to(dev) for k in ("live", "infeasible", "bound"))
        self.scores, self.icps, self.amb = (rows[k][idx].contiguous().to(dev) for k in ("scores", "icps", "amb"))
        self.icp0, self.ineff0 = icp0.to(I32), ineff0.to(I32)
        g = torch.Generator().manual_seed(77)
        self.seg_lo, self.seg_hi = torch.randn(nseg, N0, generator=g, dtype=F64).to(dev), torch.randn(nseg, N0, generator=g, dtype=F64).to(dev)
        self.seg_pw, self.seg_pb = torch.randn(nseg, NL, generator=g).to(dev), torch.randn(nseg, generator=g).to(dev)
        self.plan = sent(dev, self.entries, nseg, cap)

    def outputs(self):
        n, E, dev, N0, NL = self.n, len(self.entries), self.dev, self.engine.sizes[0], self.engine.sizes[-2]
        nan = float("nan")
        return {"imp": torch.full((n + 1,), -5.0, dtype=F64, device=dev), "kw": torch.full((n + 1, 2), -7, dtype=I32, device=dev),
                "sel_rows": torch.full((n,), -7, dtype=I32, device=dev), "sel_slots": torch.full((n,), -7, dtype=I32, device=dev),
                "sel_dec": torch.full((n, 2), -7, dtype=I32, device=dev), "m_entry": torch.full((E + 2,), -7, dtype=I32, device=dev),
                "icp": self.icp0.clone().to(dev), "ineff": self.ineff0.clone().to(dev),
                "b_lo": torch.full((2 * n + 1, N0), nan, dtype=F64, device=dev), "b_hi": torch.full((2 * n + 1, N0), nan, dtype=F64, device=dev),
                "b_pw": torch.full((2 * n + 1, NL), nan, dtype=F32, device=dev), "b_pb": torch.full((2 * n + 1,), nan, dtype=F32, device=dev)}

    def call(self, o, plan=None, **kw):
        self.engine.frontier_fallback_jobs(self.pool, self.plan if plan is None else plan, self.slots, self.live, self.infeasible, self.bound, self.scores,
                                           self.icps, self.amb, o["icp"], o["ineff"], self.seg_lo, self.seg_hi, self.seg_pw, self.seg_pb, o["imp"], o["kw"],
                                           o["sel_rows"], o["sel_slots"], o["sel_dec"], o["m_entry"], o["b_lo"], o["b_hi"], o["b_pw"], o["b_pb"],
                                           kw.pop("branching_threshold", BT), kw.pop("kwbd_threshold", KWBD), SPARSEST, DTHR, **kw)

    def run(self):
        """The jobs call; returns (raw CPU outputs, per segment what its entry got: improvements, KW decisions, m, its slice of the dense
        lists with rows counted from its first, the counter afterwards)."""
        o = self.outputs()
        self.call(o)
        got = {k: v.cpu() for k, v in o.items()}
        per, sel0 = {}, 0
        for e, (seg, row0, k) in enumerate(self.entries):
            m = int(got["m_entry"][e])
            per[seg] = {"imp": got["imp"][row0:row0 + k].tolist(), "kw": got["kw"][row0:row0 + k].tolist(), "m": m,
                        "sel_rows": (got["sel_rows"][sel0:sel0 + m] - row0).tolist(), "sel_slots": got["sel_slots"][sel0:sel0 + m].tolist(),
                        "sel_dec": got["sel_dec"][sel0:sel0 + m].tolist(), "icp": int(got["icp"][seg]), "sel0": sel0}
            sel0 += m
        return got, per

    def one_job(self, e):
        """The existing gnnb_frontier_fallback on entry e's rows with its segment's counter and table: the reference."""
        seg, row0, k = self.entries[e]
        dev, a, b = self.dev, row0, row0 + k
        icp, ineff = self.icp0[seg:seg + 1].clone().to(dev), self.ineff0[seg].clone().to(dev)
        imp, kw = torch.full((k,), -5.0, dtype=F64, device=dev), torch.full((k, 2), -7, dtype=I32, device=dev)
        sel_rows, sel_slots, sel_dec = (torch.full(s, -7, dtype=I32, device=dev) for s in ((k,), (k,), (k, 2)))
        m = torch.full((1,), -7, dtype=I32, device=dev)
        self.engine.frontier_fallback(self.pool, self.slots[a:b], self.live[2 * a:2 * b], self.infeasible[2 * a:2 * b], self.bound[2 * a:2 * b],
                                      self.scores[a:b], self.icps[a:b], self.amb[a:b], icp, ineff, imp, kw, sel_rows, sel_slots, sel_dec, m, BT, KWBD, SPARSEST, DTHR)
        assert torch.equal(ineff.cpu(), self.ineff0[seg])     # read, never written
        mm = int(m.cpu()[0])
        return {"imp": imp.cpu().tolist(), "kw": kw.cpu().tolist(), "m": mm, "sel_rows": sel_rows[:mm].cpu().tolist(),
                "sel_slots": sel_slots[:mm].cpu().tolist(), "sel_dec": sel_dec[:mm].cpu().tolist(), "icp": int(icp.cpu()[0])}


def assert_entry(got, want, what):
    assert same_floats(got["imp"], want["imp"]), (what, got["imp"], want["imp"])
    for key in ("kw", "m", "sel_rows", "sel_slots", "sel_dec", "icp"):
        assert got[key] == want[key], (what, key, got[key], want[key])


def assert_call(case, got, per):
    """Everything one jobs call wrote against the one-job reference per entry and torch indexing; what it must not touch is as it was."""
    n, E = case.n, len(case.entries)
    for e, (seg, row0, k) in enumerate(case.entries):
        assert_entry(per[seg], case.one_job(e), (seg, row0, k))
    M = sum(p["m"] for p in per.values())
    assert got["m_entry"][E].item() == M and got["m_entry"][E + 1].item() == -7
    for key in ("sel_rows", "sel_slots", "sel_dec"):          # poisoned outputs beyond M are untouched
        assert bool((got[key][M:] == -7).all()), key
    assert got["imp"][n].item() == -5.0 and got["kw"][n].tolist() == [-7, -7]
    assert got["sel_slots"][:M].tolist() == case.slots.cpu()[got["sel_rows"][:M].long()].tolist()       # global rows name global slots
    assert torch.equal(got["ineff"], case.ineff0)             # read, never written
    taking = {seg for seg, _, _ in case.entries}
    for seg in range(case.nseg):
        if seg not in taking:
            assert got["icp"][seg].item() == case.icp0[seg].item(), seg
    seg_of = (got["sel_slots"][:M].long() // case.cap).repeat_interleave(2)      # pair B's row c belongs to selected parent c >> 1
    for b, t in (("b_lo", case.seg_lo), ("b_hi", case.seg_hi), ("b_pw", case.seg_pw), ("b_pb", case.seg_pb)):
        assert torch.equal(got[b][:2 * M], t.cpu()[seg_of]), b
        assert bool(torch.isnan(got[b][2 * M:]).all()), b
    return M


def segment_tables(relu, nseg, swapped, seed):
    """ineff (nseg, R) and the starting counters (nseg): random counts below KWBD except at the two nodes synthetic_rows' "ineff_at" /
    "ineff_below" rows name -- (KWBD, KWBD - 1) there, and the other way round in the segments of ``swapped`` --; counters 0, 1, 2 cyclic."""
    R, hi = sum(relu), sum(relu[:-1])
    g = torch.Generator().manual_seed(seed)
    ineff = torch.randint(0, KWBD, (nseg, R), generator=g).to(I32)
    for s in range(nseg):
        ineff[s, hi + 7], ineff[s, hi + 8] = (KWBD - 1, KWBD) if s in swapped else (KWBD, KWBD - 1)
    return ineff, torch.tensor([(s + 1) % 3 for s in range(nseg)], dtype=I32)


@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect", "toy_kw"])
def test_fallback_jobs_against_the_one_job_call_per_entry(name, engine):
    """6 segments of 140 slots; entries of k = 3 (segment 4), k = 1 (segment 0) and k = 130 (segment 2) with a different starting counter
    each.  The k = 3 entry holds an "ineff_at", an "ineff_below" and a "score" row; the k = 1 entry a row above the threshold (m = 0,
    between two entries with m > 0); the k = 130 entry every kind of SEQ four times, in a segment whose table has the two counts the
    other way round: the node at kwbd_threshold in segment 4 is below it in segment 2.  Then each entry alone, and the entries in
    another plan order: the same per-entry results."""
    relu = bind(engine, name)
    rows = synthetic_rows(relu, 160, 61)
    nseg, cap = 6, 140
    at, below, score, above = (SEQ.index(k) for k in ("ineff_at", "ineff_below", "score", "above"))
    spec = [(4, [at, below, score]), (0, [above]), (2, list(range(29, 159)))]
    ineff0, icp0 = segment_tables(relu, nseg, {2}, 62)
    ineff0[0] = 0
    case = FallbackCase(engine, nseg, cap, spec, rows, icp0, ineff0)
    got, per = case.run()
    print(name, "m_entry", got["m_entry"].tolist(), "icp", got["icp"].tolist(), "kw of the first entries", got["kw"][:4].tolist())
    M = assert_call(case, got, per)
    # the test's own conditions
    assert per[4]["m"] > 0 and per[0]["m"] == 0 and per[2]["m"] > 0 and per[2]["sel0"] == per[4]["m"] and M == per[4]["m"] + per[2]["m"]
    assert per[4]["kw"][0] != [-1, -1] and 0 not in per[4]["sel_rows"] and 1 in per[4]["sel_rows"]      # at the threshold there: asked, not selected
    kinds = [rows["kinds"][i] for i in spec[2][1]]
    sel2 = set(per[2]["sel_rows"])
    assert all(i in sel2 for i, k in enumerate(kinds) if k == "ineff_at") and not any(i in sel2 for i, k in enumerate(kinds) if k == "ineff_below")
    assert len({icp0[s].item() for s in (4, 0, 2)}) == 3
    # alone, and in another plan order
    for sub in ([spec[0]], [spec[1]], [spec[2]], [spec[2], spec[0], spec[1]], [spec[1], spec[2]]):
        other = FallbackCase(engine, nseg, cap, sub, rows, icp0, ineff0)
        g2, p2 = other.run()
        assert_call(other, g2, p2)
        for seg in p2:
            assert_entry({k: v for k, v in p2[seg].items() if k != "sel0"}, {k: v for k, v in per[seg].items() if k != "sel0"}, ("alone", seg))


def test_fallback_jobs_prefix_over_more_entries_than_threads(engine):
    """kwg_mlp, 300 entries of k = 1 in 300 segments of 2 slots: the prefix over the entries runs past the workgroup's 256 threads, every
    thread holds more than one entry, counters and tables differ from segment to segment."""
    relu = bind(engine, "kwg_mlp")
    rows = synthetic_rows(relu, 300, 63)
    nseg = 300
    ineff0, icp0 = segment_tables(relu, nseg, set(range(0, nseg, 2)), 64)
    case = FallbackCase(engine, nseg, 2, [(s, [s]) for s in range(nseg)], rows, icp0, ineff0)
    got, per = case.run()
    M = assert_call(case, got, per)
    ms = [per[s]["m"] for s in range(nseg)]
    print("m over the entries", ms[:40], "M", M)
    assert 0 < M < nseg and 0 in ms[256:] and 1 in ms[256:] and 0 in ms[:256] and 1 in ms[:256]
    assert got["sel_rows"][:M].tolist() == [s for s in range(nseg) if ms[s]]       # plan order


# ---- 2. gnnb_frontier_choose_jobs -----------------------------------------------------------------------------------------------------
# per entry (segment, k, [(row of the entry, outcome, node)]): the outcome pair B is built for
CHOOSE_CASES = {
    "none_selected": [(3, 5, []), (1, 5, []), (0, 2, [])],
    "three_outcomes_one_node_twice_in_a_job_and_in_two_jobs": [
        (3, 5, [(0, "ineff", (1, 2)), (2, "used", (1, 4)), (3, "neither", (0, 5)), (4, "ineff", (1, 2))]),
        (0, 2, []),
        (1, 5, [(1, "ineff", (1, 2)), (3, "used", (0, 1))])],
    "all_selected": [(3, 2, [(0, "used", (0, 1)), (1, "ineff", (1, 3))]), (1, 3, [(0, "neither", (0, 2)), (1, "ineff", (1, 3)), (2, "used", (1, 5))])],
}


def view(ns, a, b):
    return types.SimpleNamespace(**{k: ([t[a:b] for t in v] if isinstance(v, list) else v[a:b]) for k, v in vars(ns).items()})


@pytest.mark.parametrize("case", list(CHOOSE_CASES))
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_choose_jobs_against_the_one_job_call_per_entry(name, case, engine):
    """4 segments of 8 slots.  The reference is the existing gnnb_frontier_choose once per entry on views: the entry's rows of pair A and
    of the outputs, its range of the dense lists (rows counted from the entry's first) and of pair B, its segment's row of ineff.
    M = 0, M = n, the three outcomes, two parents of one job naming one node (both count) and two jobs naming the same node (each
    segment's count rises by its own parents only); pair B bit-identical afterwards, unselected rows and a row past 2n untouched."""
    relu = bind(engine, name)
    sizes, R, dev = engine.sizes, engine.R, engine.device
    off = [0] + list(np.cumsum(relu))
    nseg, cap = 4, 8
    spec = CHOOSE_CASES[case]
    entries, row0 = [], 0
    for seg, k, _ in spec:
        entries.append((seg, row0, k))
        row0 += k
    n, m_e = row0, [len(sel) for _, _, sel in spec]
    M = sum(m_e)
    g = torch.Generator().manual_seed(5)
    A, B = child_rows(sizes, R, 2 * n + 1, 3), child_rows(sizes, R, 2 * max(M, 1), 4)
    pool = DomainPool(engine, nseg * cap)
    slots = torch.cat([torch.randperm(cap, generator=g)[:k] + seg * cap for seg, _, k in entries]).to(I32)
    parent = -(torch.rand(n, generator=g, dtype=F64) + 0.5)
    pb = torch.full((nseg * cap,), -9.0, dtype=F64)
    pb[slots.long()] = parent
    pool.bound.copy_(pb)
    gnn_imp = torch.rand(n, generator=g, dtype=F64) * 0.1 + 0.06       # in [0.06, 0.16)
    gnn_dec = torch.tensor([[len(relu) - 1, i] for i in range(n)], dtype=I32)
    sel_rows, sel_dec, q = [], [], 0
    for (seg, row0, k), (_, _, sel) in zip(entries, spec):
        for r, outcome, d in sel:                              # pair B's bounds from the improvement wanted: lb0 = lb1 = (1 - imp) * parent
            row = row0 + r
            p, gi = float(parent[row]), float(gnn_imp[row])
            imp = {"ineff": 0.03, "used": gi + 0.2, "neither": (0.05 + gi) / 2}[outcome]
            B.bound[2 * q], B.bound[2 * q + 1] = p * (1 - imp), p * (1 - imp)
            sel_rows.append(row)
            sel_dec.append(list(d))
            q += 1
    pad = n - M
    sel_rows_t = torch.tensor(sel_rows + [0] * pad, dtype=I32)
    sel_slots_t = torch.tensor([int(slots[r]) for r in sel_rows] + [0] * pad, dtype=I32)
    sel_dec_t = torch.tensor(sel_dec + [[0, 0]] * pad, dtype=I32).reshape(n, 2)
    m_entry = torch.tensor(m_e + [M], dtype=I32)
    ineff0 = torch.randint(0, 5, (nseg, R), generator=g).to(I32)

    def outputs():
        return (torch.full((n + 1,), float("nan"), dtype=F64, device=dev), torch.full((n + 1,), -7, dtype=I32, device=dev),
                torch.full((n + 1, 2), -7, dtype=I32, device=dev))
    # the reference: the one-job call per entry, on views
    wA, dB, w_ineff = to_dev(A, dev), to_dev(B, dev), ineff0.clone().to(dev)
    w_kw, w_used, w_dec = outputs()
    d_rows, d_slots, d_dec, d_gdec, d_gimp = sel_rows_t.to(dev), sel_slots_t.to(dev), sel_dec_t.to(dev), gnn_dec.to(dev), gnn_imp.to(dev)
    sel0 = 0
    for (seg, row0, k), m in zip(entries, m_e):
        a, b, q0 = row0, row0 + k, min(sel0, max(M - 1, 0))
        q1 = max(sel0 + m, q0 + 1)
        engine.frontier_choose(pool, k, m, (d_rows[q0:q1] - row0).contiguous(), d_slots[q0:q1], d_dec[q0:q1], d_gdec[a:b], d_gimp[a:b], view(wA, 2 * a, 2 * b),
                               view(dB, 2 * q0, 2 * q1), w_ineff[seg], w_kw[a:b], w_used[a:b], w_dec[a:b])
        sel0 += m
    # the code under test
    dA, dB2, ineff = to_dev(A, dev), to_dev(B, dev), ineff0.clone().to(dev)
    kw_imp, used, dec = outputs()
    engine.frontier_choose_jobs(pool, sent(dev, entries, nseg, cap), M, m_entry.to(dev), d_rows, d_slots, d_dec, d_gdec, d_gimp, dA, dB2, ineff, kw_imp, used,
                                dec)
    print(case, "kw_improvement", kw_imp.tolist(), "used", used.tolist(), "decisions", dec.tolist())
    assert same_floats(kw_imp.cpu().tolist(), w_kw.cpu().tolist()) and torch.equal(used, w_used) and torch.equal(dec, w_dec)
    assert math.isnan(float(kw_imp[n])) and int(used[n]) == -7 and dec[n].tolist() == [-7, -7]
    assert not bool(torch.isnan(kw_imp[:n]).any()) and bool((used[:n] >= 0).all())       # written for every row of every entry
    assert torch.equal(ineff, w_ineff)
    for got, want in zip(tensors(dA), tensors(wA)):            # chosen rows replaced, every other row (the one past 2n too) as it was
        assert torch.equal(got, want)
    for got, want in zip(tensors(dB2), tensors(B)):
        assert torch.equal(got.cpu(), want)
    # the test's own conditions, on the reference side
    want_used = [0] * n
    for (seg, row0, k), (_, _, sel) in zip(entries, spec):
        for r, outcome, _ in sel:
            want_used[row0 + r] = int(outcome == "used")
    assert w_used[:n].cpu().tolist() == want_used
    delta = (w_ineff.cpu() - ineff0)
    if case.startswith("three_outcomes"):
        node = off[1] + 2
        assert delta[3, node] == 2 and delta[1, node] == 1 and int(delta.sum()) == 3      # each segment counts its own parents only
        assert not bool(delta[0].any()) and not bool(delta[2].any())
        unselected = [r for r in range(n) if r not in sel_rows]
        for t_got, t_before in zip(tensors(dA), tensors(A)):
            for r in unselected:
                assert torch.equal(t_got[2 * r:2 * r + 2].cpu(), t_before[2 * r:2 * r + 2])
    elif case == "none_selected":
        assert not bool(delta.any()) and kw_imp[:n].cpu().tolist() == [-1.0] * n and torch.equal(dec[:n].cpu(), gnn_dec)
    else:
        assert M == n and int(delta[3, off[1] + 3]) == 1 and int(delta[1, off[1] + 3]) == 1


# ---- 3. the defining property -----------------------------------------------------------------------------------------------------------
K, ROUNDS, CAP = 2, 3, 9
TRACE_KEYS = ("parent_bounds", "decisions", "child_bounds", "child_ub", "live", "infeasible", "gnn_decisions", "gnn_improvement", "kw_decisions",
              "kw_improvement", "selected", "used_kw", "gnn_child_bounds", "gnn_child_infeasible", "kw_child_bounds", "kw_child_infeasible")
_shared = {}


def alone(threshold, kwbd=10):
    """Every job of JOBS through the existing one-job loop with the threshold mode on: [(result, trace, stats)]."""
    key = ("alone", threshold, kwbd)
    if key not in _shared:
        choice, lps = toy_jobs()
        out = []
        for lp, (_, _, _, db) in zip(lps, JOBS):
            trace, stats = [], {}
            res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS, decision_bound=db, capacity=CAP,
                                            log=lambda s: None, trace=trace, branching_threshold=threshold, kwbd_threshold=kwbd, stats=stats)
            out.append((res, trace, stats))
        _shared[key] = out
    return _shared[key]


def middle_threshold():
    """The midpoint of the middle adjacent pair of the alone runs' own GNN improvements below 1 at threshold 1.0: from the reference side,
    never from the code under test; no improvement lies within 1e-9 of it."""
    v = sorted({x for _, trace, _ in alone(1.0) for t in trace for x in t["gnn_improvement"] if x == x and x < 1.0})
    assert len(v) >= 2, v
    i = len(v) // 2
    thr = (v[i - 1] + v[i]) / 2
    assert all(abs(x - thr) > 1e-9 for x in v) and 0 < thr < 1, (thr, v)
    return thr


def same_value(a, b):
    if isinstance(a, float) or isinstance(b, float):
        return same_float(float(a), float(b))
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return a == b


def together(threshold, segments, kwbd=10):
    choice, lps = toy_jobs()
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], db) for lp, (_, _, _, db) in zip(lps, JOBS)]
    trace, stats = [], []
    got = verify_properties_threshold(choice, lps[0].layers[:-1], jobs, threshold, K=K, segments=segments, capacity=CAP, n_iter=N_ITER, lr=LR, eps=EPS_BAB,
                                      max_rounds=ROUNDS, kwbd_threshold=kwbd, log=lambda s: None, trace=trace, stats=stats)
    return got, trace, stats


def assert_jobs_equal_alone(single, got, trace, stats):
    assert len(stats) == len(single) == len(got)
    for j, ((res, one, st), g) in enumerate(zip(single, got)):
        print("job", j, "alone", res, st, "together", g, stats[j])
        assert g == res, (j, g, res)                          # floats by ==
        assert stats[j] == st, (j, stats[j], st)
        mine = sorted((t for t in trace if t["job"] == j), key=lambda t: t["round"])
        assert [t["round"] for t in mine] == list(range(len(one)))
        for a, b in zip(mine, one):
            assert set(TRACE_KEYS) | {"slots"} == set(b) and set(b) | {"job", "segment", "round"} == set(a), (sorted(a), sorted(b))
            for key in TRACE_KEYS:
                assert same_value(a[key], b[key]), (j, a["round"], key, a[key], b[key])
            assert [s - a["segment"] * CAP for s in a["slots"]] == b["slots"], (j, a["round"])


def own_conditions():
    """Asserted on the alone side over the two thresholds of the test (the rounds of the jobs that branch coincide when every job has a
    segment of its own): some round has two jobs with m > 0 (a dense offset above 0), some job has m = 0 in a round where another
    has m > 0, and at least one KW pair won.

    JOBS at K = 2 and three rounds as they stand meet all three.  The alone runs on the MI355X showed, selected parents per job and
    round: at T = 1.0 [1, 2, 2] / [1, 2, 2] / [1, 1, 2] / [1, 1, 2] / [1, 2, 2] for the five jobs that branch (five jobs with m > 0 in
    every round) and 3 / 3 / 3 / 1 / 3 KW pairs kept; at the middle threshold (0.1371) [1, 1, 1] / [1, 1, 1] / [0, 0, 1] / [0, 1, 0] /
    [1, 1, 1] (m = 0 beside m > 0 in every round) and 3 / 3 / 1 / 1 / 3 kept."""
    two = gap = won = False
    for thr in (1.0, middle_threshold()):
        single = alone(thr)
        for r in range(ROUNDS):
            ms = [len(trace[r]["selected"]) for _, trace, _ in single if len(trace) > r]
            two |= sum(m > 0 for m in ms) >= 2
            gap |= any(m > 0 for m in ms) and any(m == 0 for m in ms)
        won |= any(st["kw_used"] >= 1 for _, _, st in single)
        print("threshold", thr, "selected per job and round", [[len(t["selected"]) for t in trace] for _, trace, _ in single],
              "kw_used", [st["kw_used"] for _, _, st in single])
    assert two and gap and won, (two, gap, won)


@pytest.mark.parametrize("segments", [3, 7])
@pytest.mark.parametrize("middle", [False, True], ids=["threshold_one", "middle_threshold"])
def test_every_job_gets_the_result_it_gets_alone(middle, segments):
    """The seven JOBS of tests/test_gpu_frontier_jobs.py, K = 2, three rounds, cap 9, in 3 segments (two admission waves, a reused
    segment, jobs that start in different iterations) and in 7: five-tuples, stats dicts and per-round traces (every key; slots modulo
    the segment's first) equal each job alone through branch_and_bound_frontier(branching_threshold=T), at T = 1.0 and at a threshold
    between two of the alone runs' own improvements."""
    thr = middle_threshold() if middle else 1.0
    print("threshold", thr)
    own_conditions()
    single = alone(thr)
    got, trace, stats = together(thr, segments)
    assert_jobs_equal_alone(single, got, trace, stats)
    if middle:
        asked = [kw != [-1, -1] for _, tr, _ in single for t in tr for kw in t["kw_decisions"]]
        assert any(asked) and not all(asked)


# ---- 4. a reused segment starts clean -----------------------------------------------------------------------------------------------------
def threshold_run(n_jobs, threshold=1.0, kwbd=10):
    choice, lps = toy_jobs()
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], None) for lp in lps[:n_jobs]]
    return JobsRun(choice, lps[0].layers[:-1], jobs, tuple(lps[0].input_lb.shape), K, 3, CAP, N_ITER, LR, EPS_BAB, branching_threshold=threshold,
                   kwbd_threshold=kwbd)


def test_a_reused_segment_starts_with_a_zero_counter_and_table():
    run = threshold_run(3)
    g = torch.Generator().manual_seed(91)
    run.icp.copy_(torch.tensor([1, 2, 2], dtype=I32))
    run.ineff.copy_(torch.randint(1, 9, tuple(run.ineff.shape), generator=g).to(I32))
    icp, ineff = run.icp.clone(), run.ineff.clone()
    before = torch.cuda.get_sync_debug_mode() if hasattr(torch.cuda, "get_sync_debug_mode") else None
    try:
        if before is not None:
            torch.cuda.set_sync_debug_mode("error")           # device-side, with no synchronisation
        run.release(1)
        run.admit(1, 2)
    finally:
        if before is not None:
            torch.cuda.set_sync_debug_mode(before)
    assert run.icp.cpu().tolist() == [1, 0, 2] and not bool(run.ineff[1].any())
    assert torch.equal(run.ineff[0], ineff[0]) and torch.equal(run.ineff[2], ineff[2]) and bool(ineff[1].all()) and icp[1] == 2


# ---- 5. kwbd_threshold = 0 ------------------------------------------------------------------------------------------------------------------
def test_kwbd_threshold_zero_selects_nobody_and_equals_verify_properties():
    """No count is below 0, so no parent is ever selected and no second pair is bounded: the results and the traces are
    ``verify_properties``' bit for bit, while the trace still shows the KW decisions."""
    choice, lps = toy_jobs()
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], db) for lp, (_, _, _, db) in zip(lps, JOBS)]
    plain_trace = []
    plain = verify_properties(choice, lps[0].layers[:-1], jobs, K=K, segments=3, capacity=CAP, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=ROUNDS,
                              log=lambda s: None, trace=plain_trace)
    got, trace, stats = together(1.0, 3, kwbd=0)
    assert got == plain and len(trace) == len(plain_trace) >= 5
    for a, b in zip(trace, plain_trace):
        for key in b:
            assert a[key] == b[key], key
        assert a["selected"] == [] and a["used_kw"] == [0] * len(a["slots"]) and a["gnn_decisions"] == a["decisions"] and a["kw_child_bounds"] == []
    assert any(kw != [-1, -1] for t in trace for kw in t["kw_decisions"])
    assert all(st["kw_bounded"] == 0 and st["kw_used"] == 0 and st["domains_bounded"] == res[3] for st, res in zip(stats, plain))


# ---- 6. device residency ----------------------------------------------------------------------------------------------------------------
def test_a_threshold_round_of_three_segments_copies_nothing_but_m_entry_and_the_records():
    """Two rounds under torch.cuda.set_sync_debug_mode("error"): the read of m_entry (between the round's halves) and the read of the
    records are the two exemptions."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    run = threshold_run(3)
    for s in range(3):
        run.admit(s, s)
    run.launch_roots([0, 1, 2])
    st = run.read_state()
    before = torch.cuda.get_sync_debug_mode()
    reads, read_selected = [], run.read_selected

    def exempt_read_of_m_entry():
        with pytest.raises(RuntimeError):                  # the mode is live: the read of m_entry is a synchronising copy
            read_selected()
        torch.cuda.set_sync_debug_mode(before)             # the explicit exemption
        try:
            reads.append(read_selected())
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return reads[-1]
    run.read_selected = exempt_read_of_m_entry
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
            assert all(r[S.FS_N_OPEN] >= 1 for r in st)
            torch.cuda.set_sync_debug_mode("error")
            entries, compact, stopped = plan_round(st, K, CAP)
            assert len(entries) == 3 and not stopped
            run.launch_round(entries)
            with pytest.raises(RuntimeError):
                run.read_state()
            torch.cuda.set_sync_debug_mode(before)
            st = run.read_state()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert len(reads) == 2 and all(len(r) == 4 and r[3] == sum(r[:3]) for r in reads) and max(r[3] for r in reads) >= 1      # a second chain ran under the mode
    run.check_status()


# ---- 7. limits --------------------------------------------------------------------------------------------------------------------------
def test_limits(engine):
    """An unbound handle is GNNB_E_STATE; on a live handle a workspace one byte short is GNNB_E_NOMEM, thresholds outside their ranges, a
    null array, M outside 0..n and every plan error GNNB_E_INVALID, kwg_over (a 4097-node layer) is refused before a launch -- each with
    a message that names the entry point, with nothing written, and the handle stays usable."""
    from gnn_branching_amd.engine import ScorerEngine
    fresh = ScorerEngine(None)
    host = torch.tensor([[0, 0, 1]], dtype=I32)
    pl, pool_s, fb, ch = _lib.Plan(host.data_ptr(), host.data_ptr(), 1, 1, 1, 8), _lib.Pool(), _lib.Fallback(), _lib.Children()
    assert fresh.lib.gnnb_frontier_fallback_jobs(fresh.h, C.byref(pool_s), C.byref(pl), None, C.byref(fb), *([None] * 14), None, 0, None) == -3
    assert b"gnnb_frontier_fallback_jobs" in fresh.lib.gnnb_last_error() and b"gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_choose_jobs(fresh.h, C.byref(pool_s), C.byref(pl), 0, *([None] * 6), C.byref(ch), C.byref(ch), *([None] * 4), None) == -3
    assert b"gnnb_frontier_choose_jobs" in fresh.lib.gnnb_last_error()
    assert fresh.lib.gnnb_frontier_fallback_jobs_workspace_bytes(fresh.h, 1) == 0

    relu = bind(engine, "kwg_mlp")
    sizes, R, dev = engine.sizes, engine.R, engine.device
    rows = synthetic_rows(relu, 3, 1)
    nseg, cap = 2, 8
    ineff0, icp0 = segment_tables(relu, nseg, set(), 2)
    case = FallbackCase(engine, nseg, cap, [(0, [0]), (1, [1, 2])], rows, icp0, ineff0)
    o = case.outputs()
    start = {k: v.clone() for k, v in o.items()}

    def untouched():
        for k in o:
            a, b = o[k].cpu(), start[k].cpu()
            assert torch.equal(torch.nan_to_num(a.double(), nan=123.0), torch.nan_to_num(b.double(), nan=123.0)), k
    need = engine.lib.gnnb_frontier_fallback_jobs_workspace_bytes(engine.h, 3)
    assert need > 0
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback_jobs failed \(-4\)"):
        case.call(o, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    for bad in ({"branching_threshold": 0.0}, {"branching_threshold": 1.5}, {"kwbd_threshold": -1}):
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback_jobs failed \(-1\).*branching_threshold"):
            case.call(o, **bad)
    A, B = to_dev(child_rows(sizes, R, 8, 3), dev), to_dev(child_rows(sizes, R, 8, 4), dev)      # (room for the M = 4 that is refused)
    i3, d3, f3 = torch.zeros(4, dtype=I32, device=dev), torch.zeros(4, 2, dtype=I32, device=dev), torch.zeros(4, dtype=F64, device=dev)
    m_entry, ineff = torch.zeros(3, dtype=I32, device=dev), ineff0.clone().to(dev)

    def choose(plan, M):
        engine.frontier_choose_jobs(case.pool, plan, M, m_entry, i3, i3, d3, d3, f3, A, B, ineff, f3.clone(), i3.clone(), d3.clone())
    for M in (-1, 4):
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_choose_jobs failed \(-1\).*M = " + str(M)):
            choose(case.plan, M)
    good = case.entries
    for bad, what in (([(0, 0, 1), (2, 1, 2)], "segment 2 outside"), ([(0, 0, 1), (-1, 1, 2)], "segment -1 outside"), ([(0, 0, 3), (1, 3, 0)], "k = 0"),
                      ([(0, 0, 1), (1, 2, 2)], "starts at row 2"), ([(0, 0, 1), (1, 1, 1)], "hold 2 rows")):
        plan = sent(dev, bad, nseg, cap)
        plan.n = 3
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback_jobs failed \(-1\).*" + what):
            case.call(o, plan=plan)
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_choose_jobs failed \(-1\).*" + what):
            choose(plan, 0)
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback_jobs failed \(-1\).*3 segments of 8 slots in a pool of 16"):
        bigger = FallbackCase(engine, 3, cap, case.spec, rows, torch.zeros(3, dtype=I32), torch.zeros(3, R, dtype=I32))
        bigger.pool = case.pool
        bigger.call(bigger.outputs())
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_choose_jobs failed \(-1\).*3 segments of 8 slots in a pool of 16"):
        engine.frontier_choose_jobs(case.pool, sent(dev, good, 3, cap), 0, m_entry, i3, i3, d3, d3, f3, A, B, torch.zeros(3, R, dtype=I32, device=dev),
                                    f3.clone(), i3.clone(), d3.clone())
    # a null array: straight through ctypes, a live handle and a good plan
    st, _keep = engine._pool(case.pool)
    pl = engine._plan(case.plan)
    fb = _lib.Fallback()
    assert engine.lib.gnnb_frontier_fallback_jobs(engine.h, C.byref(st), C.byref(pl), case.slots.data_ptr(), C.byref(fb), *([None] * 14), None, 0, None) == -1
    assert b"gnnb_frontier_fallback_jobs: null argument" in engine.lib.gnnb_last_error()
    pa, _ka = engine._children(A, 6, "a")
    assert engine.lib.gnnb_frontier_choose_jobs(engine.h, C.byref(st), C.byref(pl), 1, *([None] * 6), C.byref(pa), C.byref(pa), *([None] * 4), None) == -1
    assert b"gnnb_frontier_choose_jobs: null argument" in engine.lib.gnnb_last_error()
    untouched()
    assert torch.equal(ineff.cpu(), ineff0)
    case.call(o)                                              # the handle stays usable
    choose(case.plan, 0)
    assert int(o["m_entry"][2]) == int(o["m_entry"][0]) + int(o["m_entry"][1])

    over = Net("kwg_over")
    engine.bind(over.fixed, tuple(over.shape))
    R = engine.R
    rows1 = {"parent": torch.full((1,), -1.0, dtype=F64), "live": torch.ones(2, dtype=I32), "infeasible": torch.zeros(2, dtype=I32),
             "bound": torch.full((2,), -0.9, dtype=F64), "scores": torch.zeros(1, R), "icps": torch.zeros(1, R), "amb": torch.ones(1, R)}
    wide = FallbackCase(engine, 1, 3, [(0, [0])], rows1, torch.zeros(1, dtype=I32), torch.zeros(1, R, dtype=I32))
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_fallback_jobs failed \(-1\).*4097 nodes"):
        wide.call(wide.outputs(), workspace=torch.empty(1 << 16, dtype=torch.uint8, device=dev))
    C2 = to_dev(child_rows(engine.sizes, R, 2, 3), dev)
    z = lambda *s, dt=I32: torch.zeros(*s, dtype=dt, device=dev)     # noqa: E731
    with pytest.raises(RuntimeError, match=r"gnnb_frontier_choose_jobs failed \(-1\).*4097 nodes"):
        engine.frontier_choose_jobs(wide.pool, wide.plan, 0, z(2), z(1), z(1), z(1, 2), z(1, 2), z(1, dt=F64), C2, C2, z(1, R), z(1, dt=F64), z(1), z(1, 2))
