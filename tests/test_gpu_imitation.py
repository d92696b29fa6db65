"""The imitation step on the MI355X (csrc/gnnb_k_train.h k_tloss_table, k_tscore_bwd_w_dense; gnnb_imitation_step_rows,
gnnb_imitation_loss; ``branch_and_bound_frontier(imitate=N)``).

1. the loss rule, exact against its restatement (tests/imitation_twin.py), through gnnb_imitation_loss on crafted arrays;
2. the gradient per tensor against fp64 autograd under tests/test_online_gradients.py's own yardstick;
3. bit-identity: listed rows against the same rows as a compact batch, two runs, no state shared with the online loss, the row guard;
4. twenty steps on one batch and table halve the loss;
5. the frontier against a host loop of public pieces.

The preconditions of 2 and 4 (which seeds, margin and learning rate make a case a test of the kernels and not of a hinge gate) are
asserted on the CPU, in tests of their own that run without a GPU."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

from gnn_branching_amd import synth
from tests import margins, test_online_gradients as tog
from tests.common import KW_ARCHS, register_kw_archs, register_toy_archs, state_of
from tests.imitation_twin import NAN, ImitationOracle, rule_rows, seeded_table, ulp32
from tests.test_online_gradients import FSCORE_BIAS, INP_B, K_BAR, PROPS, bits, check_gradient
from oracle.online_oracle import split_blob

I32, F32, F64 = torch.int32, torch.float32, torch.float64
MARGIN = 4.0                        # the gradient cases' margin: see test_the_gradient_cases_are_decided_by_no_hinge_gate
NEAR_ZERO = 1e-3


def make(net, B, seed):
    register_kw_archs()
    register_toy_archs()
    shape = KW_ARCHS[net][0] if net in KW_ARCHS else None
    return synth.make_batch(net, B, seed=seed, props=[PROPS[b % len(PROPS)] for b in range(B)], input_shape=shape)


def take(batch, idx):
    """The subproblems ``idx`` of a batch, in that order, as a batch of their own."""
    B = batch.batch_size
    rows = lambda t: t.reshape(B, -1, *t.shape[1:])[idx].reshape(-1, *t.shape[1:])      # noqa: E731  (batch-major flat tensors)
    return synth.SubproblemBatch([t[idx] for t in batch.lower_bounds_all], [t[idx] for t in batch.upper_bounds_all], [rows(t) for t in batch.dual_vars],
                                 [rows(t) for t in batch.primals], batch.primal_inputs[idx],
                                 {"fixed_layers": batch.layers["fixed_layers"], "prop_layers": [batch.layers["prop_layers"][i] for i in idx]},
                                 batch.masks[idx])


def new_engine(state=None, T=2, lr=1e-4, wd=1e-4):
    from gnn_branching_amd.engine import ScorerEngine
    eng = ScorerEngine(state_of("random") if state is None else state, T=T)
    eng.online_create(lr, wd)
    return eng


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------------
RULE_NET = "kwg_rect"               # R = 2904 = 1920 + 960 + 24: more than one stride of 256 threads, no multiple of it
ROWS = ["many", "edges", "one", "none", "spread"]


@lru_cache(None)
def crafted():
    """Five rows over R = 2904 flat indices (scores fp32, -inf at decided nodes; mask; table fp64), built on one mask pattern."""
    R = sum(int(np.prod(s)) for s in [(8, 12, 20), (16, 6, 10), (24,)])
    g = np.random.RandomState(5)
    mask = (g.uniform(size=R) < 0.6).astype(np.float32)
    mask[[0, 1, 2, 1919, 1920, R - 2, R - 1]] = 1.0
    open_ = np.flatnonzero(mask)
    s = np.tile(np.where(mask != 0, g.uniform(-0.1, 0.1, R), -np.inf).astype(np.float32), (len(ROWS), 1))
    m = np.tile(mask, (len(ROWS), 1))
    tau = np.full((len(ROWS), R), NAN)
    # many: a teacher, 300 violators with scores of their own (a sum of 300 different fp32 terms) and 50 candidates far below
    many = open_[5::3][:351]
    t, viol, low = many[200], np.delete(many, 200)[:300], np.delete(many, 200)[300:]
    tau[0, t], tau[0, viol], tau[0, low] = 1.0, g.uniform(0.0, 0.5, 300), 0.9
    s[0, t], s[0, low] = 0.0, -5.0
    # edges: equal tau maxima (the lower index is the teacher), a tie in tau with a higher score, a term of exactly 0, a term one ulp above 0
    e = open_[[3, 40, 41, 500, 900, 901]]
    tau[1, e] = [1.0, 1.0, 0.25, 0.5, 0.5, -3.0]
    s[1, e[0]] = 0.5
    s[1, e[1]] = 0.75                                          # tau tie with the teacher, higher score: delta 0, term 0.25 > 0
    s[1, e[2]] = -0.25                                         # -0.75 + 0.75 = 0 exactly: no violator
    s[1, e[3]] = 0.0                                           # -0.5 + 0.5 = 0 exactly
    s[1, e[4]] = 2.0 ** -24                                    # (2^-24 - 0.5) + 0.5 = 2^-24: the smallest term this sum can give above zero
    s[1, e[5]] = 3.0                                           # -3: delta 4, term 6.5
    tau[2, open_[77]] = 0.3                                    # one candidate
    # none: no candidate.  spread: 16 candidates, among them the first and the last flat index
    sp = np.concatenate([[0, R - 1, 1919, 1920], open_[100::120][:12]])
    tau[4, sp] = g.uniform(0.0, 1.0, sp.size)
    return s, m, tau, {"teacher_many": int(t), "edges": [int(v) for v in e]}


def run_rule(engine, s, m, tau, margin, poison=7.0):
    """gnnb_imitation_loss on host arrays: ds starts at 0 on the mask and at ``poison`` outside it."""
    dev = engine.device
    ds0 = np.where(m != 0, 0.0, poison).astype(np.float32)
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(dev, d)      # noqa: E731
    loss, ds, report, regret, status = engine.imitation_loss(t(s, F32), t(m, F32), t(tau, F64), margin, ds=t(ds0, F32))
    torch.cuda.synchronize()
    return loss.cpu().numpy(), ds.cpu().numpy(), report.cpu().numpy(), regret.cpu().numpy(), int(status.cpu()[0]), ds0


def same_or_nan(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_rule(got, want, m, ds0):
    loss, ds, report, regret, status, _ = got
    wl, wds, wrep, wreg, wst = want
    assert status == wst
    assert report.tolist() == wrep.tolist(), (report.tolist(), wrep.tolist())
    assert same_or_nan(regret, wreg), (regret, wreg)
    assert np.array_equal(ds[m == 0], ds0[m == 0])          # outside the mask: untouched
    assert np.array_equal(np.where(m != 0, ds, 0.0), wds), "ds differs from the twin's"
    for b in range(len(wl)):
        print(f"  row {b}: loss hip {loss[b]!r} twin {wl[b]!r} violators {report[b, 3]}")
        if math.isnan(wl[b]):
            assert math.isnan(loss[b]), b
        else:
            assert abs(float(loss[b]) - float(wl[b])) <= ulp32(wl[b]), (b, loss[b], wl[b])


@pytest.fixture(scope="module")
def engine():
    from tests.frontier_twin import bind
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    eng = ScorerEngine(None)
    assert sum(bind(eng, RULE_NET)) == crafted()[0].shape[1]
    return eng


def test_the_crafted_rows_are_what_they_were_built_to_be():
    """The twin alone (no GPU): 300 violators, the exact zeros, the one-ulp term, the tie, one and no candidate, both ends of the index range."""
    s, m, tau, info = crafted()
    loss, ds, rep, regret, status = rule_rows(s, m, tau, 1.0)
    e = info["edges"]
    assert status == 0
    assert rep[0].tolist()[0] == info["teacher_many"] and rep[0].tolist()[2:] == [351, 300] and ds[0, info["teacher_many"]] == -300.0
    assert rep[1].tolist()[0] == e[0] and rep[1].tolist()[2] == 6                   # equal maxima: the lower index
    assert [int(ds[1, q]) for q in e] == [-3, 1, 0, 0, 1, 1]                         # tie violates, both exact zeros do not, the ulp does
    assert rep[2].tolist() == [int(np.flatnonzero(~np.isnan(tau[2]))[0])] * 2 + [1, 0] and loss[2] == 0 and not ds[2].any()
    assert rep[3].tolist() == [-1, -1, 0, 0] and math.isnan(loss[3]) and math.isnan(regret[3])
    cand = np.flatnonzero(~np.isnan(tau[4]))
    assert cand[0] == 0 and cand[-1] == s.shape[1] - 1 and rep[4, 2] == 16
    term = np.float32(np.float32(s[1, e[4]] - s[1, e[0]]) + np.float32(0.5))
    assert 0 < float(term) <= 2.0 ** -24                                             # one ulp of the fp32 sum above zero


@pytest.mark.gpu
@pytest.mark.parametrize("margin", [1.0, 0.0, 0.37])
def test_the_rule_on_five_rows_and_on_each_alone(margin, engine):
    s, m, tau, _ = crafted()
    got = run_rule(engine, s, m, tau, margin)
    check_rule(got, rule_rows(s, m, tau, margin), m, got[5])
    for b in range(len(ROWS)):                                # n = 1: the same bits as in the batch
        one = run_rule(engine, s[b:b + 1], m[b:b + 1], tau[b:b + 1], margin)
        check_rule(one, rule_rows(s[b:b + 1], m[b:b + 1], tau[b:b + 1], margin), m[b:b + 1], one[5])
        assert bits(one[0]).tolist() == bits(got[0][b:b + 1]).tolist() and np.array_equal(one[1][0], got[1][b])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["decided", "+inf", "-inf"])
def test_a_refused_row_sets_the_status_and_leaves_the_others_alone(bad, engine):
    s, m, tau, _ = crafted()
    good = run_rule(engine, s, m, tau, 1.0)
    tau2 = tau.copy()
    if bad == "decided":
        tau2[4, np.flatnonzero(m[4] == 0)[10]] = 0.5           # a candidate at a decided node (score -inf there)
    else:
        tau2[4, np.flatnonzero(~np.isnan(tau[4]))[3]] = math.inf if bad == "+inf" else -math.inf
    got = run_rule(engine, s, m, tau2, 1.0)
    want = rule_rows(s, m, tau2, 1.0)
    assert want[4] == 8 and math.isnan(want[0][4])
    check_rule(got, want, m, got[5])
    assert got[4] == 8 and math.isnan(got[0][4]) and got[2][4].tolist() == [-1, -1, 0, 0] and math.isnan(got[3][4])
    assert np.array_equal(got[1][4], got[5][4])              # no ds entry in the refused row
    assert bits(got[0][:4]).tolist() == bits(good[0][:4]).tolist() and np.array_equal(got[1][:4], good[1][:4])
    assert got[2][:4].tolist() == good[2][:4].tolist()
    empty = run_rule(engine, s[3:4], m[3:4], tau[3:4], 1.0)   # no candidate: NaN and NO status bit
    assert empty[4] == 0 and math.isnan(empty[0][0])


@pytest.mark.gpu
def test_the_teacher_is_strong_picks_decision_on_a_table_it_wrote(engine):
    from gnn_branching_amd.frontier import DomainPool
    from tests.frontier_strong_twin import node_of, offsets
    from tests.test_gpu_frontier_strong import CAP, SLOTS, crafted_children
    from tests.frontier_twin import bind
    relu = bind(engine, RULE_NET)
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
        step = max(1, (R - 1) // max(1, len(cands)))
        for q, (l0, l1, i0, i1, b0, b1) in enumerate(cands):
            cand_dec.append(node_of(relu, (7 * i + q * step) % R))
            live += [l0, l1]
            infeasible += [i0, i1]
            bound += [b0, b1]
        cand0.append(len(cand_dec))
    n = cand0[-1]
    t = lambda v, d: torch.tensor(v, dtype=d).to(dev)          # noqa: E731
    dec, best, imp = torch.zeros(K, 2, dtype=I32, device=dev), torch.zeros(K, dtype=F64, device=dev), torch.zeros(n, dtype=F64, device=dev)
    table = torch.zeros(K, R, dtype=F64, device=dev)
    engine.strong_pick(pool, t(slots, I32), t(cand0, I32), t(cand_dec, I32).reshape(-1, 2), n, t(live, I32), t(infeasible, I32), t(bound, F64), dec, best,
                       imp, table)
    loss, ds, report, regret, status = engine.imitation_loss(torch.zeros(K, R, dtype=F32, device=dev), torch.ones(K, R, dtype=F32, device=dev), table, 1.0)
    off = offsets(relu)
    want = [-1 if d[0] < 0 else off[d[0]] + d[1] for d in dec.cpu().tolist()]
    assert int(status.cpu()[0]) == 0
    assert report[:, 0].cpu().tolist() == want and sum(w >= 0 for w in want) >= 4 and -1 in want
    counts = (~torch.isnan(table)).sum(1).cpu().tolist()
    assert report[:, 2].cpu().tolist() == counts


# ---- 2. the gradient --------------------------------------------------------------------------------------------------------------------
# (case, network, B, batch seed, candidates per sample or None for every undecided node, table seed, T)
GRAD_CASES = [("mlp_B2_M2", "kwg_mlp", 2, 11, 2, 1, 2), ("mlp_B2_M16", "kwg_mlp", 2, 11, 16, 1, 2), ("mlp_B2_all", "kwg_mlp", 2, 11, None, 1, 2),
              ("rect_B3_M2", "kwg_rect", 3, 12, 2, 1, 2), ("rect_B3_M16", "kwg_rect", 3, 12, 16, 1, 2), ("rect_B3_all", "kwg_rect", 3, 12, None, 3, 2),
              ("conv3_B2_M16", "toy_conv3", 2, 13, 16, 1, 2), ("conv3_B2_all", "toy_conv3", 2, 13, None, 1, 2),
              ("mlp_B2_M16_T1", "kwg_mlp", 2, 11, 16, 1, 1), ("mlp_B2_M16_T3", "kwg_mlp", 2, 11, 16, 1, 3)]
GRAD_IDS = [c[0] for c in GRAD_CASES]


class Ref:
    """Both twins on one case: named gradients, losses, terms and violator sets.  The attribute names are those
    tests.test_online_gradients.check_gradient reads (kws: the table, imps: the margin -- what ImitationOracle.step takes in their place)."""

    def __init__(self, state, args, table, margin, T=2):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.state, self.args, self.kws, self.imps, self.T = state, args, table, margin, T
        self.g, self.loss, self.terms, self.violators = {}, {}, {}, {}
        for dt in (torch.float64, torch.float32):
            o = ImitationOracle(state, T=T, dtype=dt)
            loss, _ = o.step(args, table, margin, apply=False)
            self.g[dt] = split_blob(o.grad_blob().astype(np.float64), state)
            self.loss[dt] = np.asarray(loss, np.float64)
            self.terms[dt], self.violators[dt] = o.terms, o.violators

    def below_range(self):
        return [k for k, v in self.g[torch.float64].items() if float(np.abs(v).max()) < tog.BELOW_RANGE]


@lru_cache(None)
def grad_case(case):
    _, net, B, seed, M, tseed, T = GRAD_CASES[GRAD_IDS.index(case)]
    batch = make(net, B, seed)
    table = seeded_table(batch.masks.numpy(), M, tseed)
    return batch, table, Ref(state_of("random"), batch.forward_args(), table, MARGIN, T)


@pytest.mark.parametrize("case", GRAD_IDS)
def test_the_gradient_cases_are_decided_by_no_hinge_gate(case):
    """The precondition of the gradient test, on the CPU: the fp32 and the fp64 twin have the same violators and no fp64 term lies within
    1e-3 of zero (a fp32 evaluation is ~1e-6 off), so the kernels see the same hinge gates as the yardstick; every sample has a violator,
    and only fscore.bias (and at T = 1 the input-update tensors) has a zero gradient.  The margin (4: a term moves by 4 per unit of
    improvement, so few of thousands of uniform improvements land within 1e-3 of a gate) and the seeds were chosen so that this holds."""
    batch, table, ref = grad_case(case)
    T = GRAD_CASES[GRAD_IDS.index(case)][6]
    assert ref.violators[torch.float32] == ref.violators[torch.float64]
    near = min(abs(v) for terms in ref.terms[torch.float64] for v in terms.values())
    print(case, "violators", [len(v) for v in ref.violators[torch.float64]], "of", [len(t) + 1 for t in ref.terms[torch.float64]], "closest term", near)
    assert near >= NEAR_ZERO, near
    assert all(len(v) >= 1 for v in ref.violators[torch.float64])
    assert sorted(ref.below_range()) == sorted((FSCORE_BIAS,) + (INP_B if T == 1 else ())), ref.below_range()


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAD_IDS)
def test_gradient_per_tensor_against_fp64(case, monkeypatch):
    """|g_hip - g64| <= 4 max(|g32 - g64|, 2^-23 max |g64|) per tensor: tests/test_online_gradients.py's yardstick and its ReLU-kink
    re-examination (with the imitation twin in OnlineOracle's place); the gradient of fscore.bias is exactly 0.0: every ds entry is a small
    integer and they add up to zero per sample."""
    batch, table, ref = grad_case(case)
    T = GRAD_CASES[GRAD_IDS.index(case)][6]
    eng = new_engine(T=T)
    w0 = eng.get_weights()
    loss, report, regret = eng.imitation_step(batch.forward_args(), table, MARGIN, apply=False)
    np.testing.assert_array_equal(eng.get_weights(), w0)
    g = eng.online_grad()
    assert report[:, 3].tolist() == [len(v) for v in ref.violators[torch.float64]]
    assert report[:, 2].tolist() == [len(t) + 1 for t in ref.terms[torch.float64]]
    for b in range(len(loss)):
        yard = max(abs(ref.loss[torch.float32][b] - ref.loss[torch.float64][b]), tog.EPS32 * sum(abs(v) for v in ref.terms[torch.float64][b].values()))
        print(f"  {case} loss[{b}]: hip {loss[b]:.7g} fp64 {ref.loss[torch.float64][b]:.7g} yard {yard:.3e}")
        assert abs(float(loss[b]) - ref.loss[torch.float64][b]) <= K_BAR * yard
    parts = split_blob(g, ref.state)
    assert parts[FSCORE_BIAS].tolist() == [0.0]
    monkeypatch.setattr(tog, "OnlineOracle", ImitationOracle)
    worst = check_gradient("imitation_" + case, ref, g, tuple(ref.below_range()))
    margins.record("imitation_gradients", case, worst_ratio=worst, k_bar=K_BAR, margin=MARGIN,
                   violators=",".join(str(len(v)) for v in ref.violators[torch.float64]))


# ---- 3. bit-identity --------------------------------------------------------------------------------------------------------------------
ID_NET, ID_K, ID_SEED = "kwg_mlp", 5, 21


@lru_cache(None)
def id_case():
    batch = make(ID_NET, ID_K, ID_SEED)
    return batch, seeded_table(batch.masks.numpy(), 16, 3)


def device_batch(eng, batch):
    from gnn_branching_amd.engine import make_batch
    m = eng._marshal(*batch.forward_args())
    cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
    return cb, (m, keep)


def step_rows(eng, batch, table, rows, apply, margin=1.0):
    """gnnb_imitation_step_rows on ``rows`` of the K-row batch: (loss, report, regret, status, gradient, parameters, source unchanged)."""
    dev, n = eng.device, len(rows)
    cb, keep = device_batch(eng, batch)
    m = keep[0]
    src = [t for grp in (m.lbs, m.ubs, m.duals, m.prim) for t in grp] + [m.x_lp, m.mask, m.pw, m.pb]
    before = [t.clone() for t in src]
    tab = torch.from_numpy(table).to(dev)
    tab0 = tab.clone()
    loss, report = torch.full((n,), -7.0, dtype=F32, device=dev), torch.full((n, 4), -7, dtype=I32, device=dev)
    regret, status = torch.full((n,), -7.0, dtype=F64, device=dev), torch.zeros(1, dtype=I32, device=dev)
    eng.imitation_step_rows(cb, batch.batch_size, torch.tensor(rows, dtype=I32).to(dev), tab, margin, loss, report, regret, status, apply)
    same = all(torch.equal(a, b) for a, b in zip(before, src)) and torch.equal(tab0.view(torch.int64), tab.view(torch.int64))
    return loss.cpu().numpy(), report.cpu().numpy(), regret.cpu().numpy(), int(status.cpu()[0]), eng.online_grad(), eng.get_weights(), same


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [[3], [3, 0, 4], [0, 1, 2, 3, 4]])
def test_listed_rows_equal_the_same_rows_as_a_compact_batch(rows):
    batch, table = id_case()
    for apply in (False, True):
        loss, report, regret, status, g, w, same = step_rows(new_engine(lr=1e-3), batch, table, rows, apply)
        eng = new_engine(lr=1e-3)
        w0 = eng.get_weights()
        closs, creport, cregret = eng.imitation_step(take(batch, rows).forward_args(), table[rows], 1.0, apply=apply)
        assert same and status == 0
        assert bits(loss).tolist() == bits(closs).tolist() and report.tolist() == creport.tolist() and regret.tolist() == cregret.tolist()
        assert bits(g).tolist() == bits(eng.online_grad()).tolist() and np.abs(g).max() > 0
        assert bits(w).tolist() == bits(eng.get_weights()).tolist()
        assert (bits(w) != bits(w0)).any() == apply
        assert all(r[3] >= 1 for r in report.tolist())        # every row had a violator: the step learnt from each


@pytest.mark.gpu
def test_two_runs_are_bit_equal():
    batch, table = id_case()
    a = step_rows(new_engine(lr=1e-3), batch, table, [3, 0, 4], True)
    b = step_rows(new_engine(lr=1e-3), batch, table, [3, 0, 4], True)
    for x, y in zip(a[:3] + a[4:6], b[:3] + b[4:6]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


@pytest.mark.gpu
def test_no_state_leaks_between_the_two_losses():
    """After an imitation step a gnnb_online_step gives what it gives on a fresh engine set to the same parameters, and the other way
    round: the dense fscore path and the two-node path share buffers, not state."""
    batch, table = id_case()
    one = take(batch, [1, 2])
    kws = tog.middle_kw(one.masks)
    eng = new_engine(lr=1e-3)
    eng.imitation_step(batch.forward_args(), table, 1.0)
    w1 = eng.get_weights()
    loss, _ = eng.online_step(one.forward_args(), kws, [0.1, 0.2], apply=False)
    g = eng.online_grad()
    fresh = new_engine(lr=1e-3)
    fresh.set_weights(w1)
    floss, _ = fresh.online_step(one.forward_args(), kws, [0.1, 0.2], apply=False)
    assert bits(loss).tolist() == bits(floss).tolist() and bits(g).tolist() == bits(fresh.online_grad()).tolist()
    a = eng.imitation_step(one.forward_args(), table[[1, 2]], 1.0, apply=False)      # an online step in between
    ga = eng.online_grad()
    b = fresh.imitation_step(one.forward_args(), table[[1, 2]], 1.0, apply=False)
    assert bits(a[0]).tolist() == bits(b[0]).tolist() and bits(ga).tolist() == bits(fresh.online_grad()).tolist()


@pytest.mark.gpu
def test_a_row_outside_the_batch_sets_the_status_and_the_others_are_not_affected():
    batch, table = id_case()
    loss, report, regret, status, g, w, same = step_rows(new_engine(), batch, table, [3, ID_K, 4], False)
    ok = step_rows(new_engine(), batch, table, [3, 4], False)
    assert status == 8 and same and math.isnan(loss[1]) and report[1].tolist() == [-1, -1, 0, 0] and math.isnan(regret[1])
    assert bits(loss[[0, 2]]).tolist() == bits(ok[0]).tolist() and report[[0, 2]].tolist() == ok[1].tolist() and ok[3] == 0
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    parts = split_blob(g, state_of("random"))
    assert parts[FSCORE_BIAS].tolist() == [0.0]


# ---- 4. it learns -----------------------------------------------------------------------------------------------------------------------
LEARN_LR, LEARN_WD, LEARN_STEPS = 1e-3, 1e-4, 20


@lru_cache(None)
def learn_case():
    batch = make("kwg_mlp", 2, 11)
    return batch, seeded_table(batch.masks.numpy(), 16, 1)


@lru_cache(None)
def twin_losses():
    batch, table = learn_case()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    o = ImitationOracle(state_of("random"), lr=LEARN_LR, wd=LEARN_WD, dtype=torch.float32)
    return [float(o.step(batch.forward_args(), table, 1.0)[0].sum()) for _ in range(LEARN_STEPS + 1)]


def test_the_learning_rate_halves_the_twins_loss():
    """The condition of the device test, on the CPU: with lr 1e-3 the fp32 twin's loss after 20 steps is at most half the first."""
    losses = twin_losses()
    print("twin losses", [round(v, 4) for v in losses])
    assert losses[0] > 0.1 and losses[LEARN_STEPS] <= 0.5 * losses[0]


@pytest.mark.gpu
def test_twenty_steps_halve_the_loss():
    batch, table = learn_case()
    eng = new_engine(lr=LEARN_LR, wd=LEARN_WD)
    losses = [float(eng.imitation_step(batch.forward_args(), table, 1.0)[0].sum()) for _ in range(LEARN_STEPS + 1)]
    twin = twin_losses()
    print("device losses", [round(v, 4) for v in losses])
    assert abs(losses[0] - twin[0]) <= 1e-4 * max(1.0, abs(twin[0]))      # the first step sees the same parameters
    assert losses[LEARN_STEPS] <= 0.5 * losses[0]


# ---- 5. the frontier --------------------------------------------------------------------------------------------------------------------
FR_CANDIDATES, FR_ROUNDS = 8, 4
# The shipped checkpoint's scores lie 5..50 apart and toy_kw's improvements differ by ~0.1: at margin 1 the GNN's order of the eight
# candidates violates nothing in a "gnn" run (loss 0, a step of weight decay alone; the "strong" runs visit states where it does).  The
# "gnn" cases therefore ask for 200 per unit of improvement, so that their steps carry a gradient -- the host loop asserts that they do.
FR_MARGIN = {"gnn": 200.0, "strong": 1.0}
_runs = {}


def quiet(s):
    pass


def frontier_run(K, imitate, branching, rounds=FR_ROUNDS, **kw):
    """``branch_and_bound_frontier`` on toy_kw with a fresh online GraphChoice, traced and audited."""
    from gnn_branching_amd.frontier import branch_and_bound_frontier
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    lp, choice, _ = toy(online=True)
    trace, audit, stats = [], [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=quiet, trace=trace, stats=stats,
                                    strong_candidates=FR_CANDIDATES, strong_audit=audit, branching=branching,
                                    **({} if imitate is None else {"imitate": imitate, "imitate_margin": FR_MARGIN[branching]}), **kw)
    return res, trace, audit, stats, choice


def host_loop(K, rounds, imitate, branching, tables, margin=1.0):
    """The frontier rule as a host loop of public pieces (tests.frontier_twin.twin's plain mode) that learns: per round the K open domains
    of lowest bound, each split at the GNN's decision under the CURRENT parameters ("gnn") or at the table's best candidate ("strong"),
    the children bounded by solve_many(lp="dual_device"), the keep-or-close rule -- and, in every round whose number is a multiple of
    ``imitate``, behind the commit ONE ``ScorerEngine.imitation_step`` on the picked parents' own forward arguments and their tables.
    tables: per round, per picked parent, the audit's row (candidates, improvements, strong_decision): the table is an input here."""
    from gnn_branching_amd import bab_caller, lp_producer
    from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, at_least_the_parents, toy, ub64
    lp, choice, root_mask = toy(online=True)
    eng = choice._eng()
    w_start = eng.get_weights().copy()
    fixed = {"fixed_layers": lp.layers[:-1], "prop_layers": [lp.layers[-1]]}
    n_layers, R = len(lp.layers), sum(int(m.numel()) for m in root_mask)

    def as_sub(d):
        return bab_caller.Subproblem(*d.graph_bounds(lp.pre_relu_indices, n_layers), d.dual_vars, d.ub_point, d.primals, d.mask)

    def children_of(pairs):
        items = []
        for d, dec in pairs:
            for c in (0, 1):
                m = [t.clone() for t in d.mask]
                m[dec[0]][dec[1]] = c
                items.append((m, d, dec[0]))
        return lp.solve_many(items, lp="dual_device", n_iter=N_ITER, lr=LR)

    root = lp.solve_many([(root_mask, None, None)], lp="dual_device", n_iter=N_ITER, lr=LR)[0]
    gub, closed, domains = ub64(lp, root), INF, []

    def keep_or_close(subs, gub, closed):
        for c in subs:
            if c is None:
                continue
            assert abs(c.lb - (gub - EPS_BAB)) > 1e-9, ("the host loop's comparison is within 1e-9 of its threshold", c.lb, gub - EPS_BAB)
            if any(bool((m == -1).any()) for m in c.mask) and c.lb < gub - EPS_BAB:
                domains.append(c)
            else:
                closed = min(closed, c.lb)
        return closed

    def global_lb():
        return min([d.lb for d in domains] + [closed, gub])
    closed = keep_or_close([root], gub, closed)
    out = {k: [] for k in ("decisions", "child_bounds", "loss", "report", "regret", "global_lb", "global_ub")}
    steps = rows = 0
    for r in range(1, rounds + 1):
        if not domains or not gub - global_lb() > EPS_BAB:
            break
        domains.sort(key=lambda d: d.lb)
        assert len({d.lb for d in domains}) == len(domains), "two open bounds are equal at a pick"
        picked, domains[:] = domains[:K], domains[K:]
        subs = [as_sub(d) for d in picked]
        tab = tables[r - 1]
        assert len(tab) == len(picked)
        if branching == "strong":
            decs = [list(a["strong_decision"]) for a in tab]
        else:
            decs = [lp_producer.gnn_scorer(choice, lp)(picked[0], fixed)] if K == 1 else bab_caller.BatchedGraphChoice.decision_many(choice, subs, fixed)
            decs = [[int(d[0]), int(d[1])] for d in decs]
        children = at_least_the_parents(children_of(zip(picked, decs)), [d for d in picked for _ in (0, 1)])
        gub = min([gub] + [ub64(lp, c) for c in children if c is not None])
        closed = keep_or_close(children, gub, closed)       # commit first, then learn
        loss, report, regret = [], [], []
        if r % imitate == 0 and sum(len(a["candidates"]) for a in tab) > 0:
            table = np.full((len(picked), R), NAN)
            for i, a in enumerate(tab):
                table[i, a["candidates"]] = a["improvements"]
            args, _ = bab_caller.collate(subs, fixed)
            loss, report, regret = (v.tolist() for v in eng.imitation_step(args, table, margin))
            steps, rows = steps + 1, rows + len(picked)
        for k, v in (("decisions", decs), ("child_bounds", [INF if c is None else c.lb for c in children]), ("loss", loss), ("report", report),
                     ("regret", regret), ("global_lb", global_lb()), ("global_ub", gub)):
            out[k].append(v)
    out.update(steps=steps, rows=rows, weights=eng.get_weights().copy(), weights_start=w_start)
    return out


def both(K, imitate, branching):
    key = (K, imitate, branching)
    if key not in _runs:
        run = frontier_run(K, imitate, branching)
        rows, tables = iter(run[2]), []
        for t in run[1]:
            tables.append([next(rows) for _ in t["slots"]])
        _runs[key] = (host_loop(K, FR_ROUNDS, imitate, branching, tables, FR_MARGIN[branching]), run)
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("branching", ["gnn", "strong"])
@pytest.mark.parametrize("K,imitate", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_the_frontier_equals_a_host_loop_of_public_pieces(K, imitate, branching):
    from gnn_branching_amd.engine import state_blob
    from tests.frontier_twin import masked
    host, ((glb, gub, rounds, bounded, reason), trace, audit, stats, choice) = both(K, imitate, branching)
    print("host", {k: v for k, v in host.items() if not k.startswith("weights")}, "frontier", (glb, gub, rounds, bounded, reason), stats)
    first = next((r for r, l in enumerate(host["loss"]) if l), None)
    assert first is not None and first + 1 < len(host["decisions"]), "the host loop never decided after a step: the comparison would show nothing"
    assert any(v > 0 for l in host["loss"] for v in l), "no step of the host loop carried a gradient"
    assert len(trace) == len(host["decisions"])
    assert [t["decisions"] for t in trace] == host["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == host["child_bounds"]
    for r, t in enumerate(trace):
        learnt = bool(host["loss"][r])
        assert ("imitation_loss" in t) == learnt, r
        assert learnt == ((r + 1) % imitate == 0)            # (every parent of these runs has candidates)
        assert t["global_lb"] == host["global_lb"][r] and abs(t["global_ub"] - host["global_ub"][r]) <= 1e-9 * max(1.0, abs(host["global_ub"][r]))
        if learnt:
            np.testing.assert_array_equal(bits(t["imitation_loss"]), bits(host["loss"][r]))          # the fp32 losses, bit for bit
            assert t["imitation_report"] == host["report"][r] and same_or_nan(t["imitation_regret"], host["regret"][r])
            assert all(rep[0] >= 0 for rep in t["imitation_report"])                                 # every parent of a learning round had a table
    assert glb == host["global_lb"][-1] and abs(gub - host["global_ub"][-1]) <= 1e-9 * max(1.0, abs(host["global_ub"][-1]))
    assert stats["imitation_steps"] == host["steps"] >= 1 and stats["imitation_rows"] == host["rows"]
    assert host["steps"] == sum(1 for r in range(1, len(trace) + 1) if r % imitate == 0)
    got_w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(got_w), bits(host["weights"]))                                # the final parameters, bit for bit
    assert (bits(host["weights"]) != bits(host["weights_start"])).any()
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(got_w))          # the nn.Module mirrors the device


def profiled_run(K, rounds, branching, **kw):
    """(result, trace, launch names in order, launch counts) of a run with a fresh online GraphChoice."""
    from gnn_branching_amd.frontier import branch_and_bound_frontier
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    lp, choice, _ = toy(online=True)
    eng = choice._eng()
    w0 = eng.get_weights().copy()
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.profile_trace()
        trace = []
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=quiet, trace=trace,
                                        branching=branching, **kw)
        counts = eng.profile_read()
        names = [name for name, _ in eng.profile_trace(1 << 16)]
    finally:
        eng.profile_enable(False)
    return res, trace, names, counts, (bits(eng.get_weights()) != bits(w0)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("branching", ["gnn", "strong"])
def test_imitate_none_is_the_run_without_it(branching):
    """The same results, trace and launch trace whether the keyword is left out or given as None; neither moves a parameter or launches the
    gather of the step."""
    extra = {"strong_candidates": FR_CANDIDATES} if branching == "strong" else {}
    a = profiled_run(3, 2, branching, **extra)
    b = profiled_run(3, 2, branching, imitate=None, imitate_margin=1.0, **extra)
    from tests.frontier_strong_twin import same
    assert same(list(a[0]), list(b[0])) and same(a[1], b[1]) and a[2] == b[2] and len(a[2]) > 10
    assert not a[4] and not b[4] and "k_trows_gather" not in a[2]
    c = profiled_run(3, 2, branching, imitate=1, **extra)
    assert c[4] and c[2].count("k_trows_gather") == c[0][2] >= 1      # one step per learning round, and only there


@pytest.mark.gpu
def test_a_strong_run_that_learns_launches_no_forward_kernel():
    from tests.test_gpu_frontier_babsr import FORWARD_CLASSES
    res, trace, names, counts, moved = profiled_run(3, 2, "strong", imitate=1, strong_candidates=FR_CANDIDATES)
    assert moved and res[2] >= 1 and names.count("k_trows_gather") == res[2]
    for k in FORWARD_CLASSES:
        assert k not in names and counts[k][1] == 0, k


@pytest.mark.gpu
@pytest.mark.parametrize("branching", ["gnn", "strong"])
def test_a_learning_round_copies_nothing_but_the_candidate_count_and_the_state_record(branching):
    """One learning round under torch.cuda.set_sync_debug_mode("error"): the read of cand0[K] and the read of the state record are the two
    exemptions; the step's launches run under the mode (its own stream synchronisation inside the library is not torch's)."""
    from gnn_branching_amd import _lib
    from gnn_branching_amd.frontier import FrontierRun
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    from tests.test_gpu_frontier_online import sync_mode_is_live
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy(online=True)
    run = FrontierRun(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, imitate=1, strong_candidates=FR_CANDIDATES, strong_chunk=3, branching=branching)
    st = run.root()
    if not sync_mode_is_live(run):
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
    before = torch.cuda.get_sync_debug_mode()
    w0 = run.eng.get_weights().copy()
    reads, read_candidates = [], run.read_candidates

    def exempt_read(n):
        with pytest.raises(RuntimeError):
            read_candidates(n)
        torch.cuda.set_sync_debug_mode(before)
        try:
            reads.append(read_candidates(n))
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return reads[-1]
    run.read_candidates = exempt_read
    try:
        torch.cuda.set_sync_debug_mode("error")
        run.launch_round(1, int(st[_lib.FS_IN_USE]))
        with pytest.raises(RuntimeError):
            run.read_state()                                  # the state record: a synchronising copy
        torch.cuda.set_sync_debug_mode(before)
        st = run.pool.state.cpu().tolist()                    # ... exempted by hand
        assert run.imitate_pending and run.learning
        torch.cuda.set_sync_debug_mode("error")
        run._imitate()                                        # no read of its own: the candidate count is the host's copy
        torch.cuda.set_sync_debug_mode(before)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert reads == [FR_CANDIDATES] and run.imitation_steps == 1 and run.imitation_rows == 1 and not run.imitate_pending
    run.check_status()
    assert (bits(run.eng.get_weights()) != bits(w0)).any()


# ---- GraphChoice.imitation_learning -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_choice_imitation_learning_is_one_step_on_the_last_decision():
    """decision, imitation_learning, del_score: the loss and the regret of ``ScorerEngine.imitation_step`` on the decision's arguments, the
    nn.Module mirrors the device afterwards, and without a decision there is nothing to learn from."""
    import os
    from gnn_branching_amd import nets
    from gnn_branching_amd.engine import ScorerEngine, state_blob
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice
    one = make("kwg_mlp", 1, 11)
    table = seeded_table(one.masks.numpy(), 16, 1)
    init_mask = [m[0] for m in one.bab_masks]
    g = GraphChoice(init_mask, os.path.join(nets.ASSETS, "cifar_trained_gnn.npz"), lr=1e-3, wd=1e-4)
    g.verbose = False
    sd0 = {k: v.detach().clone() for k, v in g.model.state_dict().items()}
    w0 = state_blob(sd0)
    d = g.decision(one.lower_bounds_all, one.upper_bounds_all, one.dual_vars, one.primal_inputs, [p.tolist() for p in one.primals], one.layers, init_mask)
    assert d[0] >= 0
    g.imitation_learning(table[0], margin=200.0)
    ref = ScorerEngine(sd0)
    ref.online_create(1e-3, 1e-4)
    loss, report, regret = ref.imitation_step(one.forward_args(), table, 200.0)
    assert bits([g.last_loss]).tolist() == bits(loss).tolist() and g.last_regret == regret[0] and g.last_loss > 0 and report[0, 3] >= 1
    now = state_blob(g.model.state_dict())
    assert bits(now).tolist() == bits(g._eng().get_weights()).tolist() == bits(ref.get_weights()).tolist() and (bits(now) != bits(w0)).any()
    g.del_score()
    with pytest.raises(RuntimeError):
        g.imitation_learning(table[0])
