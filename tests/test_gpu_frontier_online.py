"""Learning online inside the device-resident frontier, on the MI355X (gnn_branching_amd/frontier.py;
csrc/gnnb_k_frontier.h k_frontier_learn; csrc/gnnb_k_train.h k_trows_gather):

1. gnnb_frontier_learn against a Python restatement made of bab_caller.resolve_online and the flat ReLU index, exact, on synthetic rows
   that take every branch of the rule;
2. gnnb_online_step_rows against gnnb_online_step on the same rows picked with torch indexing (a compact B = n batch), bit for bit, the
   device-side guard of a bad index, and the limits;
3. branch_and_bound_frontier(online_threshold=...) on toy_kw against a host loop made of public pieces (the twin of
   tests/frontier_twin.py with resolve_online and ScorerEngine.online_step): K = 1 and K = 4, a threshold that is never
   reached against the plain threshold run, what crosses the link in a round, and soundness."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, frontier, synth
from gnn_branching_amd.bab_caller import resolve_online
from gnn_branching_amd.engine import ScorerEngine, make_batch, state_blob
from gnn_branching_amd.frontier import FrontierRun, branch_and_bound_frontier
from tests.common import KW_ARCHS, register_kw_archs, state_of
from tests.frontier_twin import EPS_BAB, LR, N_ITER, bind, engine, masked, toy, toy_lp0, twin   # noqa: F401  (engine: the module's fixture)

pytestmark = pytest.mark.gpu

S = _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. gnnb_frontier_learn -------------------------------------------------------------------------------------------
# the kinds of row; the first cycle names distinct GNN nodes (but for the pair), so every kind meets the count it was built for
LSEQ = ["unused", "below", "reach", "pair", "pair", "exact", "above", "kw_first", "kw_last", "none", "not_asked", "outside", "reach"]


def learn_rows(relu, K, thr, seed):
    """K parent rows of the kinds of LSEQ (cyclic) and the table they start from, as CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    L, R = len(relu), sum(relu)
    off = [0] + list(np.cumsum(relu))
    gnn_dec, kw_dec = torch.zeros(K, 2, dtype=torch.int32), torch.zeros(K, 2, dtype=torch.int32)
    used = torch.ones(K, dtype=torch.int32)
    gnn_imp = 0.2 + 0.05 * torch.rand(K, generator=g, dtype=torch.float64)
    kw_imp = gnn_imp + torch.where(torch.arange(K) % 2 == 0, 0.05, 0.3)          # used; improve 0 / 1 by the row's parity
    wrong = torch.zeros(R, dtype=torch.int32)
    kinds = [LSEQ[i % len(LSEQ)] for i in range(K)]
    n0 = len(LSEQ) + 2                                     # nodes below it belong to the first cycle
    for i, kind in enumerate(kinds):
        c, first = i % len(LSEQ), i < len(LSEQ)
        lay = c % L
        idx = c + 1 if first else int(torch.randint(n0, relu[lay], (1,), generator=g))
        if kind == "pair" and kinds[i - 1] == "pair":      # the second row of the pair names the first one's node
            lay, idx = int(gnn_dec[i - 1, 0]), int(gnn_dec[i - 1, 1])
        gnn_dec[i, 0], gnn_dec[i, 1] = lay, idx
        kl = (lay + 1) % L
        kw_dec[i, 0], kw_dec[i, 1] = kl, int(torch.randint(0, relu[kl], (1,), generator=g))
        node = off[lay] + idx
        if not first:
            continue
        if kind == "unused":
            kw_imp[i], used[i] = gnn_imp[i] - 0.01, 0
        elif kind in ("below", "pair"):
            wrong[node] = max(thr - 2, 0)
        elif kind in ("reach", "kw_first", "kw_last"):
            wrong[node] = thr - 1
            if kind == "kw_first":
                kw_dec[i, 0], kw_dec[i, 1] = 0, 3
            elif kind == "kw_last":
                kw_dec[i, 0], kw_dec[i, 1] = L - 1, relu[-1] - 1           # the last node: flat index R - 1
        elif kind == "exact":                              # 0.2 - 0.1 is 0.1 in fp64: not greater
            wrong[node], gnn_imp[i], kw_imp[i] = thr - 1, 0.1, 0.2
        elif kind == "above":
            wrong[node], gnn_imp[i], kw_imp[i] = thr - 1, 0.1, math.nextafter(0.2, 1.0)
        elif kind == "none":
            gnn_dec[i, 0], gnn_dec[i, 1] = -1, -1
        elif kind == "not_asked":
            kw_dec[i, 0], kw_dec[i, 1], kw_imp[i], used[i] = -1, -1, -1.0, 0
        elif kind == "outside":                            # one past the layer's last node: the next layer's first flat index, or R
            gnn_dec[i, 1] = relu[lay]
    return {"gnn_dec": gnn_dec, "kw_dec": kw_dec, "used": used, "gnn_imp": gnn_imp, "kw_imp": kw_imp, "wrong": wrong, "kinds": kinds}


def learn_reference(relu, rows, idx, wrong, thr):
    """The walk of an online round's step 2 over the rows ``idx`` from the table ``wrong``, restated with resolve_online and the flat
    index.  Returns ([(position, flat KW index, improve)], the table afterwards, per row (count after, learn) or None)."""
    off = [0] + list(np.cumsum(relu))

    def flat(d):
        return off[d[0]] + d[1] if 0 <= d[0] < len(relu) and 0 <= d[1] < relu[d[0]] else None
    w, out, seen = wrong.clone(), [], []
    for pos, i in enumerate(idx):
        gd, kd = rows["gnn_dec"][i].tolist(), rows["kw_dec"][i].tolist()
        seen.append(None)
        if not int(rows["used"][i]) or flat(gd) is None or flat(kd) is None:
            continue
        key = f"{gd[0]}-{gd[1]}"
        table = {key: int(w[flat(gd)])}
        dec, used, learn, improve = resolve_online(gd, float(rows["gnn_imp"][i]), kd, float(rows["kw_imp"][i]), table, thr)
        assert used and dec == kd                          # the row is consistent: used_kw is resolve_online's own choice
        w[flat(gd)] = table[key]
        seen[-1] = (table[key], learn, improve)
        if learn:
            out.append((pos, flat(kd), float(improve)))
    return out, w, seen


def run_learn(engine, rows, idx, wrong, thr):
    dev, K, i32 = engine.device, len(idx), torch.int32
    ix = torch.tensor(idx)
    out = {"rows": torch.full((K,), -7, dtype=i32, device=dev), "kw": torch.full((K,), -7, dtype=i32, device=dev),
           "imp": torch.full((K,), -7.0, dtype=torch.float32, device=dev), "n": torch.full((1,), -7, dtype=i32, device=dev), "wrong": wrong.to(dev)}
    engine.frontier_learn(K, rows["gnn_dec"][ix].contiguous().to(dev), rows["kw_dec"][ix].contiguous().to(dev), rows["used"][ix].contiguous().to(dev),
                          rows["gnn_imp"][ix].contiguous().to(dev), rows["kw_imp"][ix].contiguous().to(dev), thr, out["wrong"], out["rows"], out["kw"],
                          out["imp"], out["n"])
    return {k: v.cpu() for k, v in out.items()}


def assert_learn(got, want, what):
    lst, table, _ = want
    n = int(got["n"][0])
    assert n == len(lst), (what, n, lst)
    assert got["rows"][:n].tolist() == [p for p, _, _ in lst] and got["kw"][:n].tolist() == [k for _, k, _ in lst], what
    assert got["imp"][:n].tolist() == [v for _, _, v in lst], what                  # fp32 0.0 / 1.0, exactly
    assert got["rows"][n:].tolist() == [-7] * (len(got["rows"]) - n) and got["kw"][n:].tolist() == [-7] * (len(got["kw"]) - n), what
    assert got["imp"][n:].tolist() == [-7.0] * (len(got["imp"]) - n), what          # nothing beyond n_learn is written
    assert torch.equal(got["wrong"], table), what


@pytest.mark.parametrize("thr", [1, 5])
@pytest.mark.parametrize("K", [1, 3, 130])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_learn_against_the_restatement(name, K, thr, engine):
    """Every branch of the rule (the kinds of LSEQ) from a preloaded table, compared exactly: the dense lists, n_learn, the fp32 improve,
    the table afterwards, the poison beyond n_learn.  K = 130: ten cycles, the later ones on random nodes (counts carried between rows
    that meet).  Then the rows of the first cycle alone (K = 1 calls), each from the table the restatement had before it."""
    relu = bind(engine, name)
    rows = learn_rows(relu, K, thr, 40 + K)
    idx = list(range(K))
    want = learn_reference(relu, rows, idx, rows["wrong"], thr)
    got = run_learn(engine, rows, idx, rows["wrong"], thr)
    print(name, K, thr, "n_learn", int(got["n"][0]), "rows", got["rows"].tolist()[:16], "kw", got["kw"].tolist()[:16], "improve", got["imp"].tolist()[:16])
    assert_learn(got, want, (name, K, thr))
    if K < 130:
        return
    by = {}
    for kind, s in zip(rows["kinds"][:len(LSEQ)], want[2][:len(LSEQ)]):
        by.setdefault(kind, []).append(s)
    off = [0] + list(np.cumsum(relu))
    first = {p: (kw, imp) for p, kw, imp in want[0] if p < len(LSEQ)}
    pos = {kind: rows["kinds"].index(kind) for kind in LSEQ}
    assert by["unused"] == [None] and by["none"] == [None] and by["not_asked"] == [None] and by["outside"] == [None]
    assert all(s is not None and s[0] == thr and s[1] for s in by["reach"])         # the count reaches the threshold at this row
    assert by["pair"][1][0] == by["pair"][0][0] + 1 and by["pair"][1][1]            # both rows count; the second one crosses (thr 1: both)
    assert first[pos["exact"]][1] == 0.0 and first[pos["above"]][1] == 1.0          # exactly 0.1 is not greater
    assert first[pos["kw_first"]][0] == 3 and first[pos["kw_last"]][0] == sum(relu) - 1 and off[-2] > 3
    if thr > 1:
        assert by["below"][0][:2] == (thr - 1, False) and by["pair"][0][:2] == (thr - 1, False)
    assert {0.0, 1.0} == {imp for _, _, imp in want[0]}
    state, singles = rows["wrong"], []
    for i in range(len(LSEQ)):                             # alone, from the same table: the same row results
        w1 = learn_reference(relu, rows, [i], state, thr)
        g1 = run_learn(engine, rows, [i], state, thr)
        assert_learn(g1, w1, (name, "alone", i, rows["kinds"][i]))
        singles += [(i, kw, imp) for _, kw, imp in w1[0]]
        state = w1[1]
    assert singles == [e for e in want[0] if e[0] < len(LSEQ)]


def test_learn_limits(engine):
    """An unbound handle is GNNB_E_STATE; online_threshold < 1 and a null array GNNB_E_INVALID -- each with a message naming the entry point."""
    fresh = ScorerEngine(None)
    assert fresh.lib.gnnb_frontier_learn(fresh.h, 1, *([None] * 5), 1, *([None] * 5), None) == -3
    assert b"gnnb_frontier_learn" in fresh.lib.gnnb_last_error() and b"gnnb_bind_network first" in fresh.lib.gnnb_last_error()
    relu = bind(engine, "kwg_mlp")
    rows = learn_rows(relu, 2, 1, 3)
    for thr in (0, -4):
        with pytest.raises(RuntimeError, match=r"gnnb_frontier_learn failed \(-1\).*online_threshold"):
            run_learn(engine, rows, [0, 1], rows["wrong"], thr)
    assert engine.lib.gnnb_frontier_learn(engine.h, 2, *([None] * 5), 1, *([None] * 5), None) == -1
    assert b"gnnb_frontier_learn: null argument" in engine.lib.gnnb_last_error()
    assert_learn(run_learn(engine, rows, [0, 1], rows["wrong"], 1), learn_reference(relu, rows, [0, 1], rows["wrong"], 1), "usable")


# ---- 2. gnnb_online_step_rows -----------------------------------------------------------------------------------------
PROPS = [(3, 5), (1, 7), (0, 2), (8, 4), (6, 9)]
KB = 5


def middle_kw(masks):
    """A scored node from the middle of every sample's mask, as a flat index."""
    out = []
    for b in range(masks.shape[0]):
        idx = masks[b].nonzero().view(-1)
        out.append(int(idx[len(idx) // 2]))
    return out


_batches = {}


def batch_of(name):
    if name not in _batches:
        register_kw_archs()
        _batches[name] = synth.make_batch(name, KB, seed=17, props=PROPS, input_shape=KW_ARCHS[name][0])
    return _batches[name]


def compact_args(batch, rows):
    """The rows ``rows`` of ``batch`` as a batch of their own, in list order: torch indexing on every tensor."""
    B, ix = batch.batch_size, torch.tensor(rows)

    def flat(t):
        return t.reshape(B, -1)[ix]
    return ([t[ix] for t in batch.lower_bounds_all], [t[ix] for t in batch.upper_bounds_all], [flat(t).reshape(-1, 3) for t in batch.dual_vars],
            [flat(t).reshape(-1) for t in batch.primals], batch.primal_inputs[ix],
            {"fixed_layers": batch.layers["fixed_layers"], "prop_layers": [batch.layers["prop_layers"][r] for r in rows]}, batch.masks[ix])


class DeviceBatch:
    """A K-row batch marshalled to the device on an engine with an optimizer, as gnnb_online_step_rows reads it."""

    def __init__(self, batch):
        self.eng = ScorerEngine(state_of("random"))
        self.eng.online_create(lr=1e-2)
        self.m = self.eng._marshal(*batch.forward_args())
        self.cb, self.keep = make_batch(self.m.lbs, self.m.ubs, self.m.duals, self.m.prim, self.m.x_lp, self.m.mask, self.m.pw, self.m.pb)
        self.tensors = [*self.m.lbs, *self.m.ubs, *self.m.duals, *self.m.prim, self.m.x_lp, self.m.mask, self.m.pw, self.m.pb]
        self.before = [t.clone() for t in self.tensors]

    def step(self, rows, kws, imps, apply):
        dev = self.eng.device
        n = len(rows)
        loss = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.eng.online_step_rows(self.cb, KB, torch.tensor(rows, dtype=torch.int32).to(dev), torch.tensor(kws, dtype=torch.int32).to(dev),
                                  torch.tensor(imps, dtype=torch.float32).to(dev), loss=loss, status=status, apply=apply)
        return loss.cpu().numpy(), int(status.cpu()[0])

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.tensors, self.before))


def reference_step(batch, rows, kws, imps, apply):
    eng = ScorerEngine(state_of("random"))
    eng.online_create(lr=1e-2)
    loss, _ = eng.online_step(compact_args(batch, rows), kws, imps, apply=apply)
    return loss, eng.online_grad(), eng.get_weights()


@pytest.mark.parametrize("rows", [[3], [3, 0, 4], [0, 1, 2, 3, 4]])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_step_rows_is_online_step_on_the_picked_rows(name, rows):
    """Loss, gradient and (apply = 1) the parameters after the Adam step, bit for bit: the gather is a copy and the tape behind it the same
    kernels at the same B.  The K-row source batch is not written."""
    batch = batch_of(name)
    kws = middle_kw(batch.masks[torch.tensor(rows)])
    imps = [(0.0, 1.0, 0.25)[i % 3] for i in range(len(rows))]
    for apply in (False, True):
        want_loss, want_g, want_w = reference_step(batch, rows, kws, imps, apply)
        d = DeviceBatch(batch)
        w0 = d.eng.get_weights()
        loss, status = d.step(rows, kws, imps, apply)
        print(name, rows, "apply", apply, "loss", loss.tolist(), "reference", want_loss.tolist(), "status", status)
        assert status == 0
        np.testing.assert_array_equal(bits(loss), bits(want_loss))
        np.testing.assert_array_equal(bits(d.eng.online_grad()), bits(want_g))
        np.testing.assert_array_equal(bits(d.eng.get_weights()), bits(want_w))
        assert np.isfinite(loss).all() and float(np.abs(want_g).max()) > 0
        assert (bits(d.eng.get_weights()) != bits(w0)).any() == apply
        assert d.unchanged()


@pytest.mark.parametrize("bad", ["decided", "past_R", "negative", "row_outside"])
@pytest.mark.parametrize("name", ["kwg_mlp", "kwg_rect"])
def test_step_rows_guards_a_device_fed_index(name, bad):
    """n = 2 and row 1 names a decided node, an index >= R or < 0, or no row of the batch: status 8, loss[1] NaN, and -- as for the
    empty-mask sample of tests/test_online_gradients.py -- loss[0] and the gradient bit-equal to row 0 stepped alone."""
    batch = batch_of(name)
    rows, R = [3, 1], batch.masks.shape[1]
    kws = middle_kw(batch.masks[torch.tensor(rows)])
    if bad == "decided":
        kws[1] = int((batch.masks[rows[1]] == 0).nonzero().view(-1)[0])
    elif bad == "past_R":
        kws[1] = R + 5
    elif bad == "negative":
        kws[1] = -1
    else:
        rows = [3, KB + 2]
    want_loss, want_g, _ = reference_step(batch, rows[:1], kws[:1], [0.1], False)
    d = DeviceBatch(batch)
    loss, status = d.step(rows, kws, [0.1, 0.2], False)
    print(name, bad, "loss", loss.tolist(), "status", status)
    assert status == 8 and np.isnan(loss[1])
    np.testing.assert_array_equal(bits(loss[:1]), bits(want_loss))
    np.testing.assert_array_equal(bits(d.eng.online_grad()), bits(want_g))
    assert d.unchanged()
    loss, status = d.step(rows[:1], kws[:1], [0.1], False)            # the handle stays usable, and the status is the caller's to zero
    assert status == 0
    np.testing.assert_array_equal(bits(loss), bits(want_loss))


def test_step_rows_limits():
    """n = 0 and n > K are GNNB_E_INVALID, a call before gnnb_online_create GNNB_E_STATE, each naming the entry point."""
    batch = batch_of("kwg_mlp")
    d = DeviceBatch(batch)
    dev = d.eng.device
    r = torch.zeros(KB + 1, dtype=torch.int32, device=dev)
    f = torch.zeros(KB + 1, dtype=torch.float32, device=dev)
    for n in (0, KB + 1):
        assert d.eng.lib.gnnb_online_step_rows(d.eng.h, C.byref(d.cb), KB, r.data_ptr(), n, r.data_ptr(), f.data_ptr(), None, None, 0, None) == -1
        assert f"gnnb_online_step_rows: n = {n}".encode() in d.eng.lib.gnnb_last_error()
    assert d.eng.lib.gnnb_online_step_rows(d.eng.h, C.byref(d.cb), KB, None, 1, r.data_ptr(), f.data_ptr(), None, None, 0, None) == -1
    assert b"gnnb_online_step_rows: null argument" in d.eng.lib.gnnb_last_error()
    fresh = ScorerEngine(state_of("random"))
    m = fresh._marshal(*batch.forward_args())
    cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
    assert fresh.lib.gnnb_online_step_rows(fresh.h, C.byref(cb), KB, r.data_ptr(), 1, r.data_ptr(), f.data_ptr(), None, None, 0, None) == -3
    assert b"gnnb_online_step_rows" in fresh.lib.gnnb_last_error() and b"gnnb_online_create first" in fresh.lib.gnnb_last_error()
    with pytest.raises(RuntimeError, match="online_create"):
        fresh.online_step_rows(cb, KB, r[:1], r[:1], f[:1])


# ---- 3. the loop on toy_kw against a host loop of public pieces -------------------------------------------------------
_shared = {}


def frontier_online(K, rounds, online_threshold, threshold=1.0):
    lp, choice, _ = toy(online=True)
    trace, stats = [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace,
                                    branching_threshold=threshold, stats=stats, online_threshold=online_threshold)
    return res, trace, stats, choice


def runs(K, rounds, online_threshold):
    key = (K, rounds, online_threshold)
    if key not in _shared:
        _shared[key] = (twin(K, rounds, 1.0, online_threshold=online_threshold), frontier_online(K, rounds, online_threshold))
    return _shared[key]


def learned_then_decided(twin):
    """The twin took a learning step in some round and picked parents in a later one: a decision was made with learned parameters."""
    first = next((r for r, rows in enumerate(twin["learn_rows"]) if rows), None)
    return first is not None and first + 1 < len(twin["decisions"])


def assert_same_run(twin, run):
    (glb, gub, rounds, bounded, reason), trace, stats, choice = run
    print("twin", {k: v for k, v in twin.items() if not k.startswith("weights")}, "frontier", (glb, gub, rounds, bounded, reason), stats)
    for t in trace:
        print("round", {k: t[k] for k in ("gnn_decisions", "gnn_improvement", "kw_decisions", "kw_improvement", "used_kw", "decisions", "learn_rows",
                                          "learn_kw", "learn_improve", "loss", "global_lb", "global_ub")})
    assert learned_then_decided(twin), "the twin never decided with learned parameters: the comparison would show nothing"
    assert len(trace) == len(twin["decisions"])
    for key in ("decisions", "gnn_decisions", "kw_decisions", "used_kw", "selected", "learn_rows", "learn_kw", "learn_improve"):
        assert [t[key] for t in trace] == twin[key], key
    assert [t["gnn_improvement"] for t in trace] == twin["gnn_improvement"]               # Python floats of the same fp64 values
    assert [t["kw_improvement"] for t in trace] == twin["kw_improvement"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == twin["child_bounds"]
    for t, want in zip(trace, twin["loss"]):                                              # the fp32 losses, bit for bit
        np.testing.assert_array_equal(bits(t["loss"]), bits(want))
    assert [t["global_lb"] for t in trace] == twin["global_lb"] and glb == twin["global_lb"][-1]
    for t, want in zip(trace, twin["global_ub"]):
        assert abs(t["global_ub"] - want) <= 1e-9 * max(1.0, abs(want))
    assert stats["online_steps"] == twin["steps"] >= 1 and stats["online_rows"] == sum(len(r) for r in twin["learn_rows"])
    assert stats["kw_bounded"] == sum(len(s) for s in twin["selected"]) and stats["kw_used"] == sum(sum(u) for u in twin["used_kw"])
    got_w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(got_w), bits(twin["weights"]))                    # the final parameters, bit for bit
    assert (bits(twin["weights"]) != bits(twin["weights_start"])).any()
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(got_w))          # the nn.Module mirrors the device


# Source: the online twin ALONE on the MI355X, online_threshold = 1 and branching_threshold = 1.0 on toy_kw's property (2, 6) at eps 0.04, 12
# rounds.  The root parent's KW pair wins in round 1 at either K, so the fewest rounds after which the twin has taken a learning step and
# picked parents again (learned_then_decided, asserted again by every test) is 2.  The tests run a few more, for what 2 rounds cannot hold:
# K = 1 four rounds as tests/test_gpu_frontier_threshold.py (a second Adam step: the moments and the bias correction carried over); K = 4
# five rounds (the twin's rounds 4 and 5 learn from three and four rows at once: the summed loss of a K > 1 round; rounds 2 and 3 have
# m > 0 and no learn row).
ROUNDS_K1 = 4
ROUNDS_K4 = 5


def test_k1_equals_the_host_loop():
    """K = 1, branching_threshold = 1.0 (every parent with a negative bound asks BaBSR), online_threshold = 1 (every KW pair taken is a
    learn row): branch_and_bound_online's control flow on solve_many(lp="dual_device") children."""
    twin, run = runs(1, ROUNDS_K1, 1)
    assert_same_run(twin, run)


def test_k4_equals_the_round_wise_twin():
    """K = 4: one step per round on the summed loss of its learn rows, all scored with the round's opening parameters."""
    twin, run = runs(4, ROUNDS_K4, 1)
    assert_same_run(twin, run)
    assert max(len(r) for r in twin["learn_rows"]) >= 3 and any(s and not r for s, r in zip(twin["selected"], twin["learn_rows"]))


def test_a_threshold_never_reached_is_the_threshold_run_with_every_kw_point_bounded(monkeypatch):
    """online_threshold = 2^30: bounds, decisions and counts of the branching_threshold = 1.0, kwbd_threshold = 2^31 - 1 run bit for bit,
    the parameters untouched, no step, and ``wrong`` the per-node sum of the trace's used_kw."""
    made = []

    class Spy(FrontierRun):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(frontier, "FrontierRun", Spy)
    lp, choice, root_mask = toy(online=True)
    w0 = choice._eng().get_weights().copy()
    ref_trace, ref_stats = [], {}
    ref = branch_and_bound_frontier(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=4, log=lambda s: None, trace=ref_trace,
                                    branching_threshold=1.0, kwbd_threshold=2 ** 31 - 1, stats=ref_stats)
    trace, stats = [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=4, log=lambda s: None, trace=trace,
                                    branching_threshold=1.0, stats=stats, online_threshold=2 ** 30)
    assert res == ref and len(trace) == len(ref_trace) >= 2
    for a, b in zip(trace, ref_trace):
        for key in b:
            assert a[key] == b[key], key
        assert a["learn_rows"] == [] and a["loss"] == []
    assert stats["online_steps"] == 0 and stats["online_rows"] == 0
    assert {k: v for k, v in stats.items() if not k.startswith("online")} == ref_stats and ref_stats["kw_used"] >= 1
    np.testing.assert_array_equal(bits(choice._eng().get_weights()), bits(w0))
    relu = [int(m.numel()) for m in root_mask]
    off = [0] + list(np.cumsum(relu))
    want = torch.zeros(sum(relu), dtype=torch.int32)
    for t in trace:
        for d, u in zip(t["gnn_decisions"], t["used_kw"]):
            if u:
                want[off[d[0]] + d[1]] += 1
    assert int(want.sum()) == ref_stats["kw_used"] and torch.equal(made[-1].wrong.cpu(), want)
    assert made[0].online is None and not hasattr(made[0], "wrong")


@pytest.mark.parametrize("K", [1, 4])
def test_soundness(K):
    """As test_soundness of tests/test_gpu_frontier_threshold.py: global_lb <= global_ub, and global_lb at most the network's minimum
    over 256 sampled points of the box + 1e-5."""
    _, ((glb, gub, *_), _, _, _) = runs(K, ROUNDS_K1 if K == 1 else ROUNDS_K4, 1)
    lp0 = toy_lp0()
    assert glb <= gub
    with torch.no_grad():
        x = lp0.input_lb.float() + (lp0.input_ub - lp0.input_lb).float() * torch.rand((256,) + lp0.shapes[0], generator=torch.Generator().manual_seed(0))
        for l in lp0.layers:
            x = l(x)
    assert glb <= float(x.min()) + 1e-5


def sync_mode_is_live(run):
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run.pool.state.cpu()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(before)


def exempting(read, before, reads):
    """``read`` (a synchronising copy of a few bytes) as an explicit exemption from the "error" mode, which must be live around it."""
    def wrapped():
        with pytest.raises(RuntimeError):
            read()
        torch.cuda.set_sync_debug_mode(before)
        try:
            reads.append(read())
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return reads[-1]
    return wrapped


def test_an_online_round_copies_nothing_but_m_the_state_record_and_n_learn():
    """Two rounds under torch.cuda.set_sync_debug_mode("error"): the read of m, the state record and -- in a round with m > 0 -- the read
    of n_learn are the exemptions; everything else of the learning half (the launch of the step included, whose own stream
    synchronisation inside the library is the fourth) runs under the mode.  Then a round of a run whose threshold nobody is below: m = 0,
    nothing is pending behind the state record and n_learn is not read."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    before = torch.cuda.get_sync_debug_mode()
    for threshold in (1.0, 1e-300):
        lp, choice, _ = toy(online=True)
        run = FrontierRun(lp, choice, lp.layers, K=4, n_iter=N_ITER, lr=LR, eps=EPS_BAB, branching_threshold=threshold, online_threshold=1)
        st = run.root()
        if not sync_mode_is_live(run):
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
        ms, learns = [], []
        run.read_selected = exempting(run.read_selected, before, ms)
        run.read_learn = exempting(run.read_learn, before, learns)
        try:
            for _ in range(2):
                n_open, in_use = int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
                assert n_open >= 1
                torch.cuda.set_sync_debug_mode("error")
                run.launch_round(min(4, n_open), in_use)
                with pytest.raises(RuntimeError):
                    run.read_state()                       # the state record: a synchronising copy
                torch.cuda.set_sync_debug_mode(before)
                st = run.pool.state.cpu().tolist()         # ... exempted by hand
                assert run.learn_pending == (ms[-1] > 0)
                n_reads = len(learns)
                if run.learn_pending:
                    torch.cuda.set_sync_debug_mode("error")
                    run._learn()                           # the read of n_learn exempted inside; the step's launches run under the mode
                    torch.cuda.set_sync_debug_mode(before)
                assert len(learns) == n_reads + (ms[-1] > 0) and not run.learn_pending
        finally:
            torch.cuda.set_sync_debug_mode(before)
        if threshold == 1.0:
            assert len(ms) == 2 and max(ms) >= 1 and len(learns) >= 1 and run.online_steps == sum(n > 0 for n in learns) >= 1
        else:
            assert ms == [0, 0] and learns == [] and run.online_steps == 0
        run.check_status()
