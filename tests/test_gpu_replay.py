"""The replay buffer on the MI355X (csrc/gnnb_k_replay.h, gnn_branching_amd/frontier.py ReplayBuffer / Replay,
gnn_branching_amd/replay.py).  Every comparison is exact -- torch indexing for the copies, tests/replay_twin.py for the ring and the
draws, fp32 bits for losses, gradients and parameters -- but global_ub, within 1e-9 max(1, |ub|) as tests/test_gpu_imitation.py has it.

1. gnnb_replay_push against torch indexing and the rule; 2. gnnb_replay_sample against the restatement; 3. a step from the buffer is the
step on the source rows; 4. save / load / split; 5. ``imitate=Replay(...)`` in the frontier against a host loop of public pieces that
keeps a Python ring; 6. collection only; 7. the reads of a learning round; 8. many jobs; 9. ``train_epochs``."""
import math
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from gnn_branching_amd import nets, synth
from gnn_branching_amd.frontier import Replay, ReplayBuffer
from tests import replay_twin as twin
from tests.common import state_of
from tests.imitation_twin import NAN, ImitationOracle, seeded_table
from tests.test_gpu_imitation import FR_CANDIDATES, FR_MARGIN, FR_ROUNDS, bits, device_batch, make, new_engine, quiet, same_or_nan, step_rows, take
from tests.test_online_gradients import PROPS

I32, F32, F64 = torch.int32, torch.float32, torch.float64
# layer widths and R = 37 + 21 = 58 that are no multiples of 4: k_replay_store's scalar copies (its 16-byte copies take the input layer's
# 192 floats and the table's 2 R); kwg_mlp (64 + 48 = 112) runs the 16-byte copies everywhere
ODD_NET, ODD_SHAPE = "rp_odd", (3, 8, 8)
ODD_SPEC = [("flatten",), ("linear", 192, 37), ("relu",), ("linear", 37, 21), ("relu",), ("linear", 21, 10)]
NETS = ["kwg_mlp", ODD_NET]


def batch_of(net, B, seed):
    if net != ODD_NET:
        return make(net, B, seed)
    nets.register_arch(ODD_NET, ODD_SPEC, seed=900)
    return synth.make_batch(ODD_NET, B, seed=seed, props=[PROPS[b % len(PROPS)] for b in range(B)], input_shape=ODD_SHAPE)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def src_rows(buf, m, tab, K):
    """The source batch's tensors as (K, w) views, in the order of ``buf.row_tensors()``."""
    prims = [t for t, rows in zip(m.prim, buf.prim_rows) if rows]
    return [t.reshape(K, -1) for t in list(m.lbs) + list(m.ubs) + list(m.duals) + prims + [m.x_lp, m.pw, m.pb, m.mask, tab]]


def poison(buf):
    for t in buf.row_tensors():
        t.fill_(NAN)


def all_nan(t):
    return bool(torch.isnan(t).all())


def push(eng, buf, cb, K, rows, tab):
    status = torch.zeros(1, dtype=I32, device=eng.device)
    buf.push(cb, K, torch.tensor(rows, dtype=I32).to(eng.device), len(rows), tab, status=status)
    return int(status.cpu()[0])


# ---- 1. the push ------------------------------------------------------------------------------------------------------------------------
def crafted_table(masks, case):
    """K = 5 rows with 0, 1, 2, every and 2 candidates; "decided": row 4 names a decided node too; "inf": row 3 holds a +inf."""
    masks = np.asarray(masks)
    tab = np.full(masks.shape, NAN)
    g = np.random.RandomState(3)
    und = [np.flatnonzero(masks[b]) for b in range(5)]
    assert all(len(u) >= 3 for u in und)
    tab[1, und[1][1]] = 0.25
    tab[2, und[2][[0, -1]]] = [0.5, 0.125]
    tab[3, und[3]] = g.uniform(0.0, 1.0, len(und[3]))
    tab[4, und[4][[1, 2]]] = [0.75, 0.5]
    if case == "decided":
        dec = np.flatnonzero(masks[4] == 0)
        assert len(dec) >= 1
        tab[4, dec[0]] = 0.3
    if case == "inf":
        tab[3, und[3][1]] = math.inf
    return tab


PUSH_CASES = {"plain": [0, 1, 2, 3, 4], "decided": [0, 1, 2, 3, 4], "inf": [4, 3, 2, 1, 0], "outside": [2, 9, 3, -1, 4], "one": [3], "twice": [3, 2, 3]}


@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("case", list(PUSH_CASES))
def test_push_against_torch_indexing_and_the_rule(net, case):
    K, C, rows = 5, 7, PUSH_CASES[case]
    batch = batch_of(net, K, 21)
    eng = new_engine()
    cb, (m, keep) = device_batch(eng, batch)
    tab_h = crafted_table(batch.masks.numpy(), case)
    tab = torch.from_numpy(tab_h).to(eng.device)
    buf = ReplayBuffer(eng, C)
    assert sum(t.numel() * t.element_size() for t in buf.row_tensors()) == eng.replay_bytes(C) > 0
    poison(buf)
    buf.state.copy_(torch.tensor([5, 1, 0, 0], dtype=I32))     # head 5 of 7: three stored rows wrap
    src = src_rows(buf, m, tab, K)
    before = [t.clone() for t in src]
    status = push(eng, buf, cb, K, rows, tab)
    slots, state, want_status = twin.push(tab_h, batch.masks.numpy(), rows, K, C, [5, 1, 0, 0])
    assert buf.read_state() == state and status == want_status
    assert (status == 8) == (case in ("decided", "inf", "outside"))
    assert state[2] == {"plain": 3, "decided": 2, "inf": 2, "outside": 3, "one": 1, "twice": 3}[case]
    stored = {s: r for s, r in zip(slots, rows) if s >= 0}
    for t, s in zip(buf.row_tensors(), src):
        for slot in range(C):
            if slot in stored:
                assert same_bits(t[slot], s[stored[slot]]), (slot, tuple(t.shape))
            else:
                assert all_nan(t[slot]), (slot, tuple(t.shape))                    # no other slot was written
    assert all(same_bits(a, b) for a, b in zip(before, src))                       # the source is not written


@pytest.mark.gpu
def test_push_of_a_one_row_batch_and_what_it_refuses():
    batch = batch_of("kwg_mlp", 1, 4)
    eng = new_engine()
    cb, (m, keep) = device_batch(eng, batch)
    tab_h = seeded_table(batch.masks.numpy(), 4, 1)
    tab = torch.from_numpy(tab_h).to(eng.device)
    buf = ReplayBuffer(eng, 1)
    poison(buf)
    assert push(eng, buf, cb, 1, [0], tab) == 0 and buf.read_state() == [0, 1, 1, 0]
    for t, s in zip(buf.row_tensors(), src_rows(buf, m, tab, 1)):
        assert same_bits(t, s)
    lib, E_INVALID, E_STATE = eng.lib, -1, -3
    with pytest.raises(RuntimeError, match="gnnb_replay_push: n = 2 rows of a batch of K = 1 into C = 1"):
        buf.push(cb, 1, torch.zeros(2, dtype=I32, device=eng.device), 2, tab)
    import ctypes as C
    rows = torch.zeros(1, dtype=I32, device=eng.device)
    args = [C.byref(cb), 1, tab.data_ptr(), rows.data_ptr(), 1, C.byref(buf.batch), 1, buf.table.data_ptr(), buf.state.data_ptr(), None, None]
    for hole in (0, 2, 3, 5, 7, 8):                             # every argument but status and the stream
        a = list(args)
        a[hole] = None
        assert lib.gnnb_replay_push(eng.h, *a) == E_INVALID and b"gnnb_replay_push: null argument" in lib.gnnb_last_error(), hole
    assert lib.gnnb_replay_sample(eng.h, None, 1, 1, 0, 0, rows.data_ptr(), None) == E_INVALID and b"null argument" in lib.gnnb_last_error()
    from gnn_branching_amd import _lib
    short = _lib.Batch(cb.lb, cb.ub, cb.dual, cb.primal, cb.x_lp, cb.prop_w, cb.prop_b, None, cb.n_graph, cb.n_relu, cb.n_primal)
    a = list(args)
    a[0] = C.byref(short)
    assert lib.gnnb_replay_push(eng.h, *a) == E_INVALID and b"gnnb_replay_push: the batch does not match" in lib.gnnb_last_error()
    from gnn_branching_amd.engine import ScorerEngine
    bare = ScorerEngine(None)
    assert lib.gnnb_replay_push(bare.h, *args) == E_STATE and b"gnnb_replay_push: call gnnb_bind_network first" in lib.gnnb_last_error()
    assert bare.replay_bytes(4) == 0 and buf.read_state() == [0, 1, 1, 0]


@pytest.mark.gpu
def test_the_ring_wraps_and_a_collecting_handle_needs_no_trainer():
    from gnn_branching_amd.engine import ScorerEngine
    K, C = 5, 4
    batch = batch_of("kwg_mlp", K, 21)
    eng = ScorerEngine(state_of("random"))                     # no gnnb_online_create
    cb, (m, keep) = device_batch(eng, batch)
    tab_h = seeded_table(batch.masks.numpy(), 6, 2)
    tab = torch.from_numpy(tab_h).to(eng.device)
    buf = ReplayBuffer(eng, C)
    src = src_rows(buf, m, tab, K)
    assert push(eng, buf, cb, K, [0, 1, 2], tab) == 0 and buf.read_state() == [3, 3, 3, 0] and buf.order() == [0, 1, 2]
    assert push(eng, buf, cb, K, [3, 4, 0], tab) == 0 and buf.read_state() == [2, 4, 3, 0] and buf.order() == [2, 3, 0, 1]
    holds = {0: 4, 1: 0, 2: 2, 3: 3}                           # slot -> source row: rows 0 and 1 of the first push were overwritten
    for t, s in zip(buf.row_tensors(), src):
        for slot, r in holds.items():
            assert same_bits(t[slot], s[r]), slot
    assert not getattr(eng, "_online", False)


@pytest.mark.gpu
def test_rows_pushed_alone_equal_the_same_rows_within_a_longer_list():
    K, C = 5, 6
    batch = batch_of(ODD_NET, K, 8)
    eng = new_engine()
    cb, (m, keep) = device_batch(eng, batch)
    tab_h = crafted_table(batch.masks.numpy(), "plain")
    tab = torch.from_numpy(tab_h).to(eng.device)
    a, b = ReplayBuffer(eng, C), ReplayBuffer(eng, C)
    poison(a), poison(b)
    assert push(eng, a, cb, K, [3, 4], tab) == 0 and push(eng, b, cb, K, [0, 3, 1, 4], tab) == 0
    assert a.read_state() == [2, 2, 2, 0] and b.read_state() == [2, 2, 2, 2]
    for x, y in zip(a.row_tensors(), b.row_tensors()):
        assert same_bits(x[:2], y[:2]) and all_nan(x[2:]) and all_nan(y[2:])


# ---- 2. the sampler ---------------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(1, 1), (2, 2), (5, 3), (5, 5), (300, 256), (65536, 256), (0, 3), (3, 8), (1000, 1), (64, 16)]      # (filled, n)


@pytest.mark.gpu
@pytest.mark.parametrize("filled,n", SAMPLE_CASES)
def test_the_device_draw_equals_the_restatement(filled, n):
    eng = new_engine()
    dev, C = eng.device, 65536
    state = torch.tensor([7, filled, 0, 0], dtype=I32).to(dev)
    idx = torch.full((n + 2,), -7, dtype=I32, device=dev)
    for seed, draw in ((0, 0), (12345, 678), (2 ** 64 - 1, 2 ** 64 - 1)):
        idx.fill_(-7)
        eng.replay_sample(state, C, n, seed, draw, idx[1:n + 1])
        got = idx.cpu().tolist()
        assert got[0] == -7 and got[-1] == -7                   # nothing outside the n entries
        assert got[1:-1] == twin.sample(filled, n, seed, draw), (seed, draw)
    state[1] = C + 5                                            # a state word beyond the capacity is clamped to it
    eng.replay_sample(state, 16, min(n, 16), 1, 2, idx[1:min(n, 16) + 1])
    assert idx[1:min(n, 16) + 1].cpu().tolist() == twin.sample(16, min(n, 16), 1, 2)


# ---- 3. a step from the buffer ----------------------------------------------------------------------------------------------------------
PERM = [3, 0, 4, 1, 2]              # the order the source rows are pushed in: slot s holds row PERM[s]


@lru_cache(None)
def step_case(net):
    batch = batch_of(net, 5, 21)
    return batch, seeded_table(batch.masks.numpy(), 16, 3)


def filled_buffer(eng, net, C=8):
    batch, tab_h = step_case(net)
    cb, keep = device_batch(eng, batch)
    tab = torch.from_numpy(tab_h).to(eng.device)
    buf = ReplayBuffer(eng, C)
    if C >= 5:
        assert push(eng, buf, cb, 5, PERM, tab) == 0 and buf.read_state() == [5, 5, 5, 0]
    else:                                                       # (one push takes at most C rows)
        assert push(eng, buf, cb, 5, PERM[:3], tab) == 0 and push(eng, buf, cb, 5, PERM[3:], tab) == 0
    return buf, (cb, keep, tab)


@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("apply", [False, True])
def test_a_step_from_the_buffer_is_the_step_on_the_source_rows(net, apply):
    batch, tab_h = step_case(net)
    eng = new_engine(lr=1e-3)
    buf, keep = filled_buffer(eng, net)
    n, dev = 3, eng.device
    loss, report = torch.full((n,), -7.0, dtype=F32, device=dev), torch.full((n, 4), -7, dtype=I32, device=dev)
    regret, status = torch.full((n,), -7.0, dtype=F64, device=dev), torch.zeros(1, dtype=I32, device=dev)
    held = [t.clone() for t in buf.row_tensors()]
    idx = buf.step(n, 1.0, 99, 4, apply=apply, loss=loss, report=report, regret=regret, status=status).cpu().tolist()
    assert idx == twin.sample(5, n, 99, 4) and int(status.cpu()[0]) == 0
    g, w = eng.online_grad(), eng.get_weights()
    want = step_rows(new_engine(lr=1e-3), batch, tab_h, [PERM[s] for s in idx], apply)
    assert want[6] and want[3] == 0
    assert bits(loss.cpu().numpy()).tolist() == bits(want[0]).tolist() and report.cpu().numpy().tolist() == want[1].tolist()
    assert regret.cpu().numpy().tolist() == want[2].tolist()
    assert bits(g).tolist() == bits(want[4]).tolist() and np.abs(g).max() > 0
    assert bits(w).tolist() == bits(want[5]).tolist()
    assert all(same_bits(a, b) for a, b in zip(held, buf.row_tensors()))          # a step reads the buffer, it does not write it


@pytest.mark.gpu
def test_a_draw_beyond_the_filled_part_is_skipped_with_the_status_bit_and_evaluate_reports_every_slot():
    batch, tab_h = step_case("kwg_mlp")
    eng = new_engine(lr=1e-3)
    buf, keep = filled_buffer(eng, "kwg_mlp")
    loss, status = torch.zeros(7, dtype=F32, device=eng.device), torch.zeros(1, dtype=I32, device=eng.device)
    idx = buf.step(7, 1.0, 1, 0, apply=False, loss=loss, status=status).cpu().tolist()
    assert idx[5:] == [-1, -1] and sorted(idx[:5]) == [0, 1, 2, 3, 4] and int(status.cpu()[0]) == 8
    assert np.isnan(loss.cpu().numpy()[5:]).all() and np.isfinite(loss.cpu().numpy()[:5]).all()
    ev_loss, ev_report, ev_regret = buf.evaluate(1.0, chunk=2)
    want = step_rows(new_engine(lr=1e-3), batch, tab_h, PERM, False)
    assert bits(ev_loss.numpy()).tolist() == bits(want[0]).tolist() and ev_report.numpy().tolist() == want[1].tolist()
    assert ev_regret.numpy().tolist() == want[2].tolist()


# ---- 4. save, load, split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_save_and_load_round_trip_and_a_file_from_another_network_is_refused(tmp_path):
    eng = new_engine()
    buf, keep = filled_buffer(eng, "kwg_mlp")
    path = str(tmp_path / "buffer.pt")
    buf.save(path)
    back = ReplayBuffer.load(eng, path)
    assert back.capacity == buf.capacity and back.read_state()[:2] == [5, 5]
    assert all(same_bits(a, b) for a, b in zip(buf.row_tensors(), back.row_tensors()))
    other = new_engine()
    device_batch(other, batch_of(ODD_NET, 1, 3))               # binds the other network
    with pytest.raises(ValueError, match="layer sizes"):
        ReplayBuffer.load(other, path)
    with pytest.raises(ValueError, match="layer sizes"):
        from gnn_branching_amd.frontier import _Round
        run = _Round()
        run.eng, run.replay, run.imitate = other, Replay(1, buffer=buf), 1
        run._imitation_buffers(4)


@pytest.mark.gpu
def test_split_moves_the_newest_entries():
    eng = new_engine()
    buf, (cb, keep, tab) = filled_buffer(eng, "kwg_mlp", C=4)  # 5 stored into 4 slots: slot 0 holds the fifth, oldest first = slots 1, 2, 3, 0
    assert buf.read_state() == [1, 4, 2, 0] and buf.order() == [1, 2, 3, 0]
    held = [t.clone() for t in buf.row_tensors()]
    hold = buf.split(0.5)
    assert buf.read_state() == [2, 2, 0, 0] and hold.read_state() == [0, 2, 0, 0] and hold.capacity == 2
    for t, h, was in zip(buf.row_tensors(), hold.row_tensors(), held):
        assert same_bits(t[:2], was[[1, 2]]) and same_bits(h, was[[3, 0]])
    assert buf.split(0.0).read_state() == [0, 0, 0, 0] and buf.read_state() == [2, 2, 0, 0]
    with pytest.raises(ValueError, match="fraction"):
        buf.split(1.5)


# ---- 5. the frontier --------------------------------------------------------------------------------------------------------------------
RP = dict(capacity=16, batch=2, steps=2, seed=11)
_runs = {}


def replay_run(K, branching, repack="host", rounds=FR_ROUNDS):
    from gnn_branching_amd.frontier import branch_and_bound_frontier
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    lp, choice, _ = toy(online=True)
    trace, audit, stats = [], [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=quiet, trace=trace, stats=stats,
                                    strong_candidates=FR_CANDIDATES, strong_audit=audit, branching=branching, imitate=Replay(every=1, **RP),
                                    imitate_margin=FR_MARGIN[branching], repack=repack)
    return res, trace, audit, stats, choice


def replay_host_loop(K, rounds, branching, tables, margin, repack):
    """tests/test_gpu_imitation.py's host loop with a Python ring in the step's place: per learning round the picked parents and their
    table rows are pushed (tests/replay_twin.py's rule), then ``steps`` times a draw of min(batch, filled) entries is collated and given
    to ``ScorerEngine.imitation_step``, on an engine in the run's repack mode (as tests/test_gpu_frontier_repack.py's twins are)."""
    from gnn_branching_amd import bab_caller, lp_producer
    from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, at_least_the_parents, toy, ub64
    lp, choice, root_mask = toy(online=True)
    eng = choice._eng()
    eng.set_repack(repack)
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
    out = {k: [] for k in ("decisions", "child_bounds", "idx", "loss", "report", "regret", "stored", "filled", "global_lb", "global_ub")}
    ring, draw, steps, rows, stored_all, skipped_all = twin.Ring(RP["capacity"]), 0, 0, 0, 0, 0
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
        idx, loss, report, regret = [], [], [], []
        table = np.full((len(picked), R), NAN)
        for i, a in enumerate(tab):
            table[i, a["candidates"]] = a["improvements"]
        masks = np.stack([torch.cat([(m == -1).float().reshape(-1) for m in s.mask]).numpy() for s in subs])
        assert ring.push(subs, table, masks) == 0
        stored_all, skipped_all = stored_all + ring.state[2], skipped_all + ring.state[3]
        if ring.filled >= 1:
            b = min(RP["batch"], ring.filled)
            for _ in range(RP["steps"]):
                slots, pairs = ring.draw(b, RP["seed"], draw)
                draw += 1
                args, _ = bab_caller.collate([p[0] for p in pairs], fixed)
                l, rep, reg = (v.tolist() for v in eng.imitation_step(args, np.stack([p[1] for p in pairs]), margin))
                idx.append(slots), loss.append(l), report.append(rep), regret.append(reg)
            steps, rows = steps + RP["steps"], rows + RP["steps"] * b
        for k, v in (("decisions", decs), ("child_bounds", [INF if c is None else c.lb for c in children]), ("idx", idx), ("loss", loss),
                     ("report", report), ("regret", regret), ("stored", ring.state[2]), ("filled", ring.filled), ("global_lb", global_lb()),
                     ("global_ub", gub)):
            out[k].append(v)
    out.update(steps=steps, rows=rows, stored_all=stored_all, skipped_all=skipped_all, weights=eng.get_weights().copy(), weights_start=w_start)
    return out


def both(K, branching, repack):
    key = (K, branching, repack)
    if key not in _runs:
        run = replay_run(K, branching, repack)
        rows, tables = iter(run[2]), []
        for t in run[1]:
            tables.append([next(rows) for _ in t["slots"]])
        _runs[key] = (replay_host_loop(K, FR_ROUNDS, branching, tables, FR_MARGIN[branching], repack), run)
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("repack", ["host", "device"])
@pytest.mark.parametrize("branching", ["gnn", "strong"])
@pytest.mark.parametrize("K", [1, 3])
def test_the_frontier_with_a_replay_equals_a_host_loop_with_a_python_ring(K, branching, repack):
    from gnn_branching_amd.engine import state_blob
    from tests.frontier_twin import masked
    host, ((glb, gub, rounds, bounded, reason), trace, audit, stats, choice) = both(K, branching, repack)
    print("host", {k: v for k, v in host.items() if not k.startswith("weights")}, "frontier", (glb, gub, rounds, bounded, reason), stats)
    assert choice._eng().repack_mode == "host"                  # the run puts the engine's mode back
    assert len(trace) == len(host["decisions"]) >= 2
    assert any(v > 0 for r in host["loss"] for l in r for v in l), "no step of the host loop carried a gradient"
    assert [t["decisions"] for t in trace] == host["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == host["child_bounds"]
    for r, t in enumerate(trace):
        assert (t["replay_stored"], t["replay_filled"]) == (host["stored"][r], host["filled"][r]), r
        assert t["replay_idx"] == host["idx"][r], r             # the drawn slots
        assert t["global_lb"] == host["global_lb"][r] and abs(t["global_ub"] - host["global_ub"][r]) <= 1e-9 * max(1.0, abs(host["global_ub"][r]))
        for s in range(RP["steps"]):
            np.testing.assert_array_equal(bits(t["replay_loss"][s]), bits(host["loss"][r][s]))       # the fp32 losses, bit for bit
            assert t["replay_report"][s] == host["report"][r][s] and same_or_nan(t["replay_regret"][s], host["regret"][r][s])
    assert any(len(set(i)) == 2 for r in host["idx"] for i in r), "no step drew two entries"
    assert glb == host["global_lb"][-1] and abs(gub - host["global_ub"][-1]) <= 1e-9 * max(1.0, abs(host["global_ub"][-1]))
    assert stats["imitation_steps"] == host["steps"] == RP["steps"] * len(trace) and stats["imitation_rows"] == host["rows"]
    assert (stats["replay_stored"], stats["replay_skipped"], stats["replay_filled"]) == (host["stored_all"], host["skipped_all"], host["filled"][-1])
    got_w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(got_w), bits(host["weights"]))                                # the final parameters, bit for bit
    assert (bits(host["weights"]) != bits(host["weights_start"])).any()
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(got_w))          # the nn.Module mirrors the device


# ---- 6. collection only -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("branching", ["gnn", "strong"])
def test_steps_0_is_the_audited_run_and_creates_no_trainer(branching):
    from gnn_branching_amd.frontier import branch_and_bound_frontier
    from tests.frontier_strong_twin import same
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    out = []
    for extra in ({"strong_audit": []}, {"imitate": Replay(every=1, capacity=16, steps=0)}):
        lp, choice, _ = toy(online=True)
        w0 = choice.model.engine().get_weights().copy()
        trace, stats = [], {}
        res = branch_and_bound_frontier(lp, choice, lp.layers, K=3, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=FR_ROUNDS, log=quiet, trace=trace, stats=stats,
                                        strong_candidates=FR_CANDIDATES, branching=branching, **extra)
        assert choice._engine is None and not getattr(choice.model.engine(), "_online", False)       # no optimizer was made
        assert bits(choice.model.engine().get_weights()).tolist() == bits(w0).tolist()
        out.append((res, trace, stats))
    (a, ta, sa), (b, tb, sb) = out
    assert same(list(a), list(b)) and len(ta) == len(tb) >= 2
    for x, y in zip(ta, tb):
        for key in ("slots", "decisions", "child_bounds", "infeasible", "live"):
            assert same(x[key], y[key]), key
    assert "imitation_steps" not in sa and sb["imitation_steps"] == 0 and sb["replay_stored"] >= 2
    assert sb["replay_filled"] == min(16, sb["replay_stored"]) and sb["replay_stored"] + sb["replay_skipped"] == sum(len(t["slots"]) for t in tb)
    assert all("replay_loss" not in t for t in tb) and sum(t.get("replay_stored", 0) for t in tb) == sb["replay_stored"]


# ---- 7. the reads of a learning round ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("branching", ["gnn", "strong"])
def test_a_learning_round_copies_nothing_but_the_candidate_count_the_state_record_and_the_buffer_state(branching):
    from gnn_branching_amd import _lib
    from gnn_branching_amd.frontier import FrontierRun
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    from tests.test_gpu_frontier_online import sync_mode_is_live
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy(online=True)
    run = FrontierRun(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, imitate=Replay(every=1, capacity=8, batch=2, steps=2),
                      strong_candidates=FR_CANDIDATES, strong_chunk=3, branching=branching)
    st = run.root()
    if not sync_mode_is_live(run):
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
    before = torch.cuda.get_sync_debug_mode()
    w0 = run.eng.get_weights().copy()
    reads = []

    def exempt(read, tag):
        def wrapped(*a):
            with pytest.raises(RuntimeError):
                read(*a)
            torch.cuda.set_sync_debug_mode(before)
            try:
                reads.append((tag, read(*a)))
            finally:
                torch.cuda.set_sync_debug_mode("error")
            return reads[-1][1]
        return wrapped
    run.read_candidates = exempt(run.read_candidates, "candidates")
    run.buffer.read_state = exempt(run.buffer.read_state, "buffer")
    try:
        torch.cuda.set_sync_debug_mode("error")
        run.launch_round(1, int(st[_lib.FS_IN_USE]))            # the push is part of the launch: device work only
        with pytest.raises(RuntimeError):
            run.read_state()                                    # the state record: a synchronising copy
        torch.cuda.set_sync_debug_mode(before)
        st = run.pool.state.cpu().tolist()                      # ... exempted by hand
        assert run.imitate_pending and run.learning
        torch.cuda.set_sync_debug_mode("error")
        run._imitate()                                          # its one read: the 16 bytes of the buffer's state word
        torch.cuda.set_sync_debug_mode(before)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert reads == [("candidates", FR_CANDIDATES), ("buffer", [1, 1, 1, 0])]
    assert run.imitation_steps == 2 and run.imitation_rows == 2 and run.draw == 2 and not run.imitate_pending
    run.check_status()
    assert (bits(run.eng.get_weights()) != bits(w0)).any()
    run.close()


# ---- 8. many jobs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_jobs_run_fills_one_buffer_with_the_rows_of_both_jobs():
    from gnn_branching_amd.frontier import FrontierJob, verify_properties_strong
    from tests.frontier_jobs_imitation_twin import online_jobs
    from tests.frontier_twin import EPS_BAB, LR, N_ITER
    from tests.test_gpu_frontier_jobs import JOBS
    ids = (0, 1)
    choice, lps = online_jobs(ids)
    eng = choice._eng()
    eng.bind(lps[0].layers[:-1], (3, 32, 32))
    buf = ReplayBuffer(eng, 32)
    jobs = [FrontierJob(lp.input_lb, lp.input_ub, lp.layers[-1], JOBS[j][3]) for lp, j in zip(lps, ids)]
    learned, w0 = {}, eng.get_weights().copy()
    got = verify_properties_strong(choice, lps[0].layers[:-1], jobs, K=2, segments=2, capacity=9, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=3, log=quiet,
                                   learned=learned, imitate=Replay(every=1, buffer=buf, batch=4, steps=1, seed=3), strong_candidates=FR_CANDIDATES,
                                   branching="strong")
    head, filled, _, _ = buf.read_state()
    print(got, learned, buf.read_state())
    assert len(got) == 2 and learned["replay_filled"] == filled == learned["replay_stored"] >= 4 and learned["imitation_steps"] == learned["rounds"] >= 2
    pw = [lp.layers[-1].weight.detach().reshape(-1).float() for lp in lps]
    pb = [float(lp.layers[-1].bias.detach().reshape(-1)[0]) for lp in lps]
    assert not torch.equal(pw[0], pw[1])
    owner = []
    for s in range(filled):
        row, b = buf.prop_w[s].cpu(), float(buf.prop_b[s].cpu()[0])
        match = [j for j in (0, 1) if torch.equal(row, pw[j]) and b == pb[j]]
        assert len(match) == 1, s                               # every stored row carries its own job's property row
        owner.append(match[0])
    assert set(owner) == {0, 1}
    assert (bits(eng.get_weights()) != bits(w0)).any()


# ---- 9. train_epochs --------------------------------------------------------------------------------------------------------------------
TRAIN_B, TRAIN_BATCH, TRAIN_EPOCHS, TRAIN_SEED, TRAIN_LR, TRAIN_WD = 6, 2, 4, 5, 1e-3, 1e-4


@lru_cache(None)
def train_case():
    batch = batch_of("kwg_mlp", TRAIN_B, 11)
    return batch, seeded_table(batch.masks.numpy(), 16, 1)


@lru_cache(None)
def twin_curve():
    """The fp32 autograd twin over the draws ``train_epochs`` makes: the mean loss over all rows before and after."""
    batch, table = train_case()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    o = ImitationOracle(state_of("random"), lr=TRAIN_LR, wd=TRAIN_WD, dtype=torch.float32)

    def mean_loss():
        return float(np.mean(o.step(batch.forward_args(), table, 1.0, apply=False)[0]))
    first = mean_loss()
    for draw in range(TRAIN_EPOCHS * ((TRAIN_B + TRAIN_BATCH - 1) // TRAIN_BATCH)):
        idx = twin.sample(TRAIN_B, TRAIN_BATCH, TRAIN_SEED, draw)
        o.step(take(batch, idx).forward_args(), table[idx], 1.0)
    return first, mean_loss()


def test_the_twins_loss_falls_over_the_epochs_of_the_training_case():
    """The condition of the device test, on the CPU: the fp32 twin's mean loss over the buffer is lower after the same draws."""
    first, last = twin_curve()
    print("twin mean loss", first, "->", last)
    assert first > 0.1 and last < first


def train_choice():
    from gnn_branching_amd.graphnet.graph_score_online import GraphChoice
    batch, _ = train_case()
    g = GraphChoice([m[0] for m in batch.bab_masks], os.path.join(nets.ASSETS, "cifar_trained_gnn.npz"), lr=TRAIN_LR, wd=TRAIN_WD)
    g.verbose = False
    g.model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state_of("random").items()})
    return g


def train_buffer(choice):
    batch, tab_h = train_case()
    eng = choice._eng()
    cb, keep = device_batch(eng, batch)
    buf = ReplayBuffer(eng, 8)
    assert push(eng, buf, cb, TRAIN_B, list(range(TRAIN_B)), torch.from_numpy(tab_h).to(eng.device)) == 0
    return buf


@pytest.mark.gpu
def test_train_epochs_is_a_loop_of_buffer_steps_and_its_loss_falls():
    from gnn_branching_amd.engine import state_blob
    from gnn_branching_amd.replay import evaluate, train_epochs
    a = train_choice()
    buf = train_buffer(a)
    records = train_epochs(a, buf, TRAIN_EPOCHS, batch=TRAIN_BATCH, margin=1.0, seed=TRAIN_SEED, holdout=None)
    b = train_choice()
    buf_b = train_buffer(b)
    per_epoch = (TRAIN_B + TRAIN_BATCH - 1) // TRAIN_BATCH
    assert [r["epoch"] for r in records] == list(range(TRAIN_EPOCHS + 1)) and [r["steps"] for r in records] == [e * per_epoch for e in range(TRAIN_EPOCHS + 1)]
    curve = [evaluate(buf_b, 1.0)]
    for draw in range(TRAIN_EPOCHS * per_epoch):
        buf_b.step(TRAIN_BATCH, 1.0, TRAIN_SEED, draw)
        if (draw + 1) % per_epoch == 0:
            curve.append(evaluate(buf_b, 1.0))
    wa, wb = a._eng().get_weights(), b._eng().get_weights()
    np.testing.assert_array_equal(bits(wa), bits(wb))
    assert [r["train"] for r in records] == curve and all(r["holdout"] is None for r in records)
    np.testing.assert_array_equal(bits(state_blob(a.model.state_dict())), bits(wa))                  # the nn.Module mirrors the device
    first, last = records[0]["train"], records[-1]["train"]
    print("device curve", [(r["train"]["loss"], r["train"]["top1"]) for r in records], "twin", twin_curve())
    assert first["rows"] == TRAIN_B and abs(first["loss"] - twin_curve()[0]) <= 1e-4 * max(1.0, twin_curve()[0])      # the same parameters
    assert last["loss"] < first["loss"]
    hold = buf.split(0.34)                                      # floor(0.34 * 6) = 2 rows held out
    more = train_epochs(a, buf, 1, batch=TRAIN_BATCH, seed=TRAIN_SEED, holdout=hold)
    assert more[0]["train"]["rows"] == 4 and more[0]["holdout"]["rows"] == 2 and more[1]["steps"] == 2
