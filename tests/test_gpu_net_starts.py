"""gnnb_net_starts and gnnb_net_descend_starts on the MI355X (ScorerEngine.net_starts / net_descend_starts).

The start points are held, bit for bit at every coordinate, to the Python restatement of tests/test_net_starts_cpu.py (one correct rounding
per point, by ``fractions.Fraction``).  The descent from many starts is held, bit for bit, to the existing gnnb_net_descend fed the same
B * n_starts points as a flat batch of rows of their own -- values, steps, and through the pick the winner's point -- and the pick to a
restatement of the total order (value, start index) written here.  With S = gnnb_net_descend_starts_tile() the start counts are 1, S - 1,
S, S + 1 and 2S + 1: one start, a partly empty tile, a full one, a second tile with one start, and three tiles."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib
from tests.common import register_kw_archs, register_toy_archs
from tests.test_gpu_net_descend import BIG_STEP, NETS, STEP, case
from tests.test_net_starts_cpu import start_points

pytestmark = pytest.mark.gpu

SEED = 7


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    return ScorerEngine(None)


@lru_cache(None)
def tile():
    return _lib.load().gnnb_net_descend_starts_tile()


def start_counts():
    S = tile()
    return sorted({n for n in (1, S - 1, S, S + 1, 2 * S + 1) if n >= 1})


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def flat(c, t, rows):
    return t[rows].reshape(len(rows), -1).contiguous()


def make_starts(engine, c, R, seed=SEED, rows=None, x0=None, box=None, **kw):
    """The device's (len(rows), R + 1, N_0) start points of the case's rows."""
    rows = list(range(c.B)) if rows is None else rows
    x0 = c.x0 if x0 is None else x0
    lo, hi = (c.x_lo, c.x_hi) if box is None else box
    dev = engine.device
    return engine.net_starts(c.net.fixed, x0[rows].to(dev), flat(c, lo, rows).to(dev), flat(c, hi, rows).to(dev), R, seed, **kw)


@lru_cache(None)
def restated(name, B, R, seed=SEED):
    c = case(name, B)
    return torch.from_numpy(np.stack([start_points(c.x0[b].numpy(), c.x_lo[b].numpy(), c.x_hi[b].numpy(), R, seed) for b in range(B)]))


def descend_starts(engine, c, starts, n_steps, step=STEP, rows=None, **kw):
    """gnnb_net_descend_starts on the device tensor ``starts`` of the case's rows; everything on the CPU."""
    rows = list(range(c.B)) if rows is None else rows
    dev = engine.device
    kw = {"want_index": True, "want_values": True, "want_steps": True, **kw}
    out = engine.net_descend_starts(c.net.fixed, [c.props[b] for b in rows], starts, flat(c, c.x_lo, rows).to(dev), flat(c, c.x_hi, rows).to(dev),
                                    n_steps, step, in_shape=tuple(c.net.shape), **kw)
    return tuple(None if t is None else t.cpu() for t in out)


def flat_batch(engine, c, starts, n_steps, step=STEP, rows=None):
    """The existing gnnb_net_descend on the same points as a flat batch of len(rows) * n rows: (x_best, value, steps), (len(rows), n, .)."""
    rows = list(range(c.B)) if rows is None else rows
    n, dev = int(starts.shape[1]), engine.device
    rep = [b for b in rows for _ in range(n)]
    x_best, value, _, steps = engine.net_descend(c.net.fixed, [c.props[b] for b in rep], starts.reshape((len(rep),) + tuple(c.net.shape)),
                                                 flat(c, c.x_lo, rep).to(dev), flat(c, c.x_hi, rep).to(dev), n_steps, step, want_steps=True)
    return x_best.cpu().reshape(len(rows), n, -1), value.cpu().reshape(len(rows), n), steps.cpu().reshape(len(rows), n)


def pick(values):
    """The winner of a row in the total order (value, start index): strict <, in start order; a NaN never wins; all NaN: start 0."""
    best = None
    for i, v in enumerate(values):
        if v == v and (best is None or v < values[best]):
            best = i
    return 0 if best is None else best


def net_eval(engine, c, x, rows=None):
    rows = list(range(c.B)) if rows is None else rows
    return engine.net_eval(c.net.fixed, [c.props[b] for b in rows], x.reshape((len(rows),) + tuple(c.net.shape)).to(engine.device)).cpu()


def check_pick(engine, c, got, want, rows=None):
    """``got`` of descend_starts against ``want`` of flat_batch on the same start points: every start, then the winner."""
    x_best, value, index, values, steps = got
    fx, fv, fs = want
    assert torch.equal(bits(values), bits(fv)) and torch.equal(steps, fs)
    for b in range(values.shape[0]):
        w = pick(values[b].tolist())
        assert int(index[b]) == w, (b, int(index[b]), w)
        assert torch.equal(bits(value[b]), bits(fv[b, w])) and torch.equal(bits(x_best[b]), bits(fx[b, w])), b
    assert torch.equal(bits(value), bits(net_eval(engine, c, x_best, rows)))          # value == gnnb_net_eval(x_best), bit for bit
    return x_best, value, index, values, steps


# ---- gnnb_net_starts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("name", NETS)
def test_starts_are_the_restatement_bit_for_bit(name, B, engine):
    c, R = case(name, B), 2 * tile()
    got = make_starts(engine, c, R).cpu()
    assert got.shape == (B, R + 1, c.x0[0].numel()) and got.dtype == torch.float32
    assert torch.equal(bits(got[:, 0]), bits(c.x0.reshape(B, -1)))                    # slot 0 == x0
    assert torch.equal(bits(got), bits(restated(name, B, R)))
    lo, hi = c.x_lo.reshape(B, 1, -1), c.x_hi.reshape(B, 1, -1)
    assert bool((got.double() >= lo).all()) and bool((got.double() <= hi).all())
    assert len(torch.unique(got[:, 1:].reshape(-1))) > got[:, 1:].numel() // 2          # (not a constant)


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
def test_starts_on_a_box_of_fp64_corners(name, engine):
    """Corners that are no fp32 values and widths that are no powers of two: the fma's one rounding and the move inside the box."""
    c = case(name)
    rng = np.random.RandomState(5)
    lo = c.x_lo - torch.from_numpy(rng.uniform(0.0, 0.01, tuple(c.x_lo.shape)))
    hi = c.x_hi + torch.from_numpy(rng.uniform(0.0, 0.01, tuple(c.x_hi.shape)))
    hi[1] = lo[1] + 2.0 ** -20                                                        # a row of very narrow coordinates: rounding leaves the box
    x0 = c.x0.clone()
    x0[1] = lo[1].float()
    got = make_starts(engine, c, 3, x0=x0, box=(lo, hi)).cpu()
    want = torch.from_numpy(np.stack([start_points(x0[b].numpy(), lo[b].numpy(), hi[b].numpy(), 3, SEED) for b in range(c.B)]))
    assert torch.equal(bits(got), bits(want))
    inside = (got[:, 1:].double() >= lo.reshape(c.B, 1, -1)) & (got[:, 1:].double() <= hi.reshape(c.B, 1, -1))
    assert bool(inside[[0, 2, 3, 4]].all())


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
def test_a_rows_starts_are_its_own(name, engine):
    c, R = case(name), tile() + 1
    batch = make_starts(engine, c, R).cpu()
    for b in range(c.B):                                                              # a row alone == its row of the batch
        assert torch.equal(bits(make_starts(engine, c, R, rows=[b]).cpu()), bits(batch[b:b + 1])), (name, b)
    order = [3, 1, 4, 0, 2]                                                           # a row moved to another index gives the same starts
    assert torch.equal(bits(make_starts(engine, c, R, rows=order).cpu()), bits(batch[order]))
    other = make_starts(engine, c, R, seed=SEED + 1).cpu()                            # two seeds differ (slot 0 does not)
    assert torch.equal(bits(other[:, 0]), bits(batch[:, 0])) and bool((other[:, 1:] != batch[:, 1:]).any(dim=2).all())
    big = make_starts(engine, c, R, seed=2 ** 64 - 1).cpu()
    assert bool((big[:, 1:] != batch[:, 1:]).any(dim=2).all())


def test_a_degenerate_coordinate_a_nan_and_no_random_start(engine):
    c = case("kwg_rect")
    lo, hi = c.x_lo.clone(), c.x_hi.clone()
    hi.reshape(c.B, -1)[:, 11] = lo.reshape(c.B, -1)[:, 11]                           # x_lo == x_hi: that value (a multiple of the grid: an fp32 value)
    x0 = c.x0.clone()
    x0.reshape(c.B, -1)[:, 11] = lo.reshape(c.B, -1)[:, 11].float()
    x0.reshape(c.B, -1)[2, 5] = float("nan")                                          # a NaN stays in slot 0
    got = make_starts(engine, c, 4, x0=x0, box=(lo, hi)).cpu()
    assert torch.equal(got[:, :, 11].double(), lo.reshape(c.B, 1, -1)[:, :, 11].expand(-1, 5))
    assert torch.equal(bits(got[:, 0]), bits(x0.reshape(c.B, -1)))
    assert not bool(torch.isnan(got[:, 1:]).any())
    want = torch.from_numpy(start_points(x0[2].numpy(), lo[2].numpy(), hi[2].numpy(), 4, SEED))      # (the NaN hashes by its bits)
    assert torch.equal(bits(got[2]), bits(want))
    N0 = c.x0[0].numel()                                                              # R = 0 writes slot 0 only
    poison = torch.full((c.B, 3, N0), -77.0, dtype=torch.float32, device=engine.device)
    make_starts(engine, c, 0, starts=poison)
    host = poison.cpu().reshape(-1)
    assert torch.equal(bits(host[:c.B * N0]), bits(c.x0.reshape(-1))) and bool((host[c.B * N0:] == -77.0).all())


# ---- gnnb_net_descend_starts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("name", NETS)
def test_one_start_is_net_descend(name, B, engine):
    c = case(name, B)
    starts = make_starts(engine, c, 0)
    for n_steps, step in ((0, STEP), (8, STEP), (8, BIG_STEP)):
        x_best, value, index, values, steps = descend_starts(engine, c, starts, n_steps, step)
        fx, fv, fs = flat_batch(engine, c, starts, n_steps, step)
        assert torch.equal(bits(x_best), bits(fx[:, 0])) and torch.equal(bits(value), bits(fv[:, 0])) and torch.equal(steps, fs)
        assert index.tolist() == [0] * B and torch.equal(bits(values[:, 0]), bits(value))


@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("name", NETS)
def test_every_start_ends_where_net_descend_ends(name, B, engine):
    """n_steps 0, 1 and 8 at step 1/64 and 8 at step 1/2, at every start count: each start's value and steps are gnnb_net_descend's on that
    point as a row of its own, bit for bit, and the winner is the restatement's.  At step 1/2 the stop rule trips at different steps inside
    one tile (asserted on the flat batch's counts at the largest start count): the masking is exercised."""
    c, S = case(name, B), tile()
    for n in start_counts():
        starts = make_starts(engine, c, n - 1)
        for n_steps, step in ((0, STEP), (1, STEP), (8, STEP), (8, BIG_STEP)):
            want = flat_batch(engine, c, starts, n_steps, step)
            x_best, value, index, values, steps = check_pick(engine, c, descend_starts(engine, c, starts, n_steps, step), want)
            assert bool((x_best.double() >= c.x_lo.reshape(B, -1)).all()) and bool((x_best.double() <= c.x_hi.reshape(B, -1)).all())
            assert bool((value <= values[:, 0]).all())
            if step == BIG_STEP and n == 2 * S + 1:
                mixed = [len(set(steps[b, t:t + S].tolist())) > 1 for b in range(B) for t in range(0, n, S)]
                print(f"net_descend_starts {name} B {B}: steps per start at step 1/2 {steps.tolist()}")
                assert any(mixed), (name, B, steps.tolist())


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
def test_a_tie_a_nan_start_and_an_all_nan_row(name, engine):
    c, S = case(name), tile()
    n = 2 * S + 1
    starts = make_starts(engine, c, n - 1)
    clean = check_pick(engine, c, descend_starts(engine, c, starts, 8), flat_batch(engine, c, starts, 8))
    # a planted tie: the winner's start point once more in another slot -- the lower slot wins
    tied = starts.clone()
    twin = [(int(w) + 2) % n for w in clean[2]]
    for b, j in enumerate(twin):
        tied[b, j] = starts[b, int(clean[2][b])]
    got = check_pick(engine, c, descend_starts(engine, c, tied, 8), flat_batch(engine, c, tied, 8))
    for b, j in enumerate(twin):
        w = int(clean[2][b])
        assert torch.equal(bits(got[3][b, j]), bits(got[3][b, w])) and int(got[2][b]) == min(j, w), (name, b)
    # a NaN start in the middle of a tile never wins and leaves its neighbours' bits alone
    mid = S + 1 if S > 1 else 1
    poisoned = starts.clone()
    poisoned[:, mid, 7] = float("nan")
    x_best, value, index, values, steps = descend_starts(engine, c, poisoned, 8)
    keep = [i for i in range(n) if i != mid]
    assert bool(torch.isnan(values[:, mid]).all()) and steps[:, mid].tolist() == [0] * c.B
    assert torch.equal(bits(values[:, keep]), bits(clean[3][:, keep])) and torch.equal(steps[:, keep], clean[4][:, keep])
    for b in range(c.B):
        w = pick(values[b].tolist())
        assert w != mid and int(index[b]) == w and torch.equal(bits(value[b]), bits(values[b, w]))
    # a row whose every start holds a NaN: start 0 and its NaN, gnnb_net_descend's answer for that row
    poisoned = starts.clone()
    poisoned[2, :, 3] = float("nan")
    x_best, value, index, values, steps = descend_starts(engine, c, poisoned, 8)
    assert int(index[2]) == 0 and bool(torch.isnan(value[2])) and bool(torch.isnan(values[2]).all()) and steps[2].tolist() == [0] * n
    assert torch.equal(bits(x_best[2]), bits(poisoned[2, 0].cpu()))
    for b in (0, 1, 3, 4):
        assert torch.equal(bits(x_best[b]), bits(clean[0][b])) and torch.equal(bits(value[b]), bits(clean[1][b])) and int(index[b]) == int(clean[2][b])


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
def test_a_row_alone_is_its_row_of_the_batch_and_the_optional_outputs_may_be_null(name, engine):
    c, n = case(name), tile() + 1
    starts = make_starts(engine, c, n - 1)
    batch = descend_starts(engine, c, starts, 8, BIG_STEP)
    for b in range(c.B):
        alone = descend_starts(engine, c, starts[b:b + 1].contiguous(), 8, BIG_STEP, rows=[b])
        for got, want in zip(alone, batch):
            assert torch.equal(bits(got), bits(want[b:b + 1])), (name, b)
    x_best, value, index, values, steps = descend_starts(engine, c, starts, 8, BIG_STEP, want_index=False, want_values=False, want_steps=False)
    assert index is None and values is None and steps is None
    assert torch.equal(bits(x_best), bits(batch[0])) and torch.equal(bits(value), bits(batch[1]))


def test_limits_are_refused(engine):
    c = case("kwg_mlp")
    dev, lib = engine.device, engine.lib
    starts = make_starts(engine, c, 2)
    assert lib.gnnb_net_descend_starts_workspace_bytes(engine.h, 1, 4097) > 0          # R = 4096 random starts and the LP point
    assert lib.gnnb_net_descend_starts_workspace_bytes(engine.h, 1, 4098) == 0
    assert lib.gnnb_net_descend_starts_workspace_bytes(engine.h, 0, 4) == 0 and lib.gnnb_net_descend_starts_workspace_bytes(engine.h, 2, 0) == 0
    with pytest.raises(RuntimeError, match="gnnb_net_starts.*R = 4097"):
        make_starts(engine, c, 4097)
    with pytest.raises(RuntimeError, match="gnnb_net_starts.*R = -1"):
        make_starts(engine, c, -1, starts=starts)
    with pytest.raises(RuntimeError, match="gnnb_net_starts.*overlap"):
        x0 = c.x0.to(dev)
        engine.net_starts(c.net.fixed, x0, c.x_lo.reshape(c.B, -1).to(dev), c.x_hi.reshape(c.B, -1).to(dev), 0, starts=x0.reshape(c.B, -1))
    with pytest.raises(ValueError, match="seed"):
        make_starts(engine, c, 2, seed=-1)
    args = (c.net.fixed, c.props, starts, c.x_lo.reshape(c.B, -1).to(dev), c.x_hi.reshape(c.B, -1).to(dev))
    for kw, word in (({"n_steps": -1}, "n_steps = -1"), ({"n_steps": 1, "step": 0.0}, "step = 0"), ({"n_steps": 1, "step": 1.5}, "step = 1.5"),
                     ({"n_steps": 1, "step": float("nan")}, "step = nan")):
        with pytest.raises(RuntimeError, match="gnnb_net_descend_starts.*" + word):
            engine.net_descend_starts(*args, **kw)
    with pytest.raises(RuntimeError, match="gnnb_net_descend_starts.*workspace"):
        engine.net_descend_starts(*args, n_steps=1, workspace=torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="gnnb_net_descend_starts.*overlap"):
        engine.net_descend_starts(*args, n_steps=1, x_best=starts.reshape(c.B, -1))
    engine.net_descend_starts(*args, n_steps=1, step=1.0)                            # the upper end of the range is inside it
    from gnn_branching_amd.engine import ScorerEngine
    fresh = ScorerEngine(None)                                                       # GNNB_E_STATE before bind, and no workspace to size
    assert fresh.lib.gnnb_net_descend_starts_workspace_bytes(fresh.h, 1, 3) == 0
    one = C.c_void_p(8)
    assert fresh.lib.gnnb_net_starts(fresh.h, one, one, one, 1, 2, 0, one, None) == -3
    assert b"gnnb_net_starts" in _lib.load().gnnb_last_error()
    assert fresh.lib.gnnb_net_descend_starts(fresh.h, one, 3, one, one, one, one, 1, 1, 0.5, one, one, None, None, None, one, 8, None) == -3
    assert b"gnnb_net_descend_starts" in _lib.load().gnnb_last_error()
