"""gnnb_net_descend on the MI355X (ScorerEngine.net_descend) against a torch fp64 twin written here: the gradient at
the start point against autograd, n_steps = 0 against gnnb_net_eval bit for bit, one step against the rule's value per coordinate, eight steps
against the twin's trajectory, rows against their batch, a NaN row, and the limits.

The twin (``forward64``, ``descend64``) asserts ITS OWN conditions on the seeds chosen below -- no pre-activation within 1e-12 of zero, no
non-zero gradient entry below 1e-9 of the largest, no two consecutive values within 1e-9 -- so that what the device is held to does not
hang on a sign that fp64 rounding decides.  tests/test_frontier_witness_cpu.py runs the twin alone on every case (no GPU needed)."""
import copy
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import _lib
from tests import margins
from tests.common import register_kw_archs, register_toy_archs
from tests.test_gpu_kw_geometry import Net

pytestmark = pytest.mark.gpu

NETS = ["kwg_mlp", "kwg_rect", "kwg_gap", "kwg_s1", "kwg_single", "kwg_deep8"]
STEP = 1.0 / 64
GRID = 2.0 ** -10                   # box corners and start points are multiples of it: fp32 values
SEED = {name: 31 for name in NETS}  # checked on the CPU with the twin (its assertions hold for these)


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    return ScorerEngine(None)


class Case:
    """B start points with a box and a property row each."""

    def __init__(self, name, B):
        register_kw_archs()
        self.net, self.B = Net(name), B
        rng = np.random.RandomState(SEED[name] + B)
        shape = (B,) + tuple(self.net.shape)
        centre = np.round(rng.uniform(-1, 1, shape) / GRID) * GRID
        half = (np.array([32, 16, 64, 32, 48])[:B] * GRID).reshape((B,) + (1,) * len(self.net.shape))
        self.x_lo, self.x_hi = torch.from_numpy(centre - half), torch.from_numpy(centre + half)
        self.x0 = torch.from_numpy((centre + np.round(rng.uniform(-1, 1, shape) * half / GRID) * GRID).astype(np.float32))
        assert bool((self.x0.double() >= self.x_lo).all()) and bool((self.x0.double() <= self.x_hi).all())
        self.props = [self.net.prop(i, (i + 3) % 10) for i in range(B)]
        self.layers = [[copy.deepcopy(l).double() for l in self.net.fixed + [p]] for p in self.props]


@lru_cache(None)
def case(name, B=5):
    return Case(name, B)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def forward64(layers, x32):
    """(f, g) of the layers in fp64 at the fp32 point x32: the value and autograd's gradient.  Asserts that no ReLU's input is within 1e-12
    of zero: there the gradient is a matter of rounding."""
    x = x32.double().clone().requires_grad_(True)
    act = x[None]
    for l in layers:
        if type(l) is nn.ReLU:
            assert float(act.detach().abs().min()) > 1e-12, "a pre-activation of the twin is within 1e-12 of zero"
        act = l(act)
    f = act.reshape(())
    (g,) = torch.autograd.grad(f, x)
    return float(f.detach()), g


def rule(x32, g, x_lo, x_hi, step, sign=None):
    """The step's value per coordinate: fp64, clamped, rounded to the nearest fp32 and moved inside the box where rounding left it."""
    s = torch.sign(g) if sign is None else sign
    v = torch.minimum(torch.maximum(x32.double() - step * (x_hi - x_lo) * s, x_lo), x_hi)
    r = v.float()
    r = torch.where(r.double() < x_lo, torch.nextafter(r, torch.full_like(r, float("inf"))), r)
    return torch.where(r.double() > x_hi, torch.nextafter(r, torch.full_like(r, float("-inf"))), r)


def clear_gradient(g):
    nz = g[g != 0].abs()
    assert nz.numel() and float(nz.min()) > 1e-9 * float(g.abs().max()), "a non-zero gradient entry of the twin is below 1e-9 of the largest"


def descend64(layers, x0, x_lo, x_hi, n_steps, step):
    """The rule of gnnb_net_descend in fp64 torch.  Returns (x_best, value, steps_taken, f(x0), f of every step)."""
    x, (f, g) = x0, forward64(layers, x0)
    best, x_best, steps, f0, fs = f, x0, 0, f, []
    for _ in range(n_steps):
        clear_gradient(g)
        x = rule(x, g, x_lo, x_hi, step)
        fn, g = forward64(layers, x)
        assert abs(fn - f) > 1e-9, "two consecutive values of the twin are within 1e-9"
        steps += 1
        fs.append(fn)
        if fn < best:
            best, x_best = fn, x
        if not fn < f:
            break
        f = fn
    return x_best, best, steps, f0, fs


def twin_conditions(name, B):
    """Every assertion of the twin on the case (name, B), and the one the one-step test adds; returns the per-row trajectories."""
    c, out = case(name, B), []
    for b in range(B):
        one = descend64(c.layers[b], c.x0[b], c.x_lo[b], c.x_hi[b], 1, STEP)
        assert one[1] < one[3] - 1e-6, (name, b, "the first step does not lower f by 1e-6", one[3], one[1])
        out.append(descend64(c.layers[b], c.x0[b], c.x_lo[b], c.x_hi[b], 8, STEP))
    return out


# ---- the device -------------------------------------------------------------------------------------------------------------------------
def run(engine, c, n_steps, rows=None, x0=None, step=STEP):
    rows = list(range(c.B)) if rows is None else rows
    dev = engine.device
    x0 = c.x0 if x0 is None else x0
    flat = lambda t: t[rows].reshape(len(rows), -1).contiguous().to(dev)          # noqa: E731
    x_best, value, grad0, steps = engine.net_descend(c.net.fixed, [c.props[b] for b in rows], x0[rows].to(dev), flat(c.x_lo), flat(c.x_hi), n_steps, step,
                                                     want_grad=True, want_steps=True)
    return x_best.cpu().reshape((len(rows),) + tuple(c.net.shape)), value.cpu(), grad0.cpu().reshape((len(rows),) + tuple(c.net.shape)), steps.cpu()


def net_eval(engine, c, x, rows=None):
    rows = list(range(c.B)) if rows is None else rows
    return engine.net_eval(c.net.fixed, [c.props[b] for b in rows], x.to(engine.device)).cpu()


@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("name", NETS)
def test_grad0_against_autograd_and_zero_steps(name, B, engine):
    """g(x0) within 1e-9 max |g64| of autograd's (frontier_net_eval's bar), exactly 0 where autograd's is exactly 0 (kwg_gap: pixels no
    window reads); with n_steps = 0 x_best is x0 and value gnnb_net_eval(x0), bit for bit, and no step was taken."""
    c = case(name, B)
    x_best, value, grad0, steps = run(engine, c, 0)
    worst = 0.0
    for b in range(B):
        _, g64 = forward64(c.layers[b], c.x0[b])
        scale = float(g64.abs().max())
        assert scale > 0
        ratio = float((grad0[b] - g64).abs().max()) / scale
        worst = max(worst, ratio)
        print(f"net_descend {name} B {B} row {b}: max |g - g64| / max |g64| = {ratio:.3e}, zeros {int((g64 == 0).sum())} of {g64.numel()}")
        assert bool((grad0[b][g64 == 0] == 0).all()), (name, b)
    margins.record("frontier_net_descend", f"{name}_B{B}", worst_gradient_ratio=worst, tolerance=1e-9)
    assert worst <= 1e-9, (name, worst)
    if name == "kwg_gap":
        assert int((grad0 == 0).sum()) >= grad0.numel() // 2          # stride 3 over a 2x2 kernel reads 4 pixels of 9
    assert torch.equal(x_best.view(torch.int32), c.x0.view(torch.int32))
    assert torch.equal(value.view(torch.int64), net_eval(engine, c, c.x0).view(torch.int64))
    assert steps.tolist() == [0] * B


@pytest.mark.parametrize("name", NETS)
def test_one_step_is_the_rule_per_coordinate(name, engine):
    """step = 1/64: where |g64| > 1e-9 max |g64| the coordinate is the rule's value bit for bit, elsewhere one of its three possible values;
    the seeds make f(x_1) < f(x_0) - 1e-6 (the twin checks), so x_best is x_1."""
    c = case(name)
    x_best, value, _, steps = run(engine, c, 1)
    for b in range(c.B):
        f0, g64 = forward64(c.layers[b], c.x0[b])
        args = (c.x0[b], g64, c.x_lo[b], c.x_hi[b], STEP)
        want = rule(*args)
        f1, _ = forward64(c.layers[b], want)
        assert f1 < f0 - 1e-6, (name, b, f0, f1)
        sure = g64.abs() > 1e-9 * float(g64.abs().max())
        got = x_best[b]
        assert torch.equal(got[sure].view(torch.int32), want[sure].view(torch.int32)), (name, b)
        options = [rule(*args, sign=torch.full_like(g64, s)) for s in (-1.0, 0.0, 1.0)]
        assert bool(((got == options[0]) | (got == options[1]) | (got == options[2])).all()), (name, b)
        assert abs(float(value[b]) - f1) <= 1e-9 * max(1.0, abs(f1)), (name, b, float(value[b]), f1)
    assert steps.tolist() == [1] * c.B


@pytest.mark.parametrize("name", NETS)
def test_eight_steps_follow_the_twin(name, engine):
    c = case(name)
    x_best, value, _, steps = run(engine, c, 8)
    assert torch.equal(value.view(torch.int64), net_eval(engine, c, x_best).view(torch.int64))      # value == gnnb_net_eval(x_best), bit for bit
    f0 = net_eval(engine, c, c.x0)
    assert bool((value <= f0).all())
    assert bool((x_best.double() >= c.x_lo).all()) and bool((x_best.double() <= c.x_hi).all())
    assert int(steps.max()) <= 8 and int(steps.min()) >= 1
    for b, (_, want, n, _, fs) in enumerate(twin_conditions(name, c.B)):
        print(f"net_descend {name} row {b}: f0 {float(f0[b]):.12g} device {float(value[b]):.15g} twin {want:.15g} steps {int(steps[b])} / {n} twin values {fs}")
        assert abs(float(value[b]) - want) <= 1e-9 * max(1.0, abs(want)), (name, b, float(value[b]), want)
        assert int(steps[b]) == n, (name, b)


BIG_STEP = 0.5                      # half the box per step overshoots: the twin stops rows of every network before the eighth step


def big_step_twin(name):
    c = case(name)
    out = [descend64(c.layers[b], c.x0[b], c.x_lo[b], c.x_hi[b], 8, BIG_STEP) for b in range(c.B)]
    assert min(o[2] for o in out) < 8, (name, "no row of the twin stops early")
    return out


@pytest.mark.parametrize("name", NETS)
def test_the_stop_rule_follows_the_twin(name, engine):
    """step = 1/2: a row stops at the first step that does not lower f, its best point is an earlier one, and both are the twin's."""
    c = case(name)
    x_best, value, _, steps = run(engine, c, 8, step=BIG_STEP)
    assert torch.equal(value.view(torch.int64), net_eval(engine, c, x_best).view(torch.int64))
    assert bool((x_best.double() >= c.x_lo).all()) and bool((x_best.double() <= c.x_hi).all())
    for b, (_, want, n, _, fs) in enumerate(big_step_twin(name)):
        print(f"net_descend {name} step 1/2 row {b}: device {float(value[b]):.15g} twin {want:.15g} steps {int(steps[b])} / {n}")
        assert abs(float(value[b]) - want) <= 1e-9 * max(1.0, abs(want)), (name, b, float(value[b]), want)
        assert int(steps[b]) == n, (name, b)


@pytest.mark.parametrize("name", ["kwg_rect", "kwg_mlp"])
def test_a_row_alone_is_its_row_of_the_batch_and_a_nan_row_stays_alone(name, engine):
    c = case(name)
    batch = run(engine, c, 8)
    for b in range(c.B):
        alone = run(engine, c, 8, rows=[b])
        for got, want in zip(alone, batch):
            assert torch.equal(got.contiguous().view(torch.uint8), want[b:b + 1].contiguous().view(torch.uint8)), (name, b)
    x0 = c.x0.clone()
    x0[2].reshape(-1)[7] = float("nan")
    x_best, value, _, steps = run(engine, c, 8, x0=x0)
    assert int(steps[2]) == 0
    assert torch.equal(x_best[2].view(torch.int32), x0[2].view(torch.int32))
    for b in (0, 1, 3, 4):
        assert torch.equal(x_best[b], batch[0][b]) and float(value[b]) == float(batch[1][b]) and int(steps[b]) == int(batch[3][b]), (name, b)


def test_limits_are_refused(engine):
    c = case("kwg_mlp")
    dev = engine.device
    args = (c.net.fixed, c.props, c.x0.to(dev), c.x_lo.reshape(c.B, -1).to(dev), c.x_hi.reshape(c.B, -1).to(dev))
    for kw, word in (({"n_steps": -1}, "n_steps = -1"), ({"n_steps": 1, "step": 0.0}, "step = 0"), ({"n_steps": 1, "step": 1.5}, "step = 1.5"),
                     ({"n_steps": 1, "step": float("nan")}, "step = nan")):
        with pytest.raises(RuntimeError, match="gnnb_net_descend.*" + word):
            engine.net_descend(*args, **kw)
    with pytest.raises(RuntimeError, match="gnnb_net_descend.*workspace"):
        engine.net_descend(*args, n_steps=1, workspace=torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="gnnb_net_descend.*overlap"):
        engine.net_descend(*args, n_steps=1, x_best=args[2].reshape(c.B, -1))
    engine.net_descend(*args, n_steps=1, step=1.0)                      # the upper end of the range is inside it
    from gnn_branching_amd.engine import ScorerEngine
    fresh = ScorerEngine(None)                                           # GNNB_E_STATE before bind, and no workspace to size
    assert fresh.lib.gnnb_net_descend_workspace_bytes(fresh.h, 1) == 0
    one = C.c_void_p(8)
    assert fresh.lib.gnnb_net_descend(fresh.h, one, one, one, one, one, 1, 1, 0.5, one, one, None, None, one, 8, None) == -3
    assert b"gnnb_net_descend" in _lib.load().gnnb_last_error()
