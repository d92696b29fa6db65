"""The walk of the bound network (gnnb_k_net.h: k_net_eval, k_net_descend and k_net_descend_tile are wrappers of ONE template) computes,
bit for bit, what the library computed while the scalar and the S-wide walk were two texts.

tests/test_gpu_net_starts.py holds gnnb_net_descend_starts to gnnb_net_descend: since the fold, two instantiations of one template.  The
anchor outside it is tests/golden/net_walk_parent.npz, recorded once with the library of the commit before the fold
(tools/net_walk_record.py, which imports the cases and the run from this file).  Per case of tests/test_gpu_net_descend.py -- the six kwg_*
networks, their seeds, B = 5 and B = 1 -- it holds

  * gnnb_net_eval(x0);
  * gnnb_net_descend at (n_steps, step) = (0, 1/64), (1, 1/64), (8, 1/64), (8, 1/2): value, steps, x_best, grad0;
  * the same at (8, 1/64) with a NaN planted in one row's coordinate 7 (row 2; row 0 at B = 1);
  * gnnb_net_descend_starts with 5 and 9 starts (gnnb_net_starts, R = 4 and 8, the seed of tests/test_gpu_net_starts.py) at (8, 1/2):
    index, value, every start's value and steps, x_best -- once on the starts as generated, once with a NaN planted in coordinate 7 of a
    start in mid-tile (start 2 of 5, start 5 of 9).

Values, steps and indices are stored raw.  Points and gradients are stored as one 64-bit signature per row (a position-weighted sum of
the row's bit patterns with odd weights, so any changed bit of any coordinate changes it): grad0 alone is 167 KB of fp64 mantissas, more
than the largest fixture committed.  Each case also carries SHA-256 digests of its inputs -- the network's weights, x0, the box, the
property rows -- and the test asserts those first: a changed input fails as such and never passes for a changed kernel."""
from functools import lru_cache
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.common import GOLDEN, register_kw_archs, register_toy_archs
from tests.test_gpu_net_descend import BIG_STEP, NETS, STEP, case, net_eval, run
from tests.test_gpu_net_starts import SEED, descend_starts, make_starts

gpu = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "net_walk_parent.npz")
BS = (5, 1)
DESCENTS = ((0, STEP), (1, STEP), (8, STEP), (8, BIG_STEP))
STARTS = {5: 2, 9: 5}               # n_starts -> the start that gets the NaN: in mid-tile at 4 starts per workgroup
NAN_COORD = 7
GOLDEN_RATIO = np.uint64(0x9E3779B97F4A7C15)


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    return ScorerEngine(None)


def signatures(t, lead=1):
    """fp32 or fp64 tensor, its first ``lead`` dimensions counting rows -> uint64 per row: sum over the row of bit pattern x odd 64-bit
    weight (mod 2^64)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    a = a.reshape(a.shape[:lead] + (-1,))
    bits = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).astype(np.uint64)
    weights = (2 * np.arange(a.shape[-1], dtype=np.uint64) + 1) * GOLDEN_RATIO
    with np.errstate(over="ignore"):
        return (bits * weights).sum(-1, dtype=np.uint64)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def input_digests(name, B):
    """{what: SHA-256} of the case's inputs: weights blob, x0, box, property rows."""
    c = case(name, B)
    return {"weights": digest(*[p for l in c.net.fixed for p in l.parameters()]), "x0": digest(c.x0), "box": digest(c.x_lo, c.x_hi),
            "props": digest(*[p for l in c.props for p in l.parameters()])}


def run_case(engine, name, B):
    """{key: array} of one case on the library in use."""
    c, out = case(name, B), {}

    def descent(key, n_steps, step, x0=None):
        x_best, value, grad0, steps = run(engine, c, n_steps, x0=x0, step=step)
        out.update({f"{key}/value": value.numpy(), f"{key}/steps": steps.numpy(), f"{key}/x_sig": signatures(x_best),
                    f"{key}/grad_sig": signatures(grad0)})

    out["eval"] = net_eval(engine, c, c.x0).numpy()
    for i, (n_steps, step) in enumerate(DESCENTS):
        descent(f"descend{i}", n_steps, step)
    x0 = c.x0.clone()
    x0[min(2, B - 1)].reshape(-1)[NAN_COORD] = float("nan")
    descent("nan_row", 8, STEP, x0=x0)
    for n, mid in STARTS.items():
        starts = make_starts(engine, c, n - 1, seed=SEED)
        poisoned = starts.clone()
        poisoned[:, mid, NAN_COORD] = float("nan")
        out[f"starts{n}/start_sig"] = signatures(starts, lead=2)
        for key, pts in ((f"starts{n}", starts), (f"starts{n}_nan", poisoned)):
            x_best, value, index, values, steps = descend_starts(engine, c, pts, 8, BIG_STEP)
            out.update({f"{key}/index": index.numpy(), f"{key}/value": value.numpy(), f"{key}/values": values.numpy(), f"{key}/steps": steps.numpy(),
                        f"{key}/x_sig": signatures(x_best)})
    return out


@lru_cache(None)
def recorded():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()      # (a NaN equals itself here)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", NETS)
def test_inputs_are_the_recorded_ones(name, B):
    """No GPU needed: the digests of what the cases are built from."""
    want = recorded()
    for what, d in input_digests(name, B).items():
        assert str(want[f"{name}/B{B}/inputs/{what}"]) == d, (name, B, what)


@gpu
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", NETS)
def test_bit_identical_to_the_recorded_parent(name, B, engine):
    want = recorded()
    for what, d in input_digests(name, B).items():                # first, and a failure: a changed input is no changed kernel
        assert str(want[f"{name}/B{B}/inputs/{what}"]) == d, (name, B, what, "the case's inputs changed: the fixture does not apply")
    got = run_case(engine, name, B)
    keys = [k for k in want if k.startswith(f"{name}/B{B}/") and "/inputs/" not in k]
    assert sorted(keys) == sorted(f"{name}/B{B}/{k}" for k in got)
    for k, v in got.items():
        assert same_bits(v, want[f"{name}/B{B}/{k}"]), (name, B, k, v, want[f"{name}/B{B}/{k}"])
    nan_start = {n: got[f"starts{n}_nan/values"][:, mid] for n, mid in STARTS.items()}
    assert all(np.isnan(v).all() for v in nan_start.values()) and not np.isnan(got["nan_row/value"]).any()      # (the two conventions, recorded)
