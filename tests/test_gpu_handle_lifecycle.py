"""The life of one handle: what gnnb_bind_network makes is replaced whole by the next bind and by nothing else.

Two of the smallest networks of tests/common.py FWD_ARCHS at B = 2 -- fwg_single (one conv edge under the property layer, L = 1,
R = 512) and fwg_tall (three conv edges and a Linear edge, L = 4, R = 1824) -- bound in turn on ONE engine.  Everything is compared
bit for bit with the same call made earlier on the same engine: a rebind may leave nothing of the other network behind (gather tables,
dense operands, the bias-sum table of edge 1, the fp64 copies, the trainer's edge weights), a refused bind leaves the handle unbound, and
the buffers a call grows on demand (gnnb_forward_host, gnnb_online_step) are reused.  Every refusal here is an error code returned
before any launch."""
import copy
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import synth
from tests.common import FWD_ARCHS, random_state, register_fwd_archs

pytestmark = pytest.mark.gpu
NET_A, NET_B = "fwg_single", "fwg_tall"
BATCH = {NET_A: (5, 0.02), NET_B: (5, 0.002)}          # (seed, eps), as tests/test_gpu_forward_geometry.py draws them
PROPS = [(3, 5), (1, 7), (0, 2), (4, 3)]
GNNB_E_STATE = -3


@lru_cache(None)
def batch_of(name, B=2):
    register_fwd_archs()
    seed, eps = BATCH[name]
    return synth.make_batch(name, B, seed=seed, eps=eps, props=PROPS[:B], input_shape=FWD_ARCHS[name][0])


def new_engine():
    from gnn_branching_amd.engine import ScorerEngine
    return ScorerEngine(random_state())


def forward(eng, batch, layers=None):
    """(scores, decisions) of gnnb_forward as numpy arrays"""
    args = list(batch.forward_args())
    if layers is not None:
        args[5] = layers
    with torch.no_grad():
        res = eng.forward(*args).check()
    return res.scores.cpu().numpy(), res.decisions.cpu().numpy()


def kw_bounds(eng, batch):
    """gnnb_kw_bounds of the batch's input boxes, no node forced: the fp64 bounds of graph layers 1..L+1"""
    R = batch.masks.shape[1]
    res = eng.kw_bounds(batch.layers["fixed_layers"], batch.layers["prop_layers"], batch.lower_bounds_all[0].double(),
                        batch.upper_bounds_all[0].double(), torch.full((batch.batch_size, R), -1, dtype=torch.int8))
    assert res.infeasible.cpu().tolist() == [0] * batch.batch_size
    return [t.cpu() for t in res.lb + res.ub]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))


def test_rebinding_reproduces_the_first_bind():
    eng, a, b = new_engine(), batch_of(NET_A), batch_of(NET_B)
    first, kw_first = forward(eng, a), kw_bounds(eng, a)
    assert np.isfinite(first[0]).any()
    other = forward(eng, b)                               # the detour: fwg_tall on the same handle
    assert other[0].shape != first[0].shape and np.isfinite(other[0]).any()
    assert same(forward(eng, a), first)
    assert all(torch.equal(x, y) for x, y in zip(kw_bounds(eng, a), kw_first))
    assert same(forward(eng, b), other)


def test_a_refused_bind_leaves_the_handle_unbound():
    eng, a = new_engine(), batch_of(NET_A)
    first = forward(eng, a)
    bad = [nn.Flatten(), nn.Linear(3 * 16 * 16, 8), nn.Linear(8, 4), nn.ReLU()]
    with pytest.raises(RuntimeError, match=r"gnnb_bind_network failed \(-1\): layer 2: two linear maps without a ReLU between them"):
        eng.bind(bad, FWD_ARCHS[NET_A][0])
    # straight through the C entry points (ScorerEngine's calls bind first): the state check comes before anything is read
    some = torch.zeros(16, dtype=torch.float32, device=eng.device)
    from gnn_branching_amd import _lib
    empty = _lib.Batch()
    with torch.cuda.device(eng.device):
        rc = eng.lib.gnnb_forward(eng.h, C.byref(empty), 2, some.data_ptr(), some.data_ptr(), some.data_ptr(), some.data_ptr(), 64, None)
    assert rc == GNNB_E_STATE and eng.lib.gnnb_last_error().decode() == "gnnb_forward: call gnnb_bind_network first"
    kb = _lib.KwBatch()
    with torch.cuda.device(eng.device):
        rc = eng.lib.gnnb_kw_bounds(eng.h, C.byref(kb), 2, None, None, None, None, some.data_ptr(), some.data_ptr(), 64, None)
    assert rc == GNNB_E_STATE and eng.lib.gnnb_last_error().decode() == "gnnb_kw_bounds: call gnnb_bind_network first"
    assert eng.lib.gnnb_workspace_bytes(eng.h, 2) == 0
    # the same network again (as new layer objects: the engine skips a bind of the objects it believes bound)
    again = {"fixed_layers": copy.deepcopy(a.layers["fixed_layers"]), "prop_layers": a.layers["prop_layers"]}
    assert same(forward(eng, a, again), first)


def test_the_trainer_survives_a_rebind():
    """The trainer's torch-layout edge weights belong to the bound network, its per-batch buffers are sized by that network's R:
    R = 512, then 1824, then 512 again."""
    eng, a, b = new_engine(), batch_of(NET_A), batch_of(NET_B)
    eng.online_create()

    def step(batch):
        kw = [int(m.nonzero().view(-1)[len(m.nonzero()) // 2]) for m in batch.masks]
        loss, _ = eng.online_step(batch.forward_args(), kw, [0.1, 0.2], apply=False)
        assert np.isfinite(loss).all()
        return loss, eng.online_grad()
    loss_a, grad_a = step(a)
    assert grad_a.any()
    loss_b, grad_b = step(b)
    assert grad_b.any() and not np.array_equal(bits(grad_b), bits(grad_a))
    loss_a2, grad_a2 = step(a)
    assert np.array_equal(bits(loss_a2), bits(loss_a)) and np.array_equal(bits(grad_a2), bits(grad_a))
    h, eng.h = eng.h, None                                # destroy the handle with the trainer alive
    assert eng.lib.gnnb_destroy(h) == 0


def test_host_fed_buffers_grow_and_are_reused():
    eng, four = new_engine(), batch_of(NET_B, 4)
    for batch in (four.slice(0, 1), four, four.slice(0, 1)):          # B = 1, 4, 1
        dec, scores = eng.forward_host(*batch.forward_args(), want_scores=True)
        want_scores, want_dec = forward(eng, batch)
        assert np.array_equal(bits(scores), bits(want_scores)) and np.array_equal(dec, want_dec)
