"""-m gpu: the device pack builder (gnnb_k_repack.h) and repack mode 1 of the learning steps.

The kernels run the shared fold and emit functions of gnnb_pack.h; tests/test_repack_cpu.py compares those with build_packs on the CPU,
this file compares the device execution with the CPU execution of the same code bit for bit, and the steps of the two modes with each
other.  Network kwg_mlp (the pack image does not depend on the bound network), K = 5."""
import ctypes as C
import json
import os
import subprocess
import time

import numpy as np
import pytest
import torch

from tests import margins, test_online_gradients as tog
from tests.common import score_tol, state_of
from tests.test_gpu_imitation import device_batch, id_case
from tests.test_online_gradients import bits
from tests.test_repack_cpu import BLOBS, CSRC, PACK_NAMES, blob_of, crafted_blob

pytestmark = pytest.mark.gpu
I32, F32, F64 = torch.int32, torch.float32, torch.float64
E_INVALID, E_STATE = -1, -3
ROWS = [[3], [3, 0, 4]]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("repack") / "libgnnb_repacktest.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(CSRC, "gnnb_repack_test.cpp")])
    lib = C.CDLL(so)
    lib.gnnb_pt_repack.restype = C.c_size_t
    lib.gnnb_pt_repack.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    return lib


def engine(repack=None, state=None, lr=1e-3):
    """An engine with a trainer, bound to the case's network.  repack None: gnnb_online_set_repack is never called."""
    from gnn_branching_amd.engine import ScorerEngine
    eng = ScorerEngine(state_of("random") if state is None else state, T=2)
    eng.online_create(lr, 1e-4) if repack is None else eng.online_create(lr, 1e-4, repack=repack)
    device_batch(eng, id_case()[0])
    return eng


def images(eng):
    return [eng.pack_image(w) for w in range(14)]


def same_bits(a, b):
    return all(x.size == y.size and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)) and len(a) == len(b)


class Step:
    """One learning step on ``rows`` of the case's batch, every tensor made before the call."""
    def __init__(self, eng, rows, entry):
        batch, table = id_case()
        dev, n = eng.device, len(rows)
        self.eng, self.entry, self.batch = eng, entry, batch
        self.cb, self.keep = device_batch(eng, batch)
        self.rows = torch.tensor(rows, dtype=I32).to(dev)
        self.table = torch.from_numpy(table).to(dev)
        self.kw = torch.tensor(tog.middle_kw(batch.masks[rows]), dtype=I32).to(dev)
        self.imp = torch.tensor([0.1 + 0.1 * i for i in range(n)], dtype=F32).to(dev)
        self.loss = torch.full((n,), -7.0, dtype=F32, device=dev)
        self.status = torch.zeros(1, dtype=I32, device=dev)
        torch.cuda.synchronize()

    def __call__(self, apply=True):
        K = self.batch.batch_size
        if self.entry == "online":
            self.eng.online_step_rows(self.cb, K, self.rows, self.kw, self.imp, loss=self.loss, status=self.status, apply=apply)
        else:
            self.eng.imitation_step_rows(self.cb, K, self.rows, self.table, 1.0, loss=self.loss, status=self.status, apply=apply)

    def result(self):
        torch.cuda.synchronize()
        return self.loss.cpu().numpy(), int(self.status.cpu()[0]), self.eng.online_grad(), self.eng.get_weights()


def forward(eng):
    res = eng.forward(*id_case()[0].forward_args())
    return res.scores.cpu().numpy(), res.decisions.cpu().numpy()


def state_from(blob):
    out, o = {}, 0
    for k, v in state_of("random").items():
        v = np.asarray(v)
        out[k] = blob[o:o + v.size].reshape(v.shape).copy()
        o += v.size
    assert o == blob.size
    return out


# ---- 1. device against host execution of the same code ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BLOBS)
def test_the_device_image_is_the_cpu_run_of_the_same_code(name, shim):
    blob = crafted_blob() if name == "crafted" else blob_of(state_of(name))
    eng = engine("device")
    from gnn_branching_amd import _lib
    with torch.cuda.device(eng.device):
        _lib.check(eng.lib.gnnb_set_weights(eng.h, blob.ctypes.data_as(C.c_void_p), blob.size), "gnnb_set_weights")      # d_w := blob
        _lib.check(eng.lib.gnnb_debug_poison_packs(eng.h), "gnnb_debug_poison_packs")
    assert all(np.isnan(p).all() for p in images(eng))
    eng.repack()
    for which, pack in enumerate(PACK_NAMES):
        got = eng.pack_image(which)
        want = np.zeros(got.size, np.float32)
        assert shim.gnnb_pt_repack(blob.ctypes.data, which, want.ctypes.data, want.size) == got.size
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), pack
    assert bits(eng.get_weights()).tolist() == bits(blob).tolist()


# ---- 2. mode 0 is untouched -------------------------------------------------------------------------------------------------------------
def test_mode_0_is_the_step_of_a_handle_that_never_chose():
    a, b = engine(None), engine("device")
    b.set_repack("host")                      # there and back: the packs come from the host builder again
    assert same_bits(images(a), images(b))
    out = []
    for eng in (a, b):
        s = Step(eng, [3, 0, 4], "imitation")
        s()
        out.append(s.result() + (images(eng),) + forward(eng))
    for x, y in zip(out[0][:1] + out[0][2:4], out[1][:1] + out[1][2:4]):
        assert bits(x).tolist() == bits(y).tolist()
    assert out[0][1] == out[1][1] == 0
    assert same_bits(out[0][4], out[1][4])
    assert bits(out[0][5]).tolist() == bits(out[1][5]).tolist() and out[0][6].tolist() == out[1][6].tolist()


# ---- 3. a step in mode 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["online", "imitation"])
@pytest.mark.parametrize("rows", ROWS, ids=["one", "three"])
def test_a_step_in_mode_1(rows, entry):
    from oracle import gnn_oracle
    host, dev = engine("host"), engine("device")
    w0 = host.get_weights()
    res = []
    for eng in (host, dev):
        s = Step(eng, rows, entry)
        s()
        res.append(s.result())
    (hl, hs, hg, hw), (dl, ds, dg, dw) = res
    assert hs == ds == 0
    assert bits(hl).tolist() == bits(dl).tolist() and bits(hg).tolist() == bits(dg).tolist() and bits(hw).tolist() == bits(dw).tolist()
    assert (bits(hw) != bits(w0)).any() and np.abs(hg).max() > 0
    fresh = engine("device")
    fresh.set_weights(dw)
    assert same_bits(images(dev), images(fresh))
    sd, dd = forward(dev)
    sf, df = forward(fresh)
    assert bits(sd).tolist() == bits(sf).tolist() and dd.tolist() == df.tolist()
    # both modes' scores against the oracle at the new parameters, under the bar of tests/test_gpu_parity.py
    sh, dh = forward(host)
    batch = id_case()[0]
    with torch.no_grad():
        want = gnn_oracle.padded_scores(gnn_oracle.oracle_forward(state_from(dw), *batch.forward_args()), batch.masks).numpy()
    fin = np.isfinite(want)
    tol = score_tol("random", want[fin])
    err_h, err_d = float(np.abs(sh[fin] - want[fin]).max()), float(np.abs(sd[fin] - want[fin]).max())
    gap = float(np.abs(sh[fin] - sd[fin]).max())
    margins.record("repack", f"kwg_mlp_{entry}_rows{len(rows)}", max_err_host=err_h, max_err_device=err_d, max_gap_host_device=gap, tol=tol,
                   n_pack_floats_differing=int(sum((x.view(np.uint32) != y.view(np.uint32)).sum() for x, y in zip(images(host), images(dev)))))
    print(json.dumps({"case": f"{entry}_rows{len(rows)}", "err_host": err_h, "err_device": err_d, "gap": gap, "tol": tol}))
    assert np.array_equal(np.isfinite(sh), fin) and np.array_equal(np.isfinite(sd), fin)
    assert err_h <= tol and err_d <= tol


# ---- 4. the call does not wait ----------------------------------------------------------------------------------------------------------
def occupied(eng, ms=300.0):
    st = torch.cuda.current_stream().cuda_stream
    assert eng.lib.gnnb_debug_occupy(1, 64, 0, ms, C.c_void_p(st)) == 0


def test_a_step_in_mode_1_returns_while_the_stream_is_busy():
    eng = engine("device")
    s = Step(eng, [3, 0, 4], "imitation")
    s()                                       # the first step allocates (arena, the network's weights): not timed
    torch.cuda.synchronize()
    with torch.cuda.device(eng.device):
        occupied(eng)
        t0 = time.perf_counter()
        s()
        t1 = time.perf_counter()
        eng.repack()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        print(json.dumps({"step_call_s": t1 - t0, "repack_call_s": t2 - t1, "drain_s": t3 - t2}))
        margins.record("repack", "no_wait_probe", step_call_s=t1 - t0, repack_call_s=t2 - t1, drain_s=t3 - t2)
        assert t1 - t0 < 0.150 and t2 - t1 < 0.150
        assert t3 - t0 >= 0.25                # the stream really was held behind the calls
        eng.set_repack("host")                # the probe tells the two apart: the same call in mode 0 waits for the stream
        occupied(eng)
        t0 = time.perf_counter()
        s()
        t1 = time.perf_counter()
        assert t1 - t0 >= 0.300
    assert s.result()[1] == 0


def test_the_host_readers_wait_for_a_step_that_was_only_issued():
    """A mode-1 step on a side stream (non-blocking: a plain copy does not wait for it) behind a kernel that holds the stream:
    online_grad and get_weights, called with no synchronise of the caller's, return what the finished step leaves."""
    ref = engine("host")
    s = Step(ref, [3, 0, 4], "imitation")
    s()
    _, _, want_g, want_w = s.result()
    eng = engine("device")
    s = Step(eng, [3, 0, 4], "imitation")
    side = torch.cuda.Stream(device=eng.device)
    with torch.cuda.device(eng.device), torch.cuda.stream(side):
        occupied(eng, 100.0)
        s()
        g = eng.online_grad()
        w = eng.get_weights()
    assert bits(g).tolist() == bits(want_g).tolist() and bits(w).tolist() == bits(want_w).tolist()
    torch.cuda.synchronize()


# ---- 5. two steps back to back ----------------------------------------------------------------------------------------------------------
def test_two_steps_back_to_back_equal_two_steps_with_a_wait_between():
    out = []
    for wait in (False, True):
        eng = engine("device")
        a, b = Step(eng, [3, 0, 4], "imitation"), Step(eng, [1, 2], "online")
        a()
        torch.cuda.synchronize()              # (the first step of an engine allocates)
        a()
        if wait:
            torch.cuda.synchronize()
            eng.get_weights()
        b()
        out.append((a.result(), b.result(), images(eng)))
    for x, y in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert same_bits(out[0][2], out[1][2])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gnn_branching_amd.engine import ScorerEngine
    bare = ScorerEngine(state_of("random"), T=2)
    lib = bare.lib
    buf = np.zeros(70000, np.float32)
    n = C.c_size_t(0)
    assert lib.gnnb_online_set_repack(bare.h, 1) == E_STATE and b"gnnb_online_set_repack: no trainer" in lib.gnnb_last_error()
    assert lib.gnnb_repack(bare.h, None) == E_STATE and b"gnnb_repack: no trainer" in lib.gnnb_last_error()
    assert lib.gnnb_online_set_repack(None, 0) == E_INVALID and lib.gnnb_repack(None, None) == E_INVALID
    assert lib.gnnb_pack_image(None, 0, buf.ctypes.data, buf.size, C.byref(n)) == E_INVALID
    for which in (-1, 14):
        assert lib.gnnb_pack_image(bare.h, which, buf.ctypes.data, buf.size, C.byref(n)) == E_INVALID
        assert b"gnnb_pack_image: which" in lib.gnnb_last_error()
    assert lib.gnnb_pack_image(bare.h, 2, buf.ctypes.data, 62271, C.byref(n)) == E_INVALID and n.value == 62272
    assert b"gnnb_pack_image: room for 62271" in lib.gnnb_last_error()
    assert lib.gnnb_pack_image(bare.h, 2, buf.ctypes.data, 62272, C.byref(n)) == 0      # (a handle without a trainer has packs too)
    with pytest.raises(RuntimeError, match="online_create"):
        bare.set_repack("device")
    with pytest.raises(RuntimeError, match="online_create"):
        bare.repack()
    eng = engine(None)
    before = images(eng)
    assert lib.gnnb_online_set_repack(eng.h, 2) == E_INVALID and b"mode = 2" in lib.gnnb_last_error()
    assert lib.gnnb_online_set_repack(eng.h, -1) == E_INVALID
    for bad in ("gpu", 1, None):
        with pytest.raises(ValueError, match="repack"):
            eng.set_repack(bad)
        with pytest.raises(ValueError, match="repack"):
            eng.online_create(repack=bad)
    assert same_bits(before, images(eng)) and eng.repack_mode == "host"
    eng.set_repack("device")
    eng.online_create()                       # a new trainer: the mode is 0 again, the packs the host builder's
    assert eng.repack_mode == "host" and same_bits(before, images(eng))
