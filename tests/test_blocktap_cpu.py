"""The block form of a forward conv tile on v_mfma_f32_4x4x1_16b_f32 (gnnb_k_gather.h gather_tile16_block), emulated in numpy lane for lane:

  A  lane l = 4 b + i   -> block b, row i        (one float per lane)
  B  lane l = 4 b + j   -> block b, column j
  D  lane l = 4 b + j, register v -> block b, row v, column j:   D[b][v][j] += A[b][v] * B[b][j]

Block b holds channels 4 b .. 4 b + 3 of ONE source row, the four columns the four destination channels of a group at ONE position.  The
emulation walks every position's own kh x kw x Cs slots and is checked (1) against a plain conv aggregate on edge 1 of cifar_base_kw, on a
5 x 5 pad-0 edge and on an edge narrower than one tile, and (2) bit for bit against the 16-column form's fma chain over the padded union
window, with the host-built tap image of gnnb_pack.h (blocktap_image) -- float32 fma emulated in float64, one rounding per link."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn_branching_amd", "csrc")


@pytest.fixture(scope="module")
def btlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("blocktap") / "libgnnb_blocktaptest.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(CSRC, "gnnb_blocktap_test.cpp")])
    return C.CDLL(so)


def host_image(btlib, w, h_in, w_in, stride, pad):
    """(takes the block form?, geometry dict, image [NCG][ncy][4][4][4] or None) as bind builds them for edge 1."""
    c_out, c_in, kh, kw = w.shape
    w = np.ascontiguousarray(w, np.float32)
    geom = np.zeros(9, np.int32)
    img = np.zeros(c_out // 8 * c_in * kh * 64 + 64, np.float32)
    r = btlib.gnnb_bt_image(C.c_void_p(w.ctypes.data), c_in, h_in, w_in, c_out, kh, kw, stride, pad, C.c_void_p(geom.ctypes.data),
                            C.c_void_p(img.ctypes.data), C.c_size_t(img.size))
    g = dict(zip(["lanes", "CT", "PY", "PX", "NCG", "K2", "WY", "WX", "ncy"], (int(v) for v in geom)))
    return r, g, (img[:g["NCG"] * g["ncy"] * 64].reshape(g["NCG"], g["ncy"], 4, 4, 4) if r == 1 else None)


def fma32(a, b, c):
    """float32 fma, emulated: the product of two float32 is exact in float64; one rounding of the sum per link."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def mfma_4x4x1_16b(a, b, d):
    """One instruction.  a, b: (64,) float32 by lane; d: (64, 4) float32 by lane and register.  Returns the new d."""
    lane = np.arange(64)
    blk, col = lane >> 2, lane & 3
    out = d.copy()
    for v in range(4):
        out[:, v] = fma32(a[4 * blk + v], b[4 * blk + col], d[:, v])      # D[b][v][j] += A[b][v] B[b][j]
    return out


def block_form_aggregate(w, mu, stride, pad, image=None):
    """The aggregate (c_out, h_out, w_out, 64) of a forward conv edge from source rows mu (c_in, h_in, w_in, 64) the way the block form computes
    it: per position and group of four output channels one accumulator, lane = channel of the source row, taps in (cs, ky, kx) order.
    image: blocktap_image of the edge (its taps are then read from it: [cg][cs kh + ky][2 p + gr][c][kx]), else straight from w."""
    c_out, c_in, kh, kw = w.shape
    _, h_in, w_in, _ = mu.shape
    h_out, w_out = (h_in + 2 * pad - kh) // stride + 1, (w_in + 2 * pad - kw) // stride + 1
    out = np.zeros((c_out, h_out, w_out, 64), np.float32)
    lane = np.arange(64)
    zero_row = np.zeros(64, np.float32)
    for y in range(h_out):
        for x in range(w_out):
            for grp in range(c_out // 4):
                acc = np.zeros((64, 4), np.float32)
                for cs in range(c_in):
                    for ky in range(kh):
                        for kx in range(kw):
                            iy, ix = y * stride - pad + ky, x * stride - pad + kx
                            row = mu[cs, iy, ix] if 0 <= iy < h_in and 0 <= ix < w_in else zero_row      # (the buffer load returns 0 out of range)
                            if image is None:
                                taps = w[4 * grp:4 * grp + 4, cs, ky, kx]
                            else:
                                taps = image[grp // 2, cs * kh + ky, 2 * (x & 1) + (grp & 1), :, kx]
                            acc = mfma_4x4x1_16b(row[lane], taps[lane & 3], acc)
                # lane (b, c), register v = channel 4 b + v of destination channel 4 grp + c
                for c in range(4):
                    out[4 * grp + c, y, x, :] = acc[(lane & 3) == c].reshape(64)
    return out


def conv_aggregate64(w, mu, stride, pad):
    """sum over taps of w[co, ci, ky, kx] * mu[ci, y s - p + ky, x s - p + kx, :] in float64."""
    c_out, c_in, kh, kw = w.shape
    _, h_in, w_in, _ = mu.shape
    h_out, w_out = (h_in + 2 * pad - kh) // stride + 1, (w_in + 2 * pad - kw) // stride + 1
    mp = np.zeros((c_in, h_in + 2 * pad, w_in + 2 * pad, 64))
    mp[:, pad:pad + h_in, pad:pad + w_in] = mu
    out = np.zeros((c_out, h_out, w_out, 64))
    for ky in range(kh):
        for kx in range(kw):
            win = mp[:, ky:ky + stride * h_out:stride, kx:kx + stride * w_out:stride]                 # (c_in, h_out, w_out, 64)
            out += np.einsum("oc,cyxe->oyxe", w[:, :, ky, kx].astype(np.float64), win)
    return out


def union_chain(w, mu, stride, pad, K2):
    """The 16-column form on tile [8, 1, 2]: per destination node the fma chain over the 4 K2 slots of the padded union window (kh x 6 x Cs,
    slot order (cs, wy, wx)), structural zeros and padding included."""
    c_out, c_in, kh, kw = w.shape
    _, h_in, w_in, _ = mu.shape
    h_out, w_out = (h_in + 2 * pad - kh) // stride + 1, (w_in + 2 * pad - kw) // stride + 1
    WX = stride + kw
    out = np.zeros((c_out, h_out, w_out, 64), np.float32)
    zero_row = np.zeros(64, np.float32)
    for y in range(h_out):
        for x in range(w_out):
            px, wx0 = x & 1, (x - (x & 1)) * stride - pad
            for co in range(c_out):
                acc = np.zeros(64, np.float32)
                for k in range(4 * K2):
                    tap, row = np.float32(0), zero_row
                    if k < c_in * kh * WX:
                        cs, wy, wx = k // (kh * WX), (k // WX) % kh, k % WX
                        iy, ix = y * stride - pad + wy, wx0 + wx
                        if 0 <= iy < h_in and 0 <= ix < w_in:
                            row = mu[cs, iy, ix]
                        kx = wx - px * stride
                        if 0 <= kx < kw:
                            tap = w[co, cs, wy, kx]
                    acc = fma32(row, np.full(64, tap, np.float32), acc)
                out[co, y, x] = acc
    return out


def make(c_in, h, w_, c_out, k, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((c_out, c_in, k, k)).astype(np.float32) * np.float32(0.2)
    mu = np.maximum(rng.standard_normal((c_in, h, w_, 64)), 0).astype(np.float32)      # rows of a ReLU embedding: non-negative, many zeros
    return w, mu


CASES = {"edge 1 of cifar_base_kw": (3, 32, 32, 8, 4, 2, 1), "5 x 5, pad 0": (3, 9, 11, 8, 5, 1, 0), "narrower than one tile": (3, 8, 2, 8, 4, 2, 1)}


@pytest.mark.parametrize("case", list(CASES))
def test_lane_map_computes_the_conv_aggregate(case):
    c_in, h, w_, c_out, k, s, p = CASES[case]
    if case.startswith("edge 1"):
        h, w_ = 8, 10                  # the edge's geometry on a smaller image: every kind of tile (corner, border, interior) at a hundredth of the time
    w, mu = make(c_in, h, w_, c_out, k, 1)
    got = block_form_aggregate(w, mu, s, p).astype(np.float64)
    want = conv_aggregate64(w, mu, s, p)
    # fp32 chain of K = c_in k k links: error <= K eps32 sum |a b| (cdna_hip_programming.md section 3 quotes ~1e-7 sum |a b| at K <= 1024)
    bound = c_in * k * k * 2.0 ** -24 * conv_aggregate64(np.abs(w), np.abs(mu), s, p)
    assert got.shape == want.shape and np.all(np.abs(got - want) <= bound + 1e-30), float(np.abs(got - want).max())
    assert float(np.abs(want).max()) > 0.1


@pytest.mark.parametrize("shape", [(6, 12), (4, 4), (2, 4)])
def test_host_image_reproduces_the_union_window_chain_bit_for_bit(btlib, shape):
    """blocktap_image, walked per position in slot order, gives every destination node the bits of the 16-column chain over the 80 padded
    union slots: the links it leaves out have a tap of exactly zero (an image with interior tiles, one tile, a kernel larger than the image)."""
    w, mu = make(3, shape[0], shape[1], 8, 4, 2)
    mu[0, 0, 0, :7] = np.float32(1e-42)                                                  # subnormal rows ride through unflushed
    taken, g, image = host_image(btlib, w, shape[0], shape[1], 2, 1)
    assert taken == 1 and (g["lanes"], g["CT"], g["PY"], g["PX"], g["WX"], g["ncy"], g["K2"]) == (16, 8, 1, 2, 6, 12, 20)
    got = block_form_aggregate(w, mu, 2, 1, image=image)
    want = union_chain(w, mu, 2, 1, g["K2"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_other_first_convolutions_keep_the_16_column_form(btlib):
    for (c_in, h, w_, c_out, k, s, p) in [(3, 12, 20, 8, 5, 1, 2), (3, 32, 32, 16, 4, 2, 1), (3, 34, 10, 8, 4, 2, 1), (3, 20, 14, 8, 2, 3, 0)]:
        w, _ = make(c_in, h, w_, c_out, k, 3)
        taken, g, _ = host_image(btlib, w, h, w_, s, p)
        assert taken == 0 and g["ncy"] == 0, (c_in, h, w_, c_out, k, s, p, g)
