"""Host logic on the CPU: the operand-order weight packs of gnnb_pack.h, checked by emulating the
gfx950 MFMA lane maps (v_mfma_f32_32x32x2_f32) in numpy against plain matmuls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.common import random_state

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn_branching_amd", "csrc")
LANES = np.arange(64)
J, H = LANES & 31, LANES >> 5


@pytest.fixture(scope="module")
def packlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pack") / "libgnnb_packtest.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(CSRC, "gnnb_pack_test.cpp")])
    lib = C.CDLL(so)
    lib.gnnb_pt_blob_floats.restype = C.c_size_t
    lib.gnnb_pt_pack.restype = C.c_size_t
    lib.gnnb_pt_pack.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    return lib


@pytest.fixture(scope="module")
def packs(packlib):
    sd = random_state()
    blob = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in sd.values()])
    assert blob.size == packlib.gnnb_pt_blob_floats() == 117825
    out = {}
    for which, name in enumerate(["embed", "pre_fwd", "pre_bwd", "pre_inp", "prop", "upd_fwd_e", "upd_fwd_i", "upd_fwd_f", "upd_bwd",
                                  "upd_bwd_b", "upd_inp", "post_inp", "score_b", "score_f"]):
        n = packlib.gnnb_pt_pack(blob.ctypes.data, which, None, 0)
        buf = np.zeros(n, np.float32)
        assert packlib.gnnb_pt_pack(blob.ctypes.data, which, buf.ctypes.data, n) == n
        out[name] = buf
    return sd, out


# ---- numpy model of the wave-level data layout used by the kernels ----
def feat(R, h):
    return 8 * (R >> 2) + 4 * h + (R & 3)


def frag_from_rows(X):
    """(32 nodes, 64 features) -> frag[lane, R]"""
    f = np.zeros((64, 32), np.float64)
    for R in range(32):
        f[:, R] = X[J, feat(R, H)]
    return f


def rows_from_frag(f):
    X = np.zeros((32, 64))
    for R in range(32):
        X[J, feat(R, H)] = f[:, R]
    return X


def mfma(a, b, acc):
    """acc[lane, r] (16 regs) += A(32x2) B(2x32) with the gfx950 operand maps."""
    A = np.zeros((32, 2)); Bm = np.zeros((2, 32))
    A[J, H] = a
    Bm[H, J] = b
    D = A @ Bm
    for r in range(16):
        acc[:, r] += D[(r & 3) + 8 * (r >> 2) + 4 * H, J]


def frag_bias(bl):
    f = np.zeros((64, 32))
    for R in range(32):
        f[:, R] = bl[H * 32 + R]
    return f


def gemm_w64(wl, ksteps, acc, getB):
    for s in range(ksteps):
        for it in range(2):
            a = wl[(((s >> 2) * 2 + it) * 64 + LANES) * 4 + (s & 3)]
            mfma(a, getB(s), acc[:, 16 * it:16 * it + 16])


def bf16_pieces(x):
    """x (float32) -> three bf16-valued float32 arrays, round to nearest even each time (the kernel's v_cvt_pk_bf16_f32 + subtract)."""
    out, r = [], np.asarray(x, np.float32).copy()
    for _ in range(3):
        u = r.view(np.uint32).astype(np.uint64)
        b = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
        out.append(b)
        r = (r - b).astype(np.float32)
    return out


def gemm_w64_bf3(wl, nfrag, acc, getB):
    """numpy model of gemm_w64_bf3 (gnnb.hip): v_mfma_f32_32x32x16_bf16 operand maps, operands in three bf16 pieces, the six
    products of total order <= 4.  wl: the pack as float32 (reinterpreted as 8 bf16 per lane and entry)."""
    w16 = np.ascontiguousarray(wl[:6144 * nfrag]).view(np.uint16).reshape(nfrag * 4, 2, 3, 64, 8)
    wf = (w16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    for fk in range(4 * nfrag):
        xs = [np.stack([pc for pc in bf16_pieces(np.stack([getB(8 * fk + j) for j in range(8)], 1).astype(np.float32))][i], 0)
              for i in range(3)]                                  # xs[piece][lane, j]
        for ot in range(2):
            D = np.zeros((32, 32))
            for pw, px in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):
                A = np.zeros((32, 16)); Bm = np.zeros((16, 32))
                for j in range(8):
                    A[J, 8 * H + j] = wf[fk, ot, pw, LANES, j]
                    Bm[8 * H + j, J] = xs[px][LANES, j]
                D += A @ Bm
            for r in range(16):
                acc[:, 16 * ot + r] += D[(r & 3) + 8 * (r >> 2) + 4 * H, J]


def gemm_small(wl, ksteps, acc, x):
    for s in range(ksteps):
        for it in range(2):
            mfma(wl[(s * 2 + it) * 64 + LANES], x[s], acc[:, 16 * it:16 * it + 16])


def lin(sd, name, x):
    return x @ np.asarray(sd[name + ".weight"], np.float64).T + np.asarray(sd[name + ".bias"], np.float64)


E = "EmbedUpdates.update."


UPD = dict(WA=0, WAS=8192, BA=12288, WCB=12352, BCB=16448, BCBROW=16512, VAW=16576, WAS3=16704, WCB3=16704 + 6144,
           FLOATS3=16704 + 2 * 6144)
# the second half of Wa alone, bf16 x 3: general nodes go through WAS.(r0 x) + Wa[:, 64:].((r1 - r0) x) (PackUpdL3)
UPD.update(WA1S3=UPD["FLOATS3"], FLOATS=UPD["FLOATS3"] + 6144)


@pytest.mark.parametrize("pack,chain,proj", [
    ("upd_fwd_e", ("fc3", "fc3_2", "fc4", "fc4_2"), "inp_f_1"), ("upd_fwd_i", ("fc3", "fc3_2", "fc4", "fc4_2"), "inp_b2_2"),
    ("upd_fwd_f", ("fc3", "fc3_2", "fc4", "fc4_2"), "fc4_2"), ("upd_bwd_b", ("bc3", "bc3_1", "bc4", "bc4_1"), "bc4_1"),
    ("upd_bwd", ("bc3", "bc3_1", "bc4", "bc4_1"), None)])
def test_node_update_chain(packs, pack, chain, proj):
    """k_node_update's folded chain on one tile.  Reference: mu = d(relu(c([relax, b(relu(a([r0 nb, r1 nb])))]))).

    Folds (gnnb_pack.h PackUpd): b feeds c linearly, so Wcb = c[:, 64:].b.W and the cached term is
    P' = c[:, :64].relax + c.b + c[:, 64:].b.b; nodes with r0 == r1 use the summed halves of a; the last layer d is NOT
    applied (the kernel stores E with mu = d(E), deferred into the consumers); and when the aggregate was built from
    rows with a deferred projection p (nb = p.W.G + s.p.b), p.W is folded into a and the s-term is one small k-step."""
    sd, pk = packs
    la, lb_, lc, ld = chain
    rng = np.random.RandomState(7)
    G = rng.standard_normal((32, 64)); relax = rng.standard_normal((32, 64)); sw = rng.standard_normal(32)
    r0 = rng.uniform(0, 1, 32); r1 = 1 - r0
    if proj is None:
        nb = G
    else:
        wp, bp = np.asarray(sd[E + proj + ".weight"], np.float64), np.asarray(sd[E + proj + ".bias"], np.float64)
        nb = G @ wp.T + sw[:, None] * bp[None, :]
    w4, b4 = np.asarray(sd[E + lc + ".weight"], np.float64), np.asarray(sd[E + lc + ".bias"], np.float64)
    bcb = b4 + w4[:, 64:] @ np.asarray(sd[E + lb_ + ".bias"], np.float64)
    Pp = relax @ w4[:, :64].T + bcb                      # what k_pre caches for ambiguous nodes
    p = pk[pack]
    assert p.size == UPD["FLOATS"]
    WA, WAS, BA, WCB, BCB, BCBROW, VAW = (UPD[k] for k in ("WA", "WAS", "BA", "WCB", "BCB", "BCBROW", "VAW"))
    np.testing.assert_allclose(p[BCBROW:BCBROW + 64], bcb, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(rows_from_frag(frag_bias(p[BCB:BCB + 64]))[0], bcb, rtol=1e-6, atol=1e-7)
    if proj is None:
        assert not p[VAW:VAW + 128].any()

    def reference(nb_, r0_, r1_, relax_):
        """the rows the reference would hold BEFORE its last Linear d"""
        e = lin(sd, E + lb_, np.maximum(lin(sd, E + la, np.concatenate([nb_ * r0_[:, None], nb_ * r1_[:, None]], 1)), 0))
        return np.maximum(lin(sd, E + lc, np.concatenate([relax_, e], 1)), 0)

    def tail(Hf, H2):
        Hf = np.maximum(Hf, 0)
        gemm_w64(p[WCB:], 32, H2, lambda s: Hf[:, s])
        return rows_from_frag(np.maximum(H2, 0))
    X = frag_from_rows(G)
    # general nodes: lane half 0 feeds r0.s, half 1 feeds r1.s into the small k-step
    Hf = frag_bias(p[BA:BA + 64])
    gemm_small(p[VAW:], 1, Hf, [np.where(H == 0, r0[J], r1[J]) * sw[J]])
    gemm_w64(p[WA:], 64, Hf, lambda s: X[:, s & 31] * (r0[J] if s < 32 else r1[J]))
    np.testing.assert_allclose(tail(Hf, frag_from_rows(Pp)), reference(nb, r0, r1, relax), atol=2e-5)
    # r0 == r1 nodes without relaxation term: summed halves, P' = bcb, both lane halves feed r0.s
    Hf = frag_bias(p[BA:BA + 64])
    gemm_small(p[VAW:], 1, Hf, [r0[J] * sw[J]])
    gemm_w64(p[WAS:], 32, Hf, lambda s: X[:, s] * r0[J])
    np.testing.assert_allclose(tail(Hf, frag_bias(p[BCB:BCB + 64])), reference(nb, r0, r0, np.zeros_like(relax)), atol=2e-5)
    # the short chain on the bf16 matrix rate (three-piece operands): WAS3 / WCB3 hold the same matrices
    Hf = frag_bias(p[BA:BA + 64])
    gemm_small(p[VAW:], 1, Hf, [r0[J] * sw[J]])
    gemm_w64_bf3(p[UPD["WAS3"]:], 1, Hf, lambda s: X[:, s] * r0[J])
    Hf = np.maximum(Hf, 0)
    H2 = frag_bias(p[BCB:BCB + 64])
    gemm_w64_bf3(p[UPD["WCB3"]:], 1, H2, lambda s: Hf[:, s])
    np.testing.assert_allclose(rows_from_frag(np.maximum(H2, 0)), reference(nb, r0, r0, np.zeros_like(relax)), atol=2e-5)
    # the bf16 x 3 node update (k_node_update, k_gather_update_q): EVERY node -- ambiguous or not -- goes through
    # H = WAS.(r0 x) + Wa[:, 64:].((r1 - r0) x); the second block adds exact zeros for r0 == r1, so a node's result does not depend on
    # whether its tile ran it
    amb = np.arange(32) % 3 == 0                      # a mixed tile: every third node ambiguous (r1 != r0, cached P' row)
    r1m = np.where(amb, r1, r0)
    relaxm = np.where(amb[:, None], relax, 0.0)
    Ppm = relaxm @ w4[:, :64].T + bcb
    Hf = frag_bias(p[BA:BA + 64])
    gemm_small(p[VAW:], 1, Hf, [np.where(H == 0, r0[J], r1m[J]) * sw[J]])
    gemm_w64_bf3(p[UPD["WAS3"]:], 1, Hf, lambda s: X[:, s] * r0[J])
    before = Hf.copy()
    gemm_w64_bf3(p[UPD["WA1S3"]:], 1, Hf, lambda s: X[:, s] * (r1m[J] - r0[J]))
    assert np.array_equal(Hf[~amb[J]], before[~amb[J]])          # exact zeros for the nodes with r0 == r1
    Hf = np.maximum(Hf, 0)
    H2 = frag_from_rows(Ppm)
    gemm_w64_bf3(p[UPD["WCB3"]:], 1, H2, lambda s: Hf[:, s])
    np.testing.assert_allclose(rows_from_frag(np.maximum(H2, 0)), reference(nb, r0, r1m, relaxm), atol=2e-5)


def test_input_update_packs(packs):
    """E_0 = relu(Q + inp_b2[:, 64:].nb) with nb = bc4_1.W.G + s.bc4_1.b.  The 64x64 map is applied on the producer side
    (PackPostInp: rows F = (inp_b2[:, 64:].bc4_1.W).E of layer 1), the input kernels add the aggregate of F and the bias
    small k-step (PackUpdInp VC)."""
    sd, pk = packs
    rng = np.random.RandomState(11)
    Erows = rng.standard_normal((32, 64)); Q = rng.standard_normal((32, 64)); sw = rng.standard_normal(32)
    wp, bp = np.asarray(sd[E + "bc4_1.weight"], np.float64), np.asarray(sd[E + "bc4_1.bias"], np.float64)
    w2 = np.asarray(sd[E + "inp_b2.weight"], np.float64)
    wc = w2[:, 64:] @ wp
    # producer side, natural row order: the flat input update adds the row-major aggregate
    p = pk["post_inp"]
    assert p.size == 8192 + 2 * 6144
    X = frag_from_rows(Erows)
    F = np.zeros((64, 32)); gemm_w64(p[0:], 32, F, lambda s: X[:, s])
    np.testing.assert_allclose(rows_from_frag(F), Erows @ wc.T, atol=2e-5)
    F3 = np.zeros((64, 32)); gemm_w64_bf3(p[8192:], 1, F3, lambda s: X[:, s])          # bf16 x 3 forms of the same two maps
    np.testing.assert_allclose(rows_from_frag(F3), Erows @ wc.T, atol=2e-5)
    Fg3 = np.zeros((64, 32)); gemm_w64_bf3(p[8192 + 6144:], 1, Fg3, lambda s: X[:, s])
    # producer side, gather-permuted rows: stored channel gather_feature(R, h) holds feature frag_feature(R, h)
    Fg = np.zeros((64, 32)); gemm_w64(p[4096:], 32, Fg, lambda s: X[:, s])
    stored = rows_from_frag(Fg)                          # what the producer writes, row-major
    np.testing.assert_allclose(rows_from_frag(Fg3), stored, atol=2e-5)
    want = Erows @ wc.T
    for hh in range(2):
        for R in range(32):
            it, r = R >> 4, R & 15
            g = 2 * ((r & 3) + 8 * (r >> 2) + 4 * hh) + it
            np.testing.assert_allclose(stored[:, g], want[:, feat(R, hh)], atol=2e-5)
    # consumer side: with every node's row equal to its own aggregate (identity edge), H = Q + VC.s + F
    pu = pk["upd_inp"]
    assert pu.size == 128
    Hf = frag_from_rows(Q)
    gemm_small(pu[0:], 1, Hf, [np.where(H == 0, sw[J], 0.0)])
    Hf += frag_from_rows(want)
    nb = Erows @ wp.T + sw[:, None] * bp[None, :]
    np.testing.assert_allclose(rows_from_frag(np.maximum(Hf, 0)), np.maximum(Q + nb @ w2[:, 64:].T, 0), atol=2e-5)


def test_pre_fwd_chain(packs):
    """k_pre, forward: fc1 on the 7 scalar features, then fc1_1 folded into fc4[:, :64] (one 64x64 map), bias = folded bcb."""
    sd, pk = packs
    rng = np.random.RandomState(12)
    f7 = rng.standard_normal((32, 7))
    p = pk["pre_fwd"]
    assert p.size == 512 + 64 + 4096 + 64 + 6144          # + W2 in three bf16 pieces
    f8 = np.concatenate([f7, np.zeros((32, 1))], 1)
    H1 = frag_bias(p[512:576]); gemm_small(p[0:], 4, H1, [f8[J, 2 * s + H] for s in range(4)]); H1 = np.maximum(H1, 0)
    Pf = frag_bias(p[4672:4736]); gemm_w64(p[576:], 32, Pf, lambda s: H1[:, s])
    relax = lin(sd, E + "fc1_1", np.maximum(lin(sd, E + "fc1", f7), 0))
    w4, b4 = np.asarray(sd[E + "fc4.weight"], np.float64), np.asarray(sd[E + "fc4.bias"], np.float64)
    bcb = b4 + w4[:, 64:] @ np.asarray(sd[E + "fc3_2.bias"], np.float64)
    np.testing.assert_allclose(rows_from_frag(Pf), relax @ w4[:, :64].T + bcb, atol=1e-5)
    Pf3 = frag_bias(p[4672:4736]); gemm_w64_bf3(p[4736:], 1, Pf3, lambda s: H1[:, s])          # the same map as three-piece bf16 block
    np.testing.assert_allclose(rows_from_frag(Pf3), relax @ w4[:, :64].T + bcb, atol=1e-5)


def test_pre_bwd_chain(packs):
    """k_pre_bwd: bc1 (7 scalar features, zero-padded k-steps) .. bc2 on [s, -d2 s, d1 s] .. bc4[:, :64]."""
    sd, pk = packs
    rng = np.random.RandomState(2)
    f7 = rng.standard_normal((32, 7)); d1 = rng.uniform(0, 1, 32); d2 = rng.uniform(0, 1, 32)
    p = pk["pre_bwd"]
    W1, B1, W2, B2, W3, B3, W4, B4, W5, B5 = 0, 512, 576, 4672, 4736, 8832, 8896, 21184, 21248, 25344
    W23, W33, W53, W43 = 25408, 25408 + 6144, 25408 + 2 * 6144, 25408 + 3 * 6144      # W2, W3, W5 and the 192-wide W4 in three bf16 pieces
    assert p.size == 25408 + 3 * 6144 + 18432
    f8 = np.concatenate([f7, np.zeros((32, 1))], 1)
    x = [f8[J, 2 * s + H] for s in range(4)]
    H1 = frag_bias(p[B1:B1 + 64]); gemm_small(p[W1:], 4, H1, x); H1 = np.maximum(H1, 0)
    H2 = frag_bias(p[B2:B2 + 64]); gemm_w64(p[W2:], 32, H2, lambda s: H1[:, s]); H2 = np.maximum(H2, 0)
    S = frag_bias(p[B3:B3 + 64]); gemm_w64(p[W3:], 32, S, lambda s: H2[:, s])
    H4 = frag_bias(p[B4:B4 + 64])
    gemm_w64(p[W4:], 96, H4, lambda s: S[:, s & 31] * (1.0 if s < 32 else (-d2[J] if s < 64 else d1[J])))
    H4 = np.maximum(H4, 0)
    Pb = frag_bias(p[B5:B5 + 64]); gemm_w64(p[W5:], 32, Pb, lambda s: H4[:, s])     # bc2_1 folded into bc4[:, :64]
    got = rows_from_frag(Pb)
    s_ = lin(sd, E + "bc1_2", np.maximum(lin(sd, E + "bc1_1", np.maximum(lin(sd, E + "bc1", f7), 0)), 0))
    relax = lin(sd, E + "bc2_1", np.maximum(lin(sd, E + "bc2", np.concatenate([s_, s_ * -d2[:, None], s_ * d1[:, None]], 1)), 0))
    w4, b4 = np.asarray(sd[E + "bc4.weight"], np.float64), np.asarray(sd[E + "bc4.bias"], np.float64)
    bcb = b4 + w4[:, 64:] @ np.asarray(sd[E + "bc3_1.bias"], np.float64)      # folded bias (PackUpd)
    np.testing.assert_allclose(got, relax @ w4[:, :64].T + bcb, atol=1e-5)
    # the same chain on the bf16 matrix rate: the 64x64 blocks and the 192-wide W4 as three input fragments
    H2 = frag_bias(p[B2:B2 + 64]); gemm_w64_bf3(p[W23:], 1, H2, lambda s: H1[:, s]); H2 = np.maximum(H2, 0)
    S = frag_bias(p[B3:B3 + 64]); gemm_w64_bf3(p[W33:], 1, S, lambda s: H2[:, s])
    H4 = frag_bias(p[B4:B4 + 64])
    gemm_w64_bf3(p[W43:], 3, H4, lambda s: S[:, s & 31] * (1.0 if s < 32 else (-d2[J] if s < 64 else d1[J])))
    H4 = np.maximum(H4, 0)
    Pb = frag_bias(p[B5:B5 + 64]); gemm_w64_bf3(p[W53:], 1, Pb, lambda s: H4[:, s])
    np.testing.assert_allclose(rows_from_frag(Pb), relax @ w4[:, :64].T + bcb, atol=1e-5)


def test_embed_and_score_packs(packs):
    sd, pk = packs
    rng = np.random.RandomState(3)
    f3 = rng.standard_normal((32, 3))
    p = pk["embed"]
    # inp_f only, row-major for the VALU kernel: inp_f_1 is deferred into the forward update of ReLU layer 1
    assert p.size == 256
    np.testing.assert_array_equal(p[:192].reshape(64, 3), np.asarray(sd[E + "inp_f.weight"]))
    np.testing.assert_array_equal(p[192:256], np.asarray(sd[E + "inp_f.bias"]))
    # score head: per-lane partial dot over the lane's 32 features + the other half
    mu = rng.standard_normal((32, 64))
    live = (rng.uniform(0, 1, 32) > 0.3).astype(np.float64)
    for name, proj in (("score_b", "bc4_1"), ("score_f", "fc4_2")):
        # the rows hold E with mu = (Wp.E + bp).live
        wp, bp = np.asarray(sd[E + proj + ".weight"], np.float64), np.asarray(sd[E + proj + ".bias"], np.float64)
        Erows = mu * live[:, None]
        mu_true = (Erows @ wp.T + bp) * live[:, None]
        p = pk[name]
        X = frag_from_rows(Erows)
        Hs = frag_bias(p[4096:4160])
        gemm_small(p[4228:], 1, Hs, [np.where(H == 0, live[J], 0.0)])
        gemm_w64(p[0:], 32, Hs, lambda s: X[:, s]); Hs = np.maximum(Hs, 0)
        ws = p[4160:4224]
        part = np.array([sum(Hs[l, R] * ws[H[l] * 32 + R] for R in range(32)) for l in range(64)])
        score = part[:32] + part[32:] + p[4224]
        want = lin(sd, "ComputeFinalScore.fscore", np.maximum(lin(sd, "ComputeFinalScore.fnode", mu_true), 0))[:, 0]
        np.testing.assert_allclose(score, want, atol=2e-5)


def test_prop_pack_is_transposed(packs):
    sd, pk = packs
    p = pk["prop"]
    w2 = np.asarray(sd[E + "out2.weight"])
    np.testing.assert_array_equal(p[320:320 + 64 * 64].reshape(64, 64), w2[:, :64].T)
    # second half: folded with fc4_2 (deferred in the rows of the top ReLU layer), bias vector V2
    wp, bp = np.asarray(sd[E + "fc4_2.weight"], np.float64), np.asarray(sd[E + "fc4_2.bias"], np.float64)
    np.testing.assert_allclose(p[320 + 64 * 64:320 + 128 * 64].reshape(64, 64), (w2[:, 64:].astype(np.float64) @ wp).T, atol=1e-6)
    v2 = p[320 + 128 * 64 + 64 + 64 * 64 + 64:][:64]
    np.testing.assert_allclose(v2, w2[:, 64:].astype(np.float64) @ bp, atol=1e-6)
    np.testing.assert_array_equal(p[0:256].reshape(4, 64), np.asarray(sd[E + "out1.weight"]).T)


# ---- MFMA gather tables (conv / conv-transpose message passing as dense local blocks) ----
GEOM = ["N", "C", "H", "W", "CT", "PY", "PX", "ay", "ax", "NBY", "NBX", "NCG", "TPS", "K2", "Hs", "Ws", "Ns",
        "ystep", "ybase", "xstep", "xbase", "WY", "WX", "normalise", "n_cmat", "n_koff", "lanes"]


def build_gather(packlib, w, h_in, w_in, stride, pad, direction, normalise, allow16=0, may_be_missing=False):
    """(geometry, tap matrix, offsets, MFMAs per sample) of gnnb_pack.h build_gather; None where it finds no tiling (may_be_missing)."""
    c_out, c_in, kh, kw = w.shape
    packlib.gnnb_pt_gather.restype = C.c_long
    packlib.gnnb_pt_gather.argtypes = [C.c_void_p] + [C.c_int] * 11 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    w = np.ascontiguousarray(w, np.float32)
    geom = np.zeros(27, np.int32)
    cost = packlib.gnnb_pt_gather(w.ctypes.data, c_in, h_in, w_in, c_out, kh, kw, stride, pad, direction, normalise, allow16,
                                  geom.ctypes.data, None, 0, None, 0)
    if may_be_missing and cost < 0:
        return None
    assert cost > 0
    g = dict(zip(GEOM, geom.tolist()))
    cmat = np.zeros(g["n_cmat"], np.float32)
    koff = np.zeros(g["n_koff"], np.int32)
    packlib.gnnb_pt_gather(w.ctypes.data, c_in, h_in, w_in, c_out, kh, kw, stride, pad, direction, normalise, allow16,
                           geom.ctypes.data, cmat.ctypes.data, cmat.size, koff.ctypes.data, koff.size)
    return g, cmat.reshape(g["NCG"], g["K2"], 64), koff.reshape(-1, 2), cost


def emulate_gather(g, cmat, koff, mu_src):
    """nb (N_dst, p) for one sample from the tables, the way k_gather_update walks them."""
    p = mu_src.shape[1]
    nb = np.zeros((g["N"], p))
    seen = np.zeros(g["N"], np.int32)
    for t in range(g["TPS"]):
        cg, rem = divmod(t, g["NBY"] * g["NBX"])
        by, bx = divmod(rem, g["NBX"])
        y0, x0 = by * g["PY"] + g["ay"], bx * g["PX"] + g["ax"]
        wy0, wx0 = by * g["ystep"] + g["ybase"], bx * g["xstep"] + g["xbase"]
        origin = wy0 * g["Ws"] + wx0
        lanes = g["lanes"]
        spk = 64 // lanes                      # window slots per k-step: 2 (32x32x2 MFMA) or 4 (16x16x4)
        acc = np.zeros((lanes, p))
        assert len(koff) == spk * g["K2"] + 8 * spk and all(p & 0xffff == 0x7fff for _, p in koff[spk * g["K2"]:])
        for k in range(spk * g["K2"]):
            off, packed = koff[k]
            wy, wx = wy0 + (packed & 0xffff), wx0 + (packed >> 16)
            if not (0 <= wy < g["Hs"] and 0 <= wx < g["Ws"]):
                continue
            row = mu_src[origin + off]
            acc += np.outer(cmat[cg, k // spk, (k % spk) * lanes:(k % spk) * lanes + lanes], row)
        for j in range(g["CT"] * g["PY"] * g["PX"]):
            cl, rem = divmod(j, g["PY"] * g["PX"])
            py, px = divmod(rem, g["PX"])
            y, x = y0 + py, x0 + px
            if 0 <= y < g["H"] and 0 <= x < g["W"]:
                n = ((cg * g["CT"] + cl) * g["H"] + y) * g["W"] + x
                nb[n] = acc[j]
                seen[n] += 1
    assert (seen == 1).all()          # every dst node belongs to exactly one (tile, lane)
    return nb


CONVS = [  # (c_in, c_out, k, stride, pad, h_in)  -- every conv of cifar_{base,wide,deep}_kw
    (3, 8, 4, 2, 1, 32), (8, 16, 4, 2, 1, 16), (3, 16, 4, 2, 1, 32), (16, 32, 4, 2, 1, 16),
    (8, 8, 3, 1, 1, 16), (8, 8, 4, 2, 1, 16),
]


def check_gather_tables(packlib, cfg, direction, allow16, may_be_missing=False):
    """The tables of one conv (c_in, c_out, k, stride, pad, h_in, w_in) in one direction, walked as the kernels walk them, against
    F.conv2d / F.conv_transpose2d.  Returns False where build_gather has no tables for it."""
    import torch
    import torch.nn.functional as F
    c_in, c_out, k, s, pad, h_in, w_in = cfg
    rng = np.random.RandomState(c_in * 100 + c_out + direction)
    w = rng.standard_normal((c_out, c_in, k, k)).astype(np.float32)
    built = build_gather(packlib, w, h_in, w_in, s, pad, direction, normalise=direction, allow16=allow16, may_be_missing=may_be_missing)
    if built is None:
        return False
    g, cmat, koff, cost = built
    assert g["lanes"] in ((16, 32) if allow16 else (32,))
    if allow16:                                      # never worse than the 32-node tiling, usually a third cheaper
        wide = build_gather(packlib, w, h_in, w_in, s, pad, direction, normalise=direction, may_be_missing=may_be_missing)
        assert wide is None and g["lanes"] == 16 or cost <= wide[3]      # (a 7x7 window on 8x8 only has 16-node tiles)
    h_out, w_out = (h_in + 2 * pad - k) // s + 1, (w_in + 2 * pad - k) // s + 1
    p = 4
    if direction == 0:
        mu = rng.standard_normal((c_in * h_in * w_in, p))
        x = torch.from_numpy(mu.T.reshape(p, c_in, h_in, w_in))
        want = F.conv2d(x, torch.from_numpy(w).double(), None, s, pad).reshape(p, -1).T.numpy()
    else:
        mu = rng.standard_normal((c_out * h_out * w_out, p))
        x = torch.from_numpy(mu.T.reshape(p, c_out, h_out, w_out))
        y = F.conv_transpose2d(x, torch.from_numpy(w).double(), None, s, pad)
        assert tuple(y.shape[-2:]) == (h_in, w_in)
        want = y.reshape(p, -1).T.numpy()            # the tap-count division is applied by the kernel, not the tables
    got = emulate_gather(g, cmat, koff, mu)
    np.testing.assert_allclose(got, want, atol=1e-5)
    dense = cost * 2 * 32 * 32 * 2 / 2          # MACs issued per sample (each MFMA: 32x32x2)
    useful = w.size * (h_out * w_out)           # MACs of the sparse map per channel
    print(f"conv {cfg} dir {direction} lanes {g['lanes']}: tile {g['CT']}x{g['PY']}x{g['PX']} align ({g['ay']},{g['ax']}) tiles {g['NBY']}x{g['NBX']} "
          f"window {g['WY']}x{g['WX']} K2={g['K2']} tiles/sample={g['TPS']} mfma/sample={cost} density={useful / (dense / 64 * 32):.2f}")
    return True


@pytest.mark.parametrize("cfg", CONVS)
@pytest.mark.parametrize("direction,allow16", [(0, 0), (1, 0), (0, 1)])
def test_gather_tables_match_torch_conv(packlib, cfg, direction, allow16):
    c_in, c_out, k, s, pad, h_in = cfg
    assert check_gather_tables(packlib, (c_in, c_out, k, s, pad, h_in, h_in), direction, allow16)


def fwd_arch_convs():
    """{arch: [(graph layer k, (c_in, c_out, k, stride, pad, h_in, w_in))]} of tests/common.py FWD_ARCHS."""
    from tests.common import FWD_ARCHS
    out = {}
    for name, ((_, h, w), spec) in FWD_ARCHS.items():
        out[name], layer = [], 0
        for sp in spec:
            if sp[0] == "conv":
                _, ci, co, k, st, pad = sp
                layer += 1
                out[name].append((layer, (ci, co, k, st, pad, h, w)))
                h, w = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
            elif sp[0] == "linear":
                layer += 1
    return out


# (c_in, c_out, k, stride, pad, h_in, w_in) with h_in != w_in, kernels 1..7, strides 1..4, pad 0..3, channels 3, 6, 8, 12, 16; kernels
# larger than the image; and every conv of FWD_ARCHS.  An exchanged H and W in the tables is invisible on the square CONVS above.
RECT_CONVS = sorted({(3, 8, 5, 1, 2, 12, 20), (8, 16, 2, 2, 0, 12, 20), (3, 8, 2, 3, 0, 20, 14), (8, 16, 1, 1, 0, 7, 5), (3, 8, 4, 2, 1, 10, 34),
                     (8, 8, 3, 1, 0, 9, 11), (3, 12, 3, 1, 1, 6, 6), (12, 6, 4, 2, 1, 6, 10), (3, 12, 3, 1, 1, 6, 10), (12, 6, 4, 2, 1, 6, 6),
                     (6, 16, 3, 1, 1, 6, 10), (8, 8, 3, 3, 0, 9, 15), (8, 16, 3, 2, 1, 7, 9), (8, 8, 7, 1, 3, 8, 8), (3, 8, 4, 4, 0, 8, 12),
                     (3, 8, 4, 2, 1, 4, 4), (8, 8, 4, 2, 1, 2, 2)} | {cfg for convs in fwd_arch_convs().values() for _, cfg in convs})


@pytest.mark.parametrize("cfg", RECT_CONVS, ids=lambda c: "{}to{}_k{}s{}p{}_{}x{}".format(*c))
@pytest.mark.parametrize("direction,allow16", [(0, 0), (1, 0), (0, 1)])
def test_gather_tables_match_torch_conv_on_rectangles(packlib, cfg, direction, allow16):
    """Where build_gather has tables for a geometry they are the conv / transposed conv (a geometry without tables takes the VALU
    kernels: test_gather_table_map_of_the_forward_geometry_archs pins which)."""
    if not check_gather_tables(packlib, cfg, direction, allow16, may_be_missing=True):
        print(f"conv {cfg} dir {direction}: no tables")


def test_gather_table_map_of_the_forward_geometry_archs(packlib):
    """Which directions of every conv edge of FWD_ARCHS have MFMA gather tables (as gnnb_bind_network asks for them: 16-lane tiles
    allowed).  Three of the networks are there BECAUSE an edge has none and takes the VALU conv kernels: a change to build_gather
    that gives them tables moves them onto other kernels, and must not do so unseen."""
    have = {}
    for name, convs in fwd_arch_convs().items():
        for layer, cfg in convs:
            c_in, c_out, k, s, pad, h_in, w_in = cfg
            w = np.ones((c_out, c_in, k, k), np.float32)
            have[(name, layer)] = tuple(build_gather(packlib, w, h_in, w_in, s, pad, d, normalise=int(d == 1 and layer > 1), allow16=1,
                                                     may_be_missing=True) is not None for d in (0, 1))
            print(f"{name} edge {layer} {c_in}->{c_out} {k}x{k}/{s}/{pad} on {h_in}x{w_in}: forward tables {have[(name, layer)][0]}, "
                  f"transposed tables {have[(name, layer)][1]}")
    assert have[("fwg_k7", 2)] == (True, False)          # 8 -> 8 7x7/1/3 on 8x8: forward tables only
    assert have[("fwg_valu", 2)] == (False, False)       # 16 -> 32 5x5/1/2 on 6x6: none in either direction
    assert have[("fwg_gap", 1)][1] is False              # 3 -> 8 2x2 stride 3: no transposed tables (k_convT_bwd + k_input_update)
    # the neighbours of the table-less edges do have them
    assert have[("fwg_k7", 1)] == (True, True) and have[("fwg_valu", 1)] == (True, True)


# ---- the host half of gnnb_bind_network (gnnb_pack.h parse_layers .. zero_tap_layer) ----
def layer_list(spec, null_weight_at=None):
    """(ctypes array, keep-alive) of a layer list written as in tests/common.py: ("conv", c_in, c_out, k, stride, pad),
    ("linear", n_in, n_out), ("relu",), ("flatten",), or ("kind", i) for a raw kind number."""
    from gnn_branching_amd._lib import GNNB_CONV, GNNB_FLATTEN, GNNB_LINEAR, GNNB_RELU, LayerDesc
    descs, keep = (LayerDesc * len(spec))(), []
    rng = np.random.RandomState(5)
    for q, (d, sp) in enumerate(zip(descs, spec)):
        if sp[0] == "conv":
            _, ci, co, k, st, pad = sp
            w, b = rng.standard_normal((co, ci, k, k)).astype(np.float32), rng.standard_normal(co).astype(np.float32)
            d.kind, d.c_in, d.c_out, d.kh, d.kw, d.stride, d.pad = GNNB_CONV, ci, co, k, k, st, pad
        elif sp[0] == "linear":
            _, ni, no = sp
            w, b = rng.standard_normal((no, ni)).astype(np.float32), rng.standard_normal(no).astype(np.float32)
            d.kind, d.n_in, d.n_out = GNNB_LINEAR, ni, no
        else:
            d.kind = {"relu": GNNB_RELU, "flatten": GNNB_FLATTEN}.get(sp[0], sp[-1])
            continue
        keep += [w, b]
        if q != null_weight_at:
            d.weight, d.bias = w.ctypes.data, b.ctypes.data
    return descs, keep


def parse(packlib, spec, shape, **kw):
    """parse_layers: (N, relu_q, hw, R, n_fixed), or the refusal as a string."""
    descs, keep = layer_list(spec, **kw)
    N, rq, hw, rn = (np.zeros(16, np.int32) for _ in range(4))
    err = C.create_string_buffer(512)
    packlib.gnnb_pt_parse.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    K = packlib.gnnb_pt_parse(descs, len(spec), *shape, N.ctypes.data, rq.ctypes.data, hw.ctypes.data, 16, rn.ctypes.data, err, 512)
    if K < 0:
        return err.value.decode()
    return N[:K].tolist(), rq[:K - 1].tolist(), hw[:K - 1].tolist(), int(rn[0]), int(rn[1])


RELU, FLAT = ("relu",), ("flatten",)
REFUSALS = [
    ([FLAT, ("conv", 3, 8, 3, 1, 1), RELU], (3, 4, 4), {}, "layer 1: conv after flatten"),
    ([("conv", 3, 8, 3, 1, 1), ("conv", 8, 8, 3, 1, 1), RELU], (3, 4, 4), {}, "layer 1: two linear maps without a ReLU between them"),
    ([FLAT, ("linear", 48, 6), ("linear", 6, 4), RELU], (3, 4, 4), {}, "layer 2: two linear maps without a ReLU between them"),
    ([("conv", 4, 8, 3, 1, 1), RELU], (3, 4, 4), {}, "layer 0: conv expects 4 input channels, graph has 3"),
    ([FLAT, ("linear", 10, 6), RELU], (3, 4, 4), {}, "layer 1: linear expects 10 inputs, graph has 48"),
    ([("conv", 3, 8, 3, 1, 1), RELU], (3, 4, 4), {"null_weight_at": 0}, "layer 0: null weight/bias"),
    ([FLAT, ("linear", 48, 6), RELU], (3, 4, 4), {"null_weight_at": 1}, "layer 1: null weight/bias"),
    ([("conv", 3, 8, 3, 0, 1), RELU], (3, 4, 4), {}, "layer 0: bad conv geometry"),
    ([("conv", 3, 8, 3, 2, 0), RELU], (3, 4, 4), {},
     "layer 0: conv geometry leaves a remainder (conv_transpose2d of the reference would need output_padding)"),
    ([FLAT, ("linear", 48, 6), RELU, ("linear", 6, 4)], (3, 4, 4), {}, "fixed layers must end after a ReLU (the property layer is passed per batch)"),
    ([FLAT, ("linear", 48, 4), RELU] + [("linear", 4, 4), RELU] * 8, (3, 4, 4), {}, "unsupported number of ReLU layers 9 (max 8)"),
    ([FLAT, FLAT], (3, 4, 4), {}, "unsupported number of ReLU layers 0 (max 8)"),
    ([FLAT, ("linear", 40368, 2), RELU], (3, 116, 116), {}, "graph layer 0 has 40368 nodes, more than the 40000 k_livesum holds in LDS"),
    ([RELU, FLAT], (3, 4, 4), {}, "layer 0: ReLU without a preceding conv/linear"),
    ([("kind", 7), RELU], (3, 4, 4), {}, "layer 0: unknown kind 7"),
]


@pytest.mark.parametrize("spec,shape,kw,message", REFUSALS, ids=[r[3][:40].replace(" ", "_") for r in REFUSALS])
def test_layer_list_refusals(packlib, spec, shape, kw, message):
    """One minimal layer list per refusal of parse_layers, with the wording gnnb_bind_network reports."""
    assert parse(packlib, spec, shape, **kw) == message


def test_layer_list_accepted(packlib):
    """Two convs and two linear maps on 3x8x8: one graph layer per ReLU, the input in front and the property node behind."""
    spec = [("conv", 3, 8, 4, 2, 1), RELU, ("conv", 8, 16, 4, 2, 1), RELU, FLAT, ("linear", 64, 20), RELU, ("linear", 20, 10), RELU]
    N, relu_q, hw, R, n_fixed = parse(packlib, spec, (3, 8, 8))
    assert N == [192, 8 * 4 * 4, 16 * 2 * 2, 20, 10, 1]
    assert R == 128 + 64 + 20 + 10 and n_fixed == len(spec)
    assert relu_q == [-1, 1, 3, 6, 8]              # the ReLU of graph layer k in the fixed-layer list
    assert hw == [1, 16, 4, 1, 1]                  # nodes per bias entry: H x W of a conv's output, 1 behind a Linear


def row_sums(packlib, w, geom=None):
    w = np.ascontiguousarray(w, np.float32)
    if geom is None:
        n_out, n_in = w.shape
        args, n = (1, 0, 0, 0, 0, 0, 0, 0, 0, n_in, n_out), n_out
    else:
        (c_out, c_in, kh, kw), (h_in, w_in, stride, pad) = w.shape, geom
        n = c_out * ((h_in + 2 * pad - kh) // stride + 1) * ((w_in + 2 * pad - kw) // stride + 1)
        args = (0, c_in, h_in, w_in, c_out, kh, kw, stride, pad, 0, 0)
    out = np.zeros(n, np.float32)
    packlib.gnnb_pt_row_sums.argtypes = [C.c_void_p] + [C.c_int] * 11 + [C.c_void_p]
    assert packlib.gnnb_pt_row_sums(w.ctypes.data, *args, out.ctypes.data) == n
    return out


@pytest.mark.parametrize("k,stride,pad,h_in,w_in", [(4, 2, 1, 8, 8), (3, 1, 0, 5, 7)])
def test_row_sums_of_a_conv_edge_1(packlib, k, stride, pad, h_in, w_in):
    """s[node] = the sum of the weights of the taps that lie inside the image (the border nodes of a padded conv lose taps), added
    in fp32: within n 2^-24 sum|w| of the fp64 sum over the same n taps."""
    w = np.random.RandomState(k).standard_normal((8, 3, k, k)).astype(np.float32)
    h_out, w_out = (h_in + 2 * pad - k) // stride + 1, (w_in + 2 * pad - k) // stride + 1
    got = row_sums(packlib, w, (h_in, w_in, stride, pad)).reshape(8, h_out, w_out)
    lost = 0
    for oy in range(h_out):
        for ox in range(w_out):
            ys = [ky for ky in range(k) if 0 <= oy * stride - pad + ky < h_in]
            xs = [kx for kx in range(k) if 0 <= ox * stride - pad + kx < w_in]
            taps = w[:, :, ys][:, :, :, xs].astype(np.float64).reshape(8, -1)
            lost += taps.shape[1] < 3 * k * k
            bound = taps.shape[1] * 2.0 ** -24 * np.abs(taps).sum(1)
            assert (np.abs(got[:, oy, ox] - taps.sum(1)) <= bound).all(), (oy, ox)
    assert (lost > 0) == (pad > 0)


def test_row_sums_of_a_linear_edge_1(packlib):
    w = np.random.RandomState(1).standard_normal((6, 10)).astype(np.float32)
    got = row_sums(packlib, w)
    assert (np.abs(got - w.astype(np.float64).sum(1)) <= 10 * 2.0 ** -24 * np.abs(w.astype(np.float64)).sum(1)).all()


@pytest.mark.parametrize("n_in,n_out", [(10, 6), (64, 32), (65, 33), (130, 100)])
def test_dense_operands_of_a_linear_edge(packlib, n_in, n_out):
    """Both padded images of a Linear edge and their mt / ld / ksq / kpad.  The expected geometry is written out here from the
    formulas the dense kernels were built against (DENSE_CH = 8 k-steps per chunk), not read from the code under test."""
    w = np.random.RandomState(n_in).standard_normal((n_out, n_in)).astype(np.float32)
    geom = np.zeros(10, np.int32)
    packlib.gnnb_pt_dense.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    packlib.gnnb_pt_dense.restype = None
    packlib.gnnb_pt_dense(w.ctypes.data, n_in, n_out, geom.ctypes.data, None, 0, None, 0)
    ld_fwd, mt_fwd, ksq_fwd, ld_bwd, mt_bwd, ksq_bwd, kpad_fwd, kpad_bwd, n_fwd, n_bwd = geom.tolist()

    def ksq_of(K):          # k-steps per wave: ceil(ceil(K / 2) / 4) rounded up to whole chunks of 8
        return ((((K + 1) // 2 + 3) // 4 + 7) // 8) * 8
    assert (mt_fwd, ld_fwd, ksq_fwd, kpad_fwd) == ((n_out + 31) // 32, (n_out + 31) // 32 * 32, ksq_of(n_in), (n_in + 63) // 64 * 64)
    assert (mt_bwd, ld_bwd, ksq_bwd, kpad_bwd) == ((n_in + 31) // 32, (n_in + 31) // 32 * 32, ksq_of(n_out), (n_out + 15) // 16 * 16)
    rows_f, rows_b = max(8 * ksq_fwd + 16, kpad_fwd + 32), max(8 * ksq_bwd + 16, kpad_bwd + 64)
    assert (n_fwd, n_bwd) == (rows_f * ld_fwd, rows_b * ld_bwd)
    fwd, bwd = np.full(n_fwd, np.nan, np.float32), np.full(n_bwd, np.nan, np.float32)
    packlib.gnnb_pt_dense(w.ctypes.data, n_in, n_out, geom.ctypes.data, fwd.ctypes.data, n_fwd, bwd.ctypes.data, n_bwd)
    fwd, bwd = fwd.reshape(rows_f, ld_fwd), bwd.reshape(rows_b, ld_bwd)
    np.testing.assert_array_equal(fwd[:n_in, :n_out], w.T)           # forward image [i][o] == W[o][i]
    np.testing.assert_array_equal(bwd[:n_out, :n_in], w)             # transposed image [o][i] == W[o][i]
    fwd[:n_in, :n_out] = 0
    bwd[:n_out, :n_in] = 0
    assert not fwd.view(np.uint32).any() and not bwd.view(np.uint32).any()      # every padded entry is exactly +0


def test_tile_table_of_the_forward_geometry_archs(packlib):
    """The packed tile table of every gather geometry test_gather_table_map_of_the_forward_geometry_archs builds: entry t is
    (channel group, block row, block column) = (t / (NBY NBX), (t % (NBY NBX)) / NBX, t % NBX) in 8 + 12 + 12 bits."""
    packlib.gnnb_pt_tile_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    seen = 0
    for name, convs in fwd_arch_convs().items():
        for layer, (c_in, c_out, k, s, pad, h_in, w_in) in convs:
            w = np.ones((c_out, c_in, k, k), np.float32)
            for d in (0, 1):
                built = build_gather(packlib, w, h_in, w_in, s, pad, d, normalise=int(d == 1 and layer > 1), allow16=1, may_be_missing=True)
                if built is None:
                    continue
                g = built[0]
                tt = np.full(g["TPS"], -1, np.int32)
                assert packlib.gnnb_pt_tile_table(g["NCG"], g["NBY"], g["NBX"], tt.ctypes.data) == 1
                t = np.arange(g["TPS"])
                per = g["NBY"] * g["NBX"]
                np.testing.assert_array_equal(tt & 0xff, t // per)
                np.testing.assert_array_equal((tt >> 8) & 0xfff, (t % per) // g["NBX"])
                np.testing.assert_array_equal((tt >> 20) & 0xfff, t % g["NBX"])
                seen += 1
    assert seen >= 8
    tt = np.zeros(1, np.int32)
    for over in ((256, 1, 1), (1, 4096, 1), (1, 1, 4096)):          # a field that does not fit its bits: refused, nothing written
        assert packlib.gnnb_pt_tile_table(*over, tt.ctypes.data) == 0


def zero_tap(packlib, spec, shape):
    descs, keep = layer_list(spec)
    yx = np.full(2, -1, np.int32)
    packlib.gnnb_pt_zero_tap.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    return packlib.gnnb_pt_zero_tap(descs, len(spec), *shape, yx.ctypes.data), tuple(yx.tolist())


def test_zero_tap_layer(packlib):
    """An inner conv with stride > kernel leaves pixels of the layer below that no window reads (2x2 windows every 3 pixels: row /
    column 2 is the first).  Edge 1 is not normalised and may; a covering conv has none."""
    gap = ("conv", 8, 8, 2, 3, 0)                       # on 8x8: windows at 0-1, 3-4, 6-7
    k, (y, x) = zero_tap(packlib, [("conv", 3, 8, 3, 1, 1), RELU, gap, RELU], (3, 8, 8))
    assert k == 2 and (y, x) == (2, 2)
    assert zero_tap(packlib, [("conv", 8, 8, 2, 3, 0), RELU, ("conv", 8, 8, 3, 1, 1), RELU], (8, 8, 8))[0] == 0      # the same conv as edge 1
    assert zero_tap(packlib, [("conv", 3, 8, 3, 1, 1), RELU, ("conv", 8, 8, 4, 2, 1), RELU], (3, 8, 8))[0] == 0      # a covering conv


# ---- the one check of a gnnb_batch against a layer graph (gnnb_pack.h check_batch) ----
# conv 3 -> 8 4x4 stride 2 pad 1 on 3x8x8, ReLU, flatten, Linear 128 -> 33, ReLU (tools/bind_host_sanitize.cpp): N = [192, 128, 33, 1],
# 4 bound, 2 dual and 6 primal tensors; the ReLUs are network layers 1 and 4, so primals 0, 1, 3, 4 and the last (5) are read, 2 is not.
BATCH_SPEC, BATCH_SHAPE = [("conv", 3, 8, 4, 2, 1), RELU, FLAT, ("linear", 128, 33), RELU], (3, 8, 8)
ENTRY_POINTS = ("gnnb_forward", "gnnb_forward_host", "gnnb_pack_amb_records", "gnnb_online_step")
ALL, NONE = (True,) * 4, (False,) * 4
# (case, change to the valid batch, accepted by (forward, forward_host, pack_amb_records, online_step)) -- every verdict written by hand
BATCH_CASES = [
    ("valid", {}, ALL),
    ("B=0", {"B": 0}, NONE),
    ("n_graph-1", {"n_graph": 3}, NONE), ("n_graph+1", {"n_graph": 5}, NONE),
    ("n_relu-1", {"n_relu": 1}, NONE), ("n_relu+1", {"n_relu": 3}, NONE),
    # n_primal: exactly n_fixed + 1 = 6 everywhere but in gnnb_online_step, whose own rule is n_primal >= n_fixed = 5 (it reads the two
    # primals of every ReLU layer, at most entry n_fixed - 1, and the LAST entry given): 5 is its boundary, 4 is below it
    ("n_primal-1", {"n_primal": 5}, (False, False, False, True)), ("n_primal+1", {"n_primal": 7}, (False, False, False, True)),
    ("n_primal-2", {"n_primal": 4}, NONE),
    ("lb table NULL", {"lb": None}, NONE), ("ub table NULL", {"ub": None}, NONE),
    ("dual table NULL", {"dual": None}, NONE), ("primal table NULL", {"primal": None}, NONE),
    # entries: the packer reads only the ReLU layers' rows and primals[-1]; the host form and the online step skip the unread primal
    ("lb[0] NULL", {"lb": 0}, (False, False, True, False)), ("lb[1] NULL", {"lb": 1}, NONE), ("lb[2] NULL", {"lb": 2}, NONE),
    ("lb[3] NULL", {"lb": 3}, (False, False, True, False)),
    ("ub[0] NULL", {"ub": 0}, (False, False, True, False)), ("ub[1] NULL", {"ub": 1}, NONE), ("ub[2] NULL", {"ub": 2}, NONE),
    ("ub[3] NULL", {"ub": 3}, (False, False, True, False)),
    ("dual[0] NULL", {"dual": 0}, NONE), ("dual[1] NULL", {"dual": 1}, NONE),
    ("primal[0] NULL", {"primal": 0}, NONE), ("primal[1] NULL", {"primal": 1}, NONE),
    ("primal[2] NULL", {"primal": 2}, (False, True, True, True)),
    ("primal[3] NULL", {"primal": 3}, NONE), ("primal[4] NULL", {"primal": 4}, NONE), ("primal[5] NULL", {"primal": 5}, NONE),
    ("x_lp NULL", {"x_lp": None}, (False, False, True, False)), ("prop_w NULL", {"prop_w": None}, (False, False, True, False)),
    ("prop_b NULL", {"prop_b": None}, (False, False, True, False)), ("mask NULL", {"mask": None}, (False, False, True, False)),
]


@pytest.mark.parametrize("case,change,accepted", BATCH_CASES, ids=[c[0].replace(" ", "_") for c in BATCH_CASES])
def test_check_batch(packlib, case, change, accepted):
    """A batch with the right counts and every pointer set passes under the needs of each entry point; a batch size below 1, a count that
    is off, a NULL table and a NULL entry the entry point reads are refused -- before anything is indexed: the tables hold exactly as many
    entries as the batch says -- and an entry the entry point does not read may be NULL."""
    from gnn_branching_amd._lib import Batch
    descs, keep = layer_list(BATCH_SPEC)
    some = np.zeros(1, np.float32).ctypes.data             # (check_batch looks at no tensor's memory)
    counts = {"n_graph": 4, "n_relu": 2, "n_primal": 6}
    counts.update({k: v for k, v in change.items() if k in counts})
    tabs = {"lb": [some] * counts["n_graph"], "ub": [some] * counts["n_graph"], "dual": [some] * counts["n_relu"], "primal": [some] * counts["n_primal"]}
    loose = {"x_lp": some, "prop_w": some, "prop_b": some, "mask": some}
    for name, v in change.items():
        if name in tabs and v is None:
            tabs[name] = None
        elif name in tabs:
            tabs[name][v] = None
        elif name in loose:
            loose[name] = None
    ctabs = {k: None if t is None else (C.c_void_p * len(t))(*t) for k, t in tabs.items()}
    batch = Batch(ctabs["lb"], ctabs["ub"], ctabs["dual"], ctabs["primal"], loose["x_lp"], loose["prop_w"], loose["prop_b"], loose["mask"],
                  counts["n_graph"], counts["n_relu"], counts["n_primal"])
    err = C.create_string_buffer(512)
    packlib.gnnb_pt_check_batch.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    for which, (entry, want) in enumerate(zip(ENTRY_POINTS, accepted)):
        got = packlib.gnnb_pt_check_batch(descs, len(BATCH_SPEC), *BATCH_SHAPE, C.byref(batch), change.get("B", 2), which, err, 512)
        assert got == int(want), (case, entry, err.value.decode())
        assert (err.value == b"") == want and (want or err.value.startswith(b"the batch does not match the bound network: "))
