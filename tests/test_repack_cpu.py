"""The device pack builder's shared code on the CPU: the fold and emit functions of gnnb_pack.h that gnnb_k_repack.h runs one thread
per element, run as plain loops (csrc/gnnb_repack_test.cpp) and compared with build_packs (gnnb_pt_pack) for all 14 packs.

Copied and permuted values are bit-equal.  A folded entry is one fp64 sum of n <= 129 terms rounded to fp32 once in both builders;
with A = |y0| + sum |a_k| |b_k| and the exact value from a numpy.longdouble sum, each fp64 sum lies within (n + 1) 2^-53 A of the
exact value, so
  * where A <= 2^20 |exact| both builders are within 1 fp32 ulp of each other and of the exact value rounded to fp32;
  * where A is larger (cancellation) the new value is within 2^-40 A of the exact value -- plus 2^-150, half the smallest fp32
    subnormal, which is the rounding of the fp32 format itself where the result is subnormal (the shipped checkpoint's forward
    weights are all subnormal, so its folds are);
  * entries an inf or NaN reaches are compared by class.
B2 and B5 start from the builder's own rounded bcb: their exact value is taken from the new builder's bcb."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.common import state_of

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn_branching_amd", "csrc")
PACK_NAMES = ["embed", "pre_fwd", "pre_bwd", "pre_inp", "prop", "upd_fwd_e", "upd_fwd_i", "upd_fwd_f", "upd_bwd", "upd_bwd_b",
              "upd_inp", "post_inp", "score_b", "score_f"]
# the 26 Linear layers in blob order: (name, out, in)
LAYERS = [("inp_f", 64, 3), ("inp_f_1", 64, 64), ("inp_b", 64, 2), ("inp_b_1", 64, 64), ("inp_b2", 64, 128), ("inp_b2_2", 64, 64),
          ("fc1", 64, 7), ("fc1_1", 64, 64), ("fc3", 64, 128), ("fc3_2", 64, 64), ("fc4", 64, 128), ("fc4_2", 64, 64), ("out1", 64, 4),
          ("out2", 64, 128), ("out3", 64, 64), ("bc1", 64, 7), ("bc1_1", 64, 64), ("bc1_2", 64, 64), ("bc2", 64, 192), ("bc2_1", 64, 64),
          ("bc3", 64, 128), ("bc3_1", 64, 64), ("bc4", 64, 128), ("bc4_1", 64, 64), ("fnode", 64, 64), ("fscore", 1, 64)]
# float offsets inside the packs (the Pack* enums of gnnb_pack.h)
UPD = dict(WA=0, WAS=8192, BA=12288, WCB=12352, BCB=16448, BCBROW=16512, VAW=16576, WAS3=16704, WCB3=22848, WA1S3=28992, ALL=35136)
PRE_FWD = dict(W2=576, B2=4672, W23=4736)
PRE_BWD = dict(W5=21248, B5=25344, W53=37696)
PRE_INP = dict(W2=192, B2=4288, W23=4352)
POST_INP = dict(WPN=0, WPG=4096, WPN3=8192, WPG3=14336)
SCORE = dict(W1=0, V1=4228)
PROP = dict(W2T=320, V2=12736)
LD = np.longdouble


def blob_of(sd):
    return np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in sd.values()])


def layer_views(blob):
    """name -> (W (out, in), b (out)) views of a blob."""
    out, o = {}, 0
    for name, no, ni in LAYERS:
        out[name] = (blob[o:o + no * ni].reshape(no, ni), blob[o + no * ni:o + no * ni + no])
        o += no * ni + no
    assert o == blob.size == 117825
    return out


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def crafted_blob():
    """The random blob with +-0, subnormals, 2^-126, 0x3F7FFFFF (a bf16 rounding that carries into the exponent), +-inf and NaN in a
    few known places of Linear weights that are folded (fc3_2, inp_b2_2, bc2_1, fc4) and copied (bc1_1, bc2, fc3)."""
    blob = blob_of(state_of("random")).copy()
    lv = layer_views(blob)
    specials = [0.0, -0.0, f32(0x00000001), -f32(0x00012345), f32(0x007FFFFF), f32(0x00800000), f32(0x3F7FFFFF), -f32(0x3F7FFFFF),
                f32(0x477FFFFF)]
    for name in ["fc3_2", "inp_b2_2", "bc2_1", "fc4", "bc1_1", "bc2", "fc3"]:
        W = lv[name][0]
        for q, v in enumerate(specials):
            W[(5 * q + 3) % 64, (11 * q + 2) % W.shape[1]] = v
            W[(7 * q + 1) % 64, (13 * q + 70) % W.shape[1]] = v
    lv["fc3_2"][0][9, 17] = np.inf
    lv["bc2_1"][0][40, 3] = -np.inf
    lv["inp_b2_2"][0][22, 50] = np.nan
    lv["bc1_1"][0][12, 12] = np.inf
    lv["bc2"][0][33, 150] = np.nan
    lv["bc1_2"][0][2, 60] = -np.inf
    return blob


BLOBS = ["shipped", "random", "crafted"]


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("repack")
    out = []
    for src in ["gnnb_pack_test.cpp", "gnnb_repack_test.cpp"]:
        so = str(d / ("lib" + src[:-4] + ".so"))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(CSRC, src)])
        out.append(C.CDLL(so))
    old, new = out
    for fn in (old.gnnb_pt_pack, new.gnnb_pt_repack):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    new.gnnb_pt_repack_cover.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return old, new


def all_packs(fn, blob):
    out = {}
    for which, name in enumerate(PACK_NAMES):
        n = fn(blob.ctypes.data, which, None, 0)
        buf = np.zeros(n, np.float32)
        assert fn(blob.ctypes.data, which, buf.ctypes.data, n) == n
        out[name] = buf
    return out


@pytest.fixture(scope="module")
def built(libs):
    """blob name -> (blob, old packs, new packs): each builder runs once per blob."""
    old, new = libs
    out = {}
    for name in BLOBS:
        blob = crafted_blob() if name == "crafted" else blob_of(state_of(name))
        out[name] = (blob, all_packs(old.gnnb_pt_pack, blob), all_packs(new.gnnb_pt_repack, blob))
    return out


# ---- the layouts, written forwards from the comments of gnnb_pack.h ----
def feat(R, h):
    return 8 * (R >> 2) + 4 * h + (R & 3)


def gfeat(R, h):
    it, r = R >> 4, R & 15
    return 2 * ((r & 3) + 8 * (r >> 2) + 4 * h) + it


def w64_map(nfrag):
    """(row, col) of the 64 x (64 nfrag) matrix held by float d of a pack_w64 block."""
    s, it, lane = np.meshgrid(np.arange(32 * nfrag), np.arange(2), np.arange(64), indexing="ij")
    d = ((((s >> 2) * 2 + it) * 64 + lane) * 4 + (s & 3)).ravel()
    row = np.empty(d.size, np.int64)
    col = np.empty(d.size, np.int64)
    row[d] = (32 * it + (lane & 31)).ravel()
    col[d] = (64 * (s >> 5) + feat(s & 31, lane >> 5)).ravel()
    return row, col


def bf3_map():
    """(row, col, piece) of the 64 x 64 matrix held by bf16 entry u of a one-fragment pack_w64_bf3 block."""
    ks, ot, p, lane, j = np.meshgrid(np.arange(4), np.arange(2), np.arange(3), np.arange(64), np.arange(8), indexing="ij")
    u = (((ks * 2 + ot) * 3 + p) * 512 + lane * 8 + j).ravel()
    row, col, piece = (np.empty(u.size, np.int64) for _ in range(3))
    row[u] = (32 * ot + (lane & 31)).ravel()
    col[u] = feat(8 * ks + j, lane >> 5).ravel()
    piece[u] = p.ravel()
    return row, col, piece


def vec64_map():
    h, R = np.meshgrid(np.arange(2), np.arange(32), indexing="ij")
    m = np.empty(64, np.int64)
    m[(h * 32 + R).ravel()] = feat(R, h).ravel()
    return m


def pair_map():
    """(row, col) of a 64 x 2 matrix in pack_wsmall order, one k-step."""
    it, lane = np.meshgrid(np.arange(2), np.arange(64), indexing="ij")
    d = (it * 64 + lane).ravel()
    row, col = np.empty(128, np.int64), np.empty(128, np.int64)
    row[d] = (32 * it + (lane & 31)).ravel()
    col[d] = (lane >> 5).ravel()
    return row, col


def bf16_pieces(x):
    """bf3_split_512's rule on an fp32 array: (3, ...) uint16."""
    x = np.array(x, np.float32)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(3):
            u = x.view(np.uint32).astype(np.uint64)
            special = (u >> 16) | np.where(u & 0xffff, 0x40, 0).astype(np.uint64)
            rounded = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
            b = np.where((u & 0x7f800000) == 0x7f800000, special, rounded).astype(np.uint32)
            out.append(b.astype(np.uint16))
            x = (x - (b << 16).astype(np.uint32).view(np.float32)).astype(np.float32)
    return np.stack(out)


# ---- the folded quantities, exactly ----
class Fold:
    """exact (longdouble) value and the bound A of a folded block; n: terms of its sum."""
    def __init__(self, exact, A, n):
        self.exact, self.A, self.n = exact, A, n


def mm(A, B):
    with np.errstate(invalid="ignore", over="ignore"):
        return Fold(A.astype(LD) @ B.astype(LD), np.abs(A).astype(LD) @ np.abs(B).astype(LD), A.shape[1])


def mv(A, x, y0=None):
    y = np.zeros(A.shape[0], LD) if y0 is None else y0.astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        return Fold(A.astype(LD) @ x.astype(LD) + y, np.abs(A).astype(LD) @ np.abs(x).astype(LD) + np.abs(y), A.shape[1] + 1)


def add(f, g):
    with np.errstate(invalid="ignore"):
        return Fold(f.exact + g.exact, f.A + g.A, f.n + g.n)


def pairs(f, g=None):
    z = Fold(np.zeros(64, LD), np.zeros(64, LD), 1) if g is None else g
    return Fold(np.stack([f.exact, z.exact], 1), np.stack([f.A, z.A], 1), f.n)


def folded_regions(blob, new):
    """[(pack, offset, layout, Fold)]: every folded fp32 region of the image.  layout: w64 / w64x2 / vec64 / row / pair / trans."""
    lv = layer_views(blob)
    W = {k: v[0] for k, v in lv.items()}
    b = {k: v[1] for k, v in lv.items()}
    G = np.empty(64, np.int64)
    for h in range(2):
        for R in range(32):
            G[gfeat(R, h)] = feat(R, h)
    out = []
    cb = {}
    for d, (lb_, lc_) in {"fwd": ("fc3_2", "fc4"), "bwd": ("bc3_1", "bc4")}.items():
        cb[d] = (mm(W[lc_][:, 64:], W[lb_]), mv(W[lc_][:, 64:], b[lb_], b[lc_]))
    for pack, a, d, proj in [("upd_fwd_e", "fc3", "fwd", "inp_f_1"), ("upd_fwd_i", "fc3", "fwd", "inp_b2_2"), ("upd_fwd_f", "fc3", "fwd", "fc4_2"),
                             ("upd_bwd", "bc3", "bwd", None), ("upd_bwd_b", "bc3", "bwd", "bc4_1")]:
        if proj:
            t0, t1 = mm(W[a][:, :64], W[proj]), mm(W[a][:, 64:], W[proj])
            out.append((pack, UPD["WA"], "w64x2", Fold(np.concatenate([t0.exact, t1.exact], 1), np.concatenate([t0.A, t1.A], 1), 64)))
            out.append((pack, UPD["WAS"], "w64", add(t0, t1)))
            out.append((pack, UPD["VAW"], "pair", pairs(mv(W[a][:, :64], b[proj]), mv(W[a][:, 64:], b[proj]))))
        else:
            out.append((pack, UPD["WAS"], "w64", Fold(W[a][:, :64].astype(LD) + W[a][:, 64:].astype(LD),
                                                    np.abs(W[a][:, :64]).astype(LD) + np.abs(W[a][:, 64:]).astype(LD), 2)))
        out.append((pack, UPD["WCB"], "w64", cb[d][0]))
        out.append((pack, UPD["BCB"], "vec64", cb[d][1]))
        out.append((pack, UPD["BCBROW"], "row", cb[d][1]))
    bcb_f = new["upd_fwd_f"][UPD["BCBROW"]:UPD["BCBROW"] + 64]
    bcb_b = new["upd_bwd"][UPD["BCBROW"]:UPD["BCBROW"] + 64]
    out.append(("pre_fwd", PRE_FWD["W2"], "w64", mm(W["fc4"][:, :64], W["fc1_1"])))
    out.append(("pre_fwd", PRE_FWD["B2"], "vec64", mv(W["fc4"][:, :64], b["fc1_1"], bcb_f)))
    out.append(("pre_bwd", PRE_BWD["W5"], "w64", mm(W["bc4"][:, :64], W["bc2_1"])))
    out.append(("pre_bwd", PRE_BWD["B5"], "vec64", mv(W["bc4"][:, :64], b["bc2_1"], bcb_b)))
    out.append(("pre_inp", PRE_INP["W2"], "w64", mm(W["inp_b2"][:, :64], W["inp_b_1"])))
    out.append(("pre_inp", PRE_INP["B2"], "vec64", mv(W["inp_b2"][:, :64], b["inp_b_1"], b["inp_b2"])))
    wc = mm(W["inp_b2"][:, 64:], W["bc4_1"])
    out.append(("upd_inp", 0, "pair", pairs(mv(W["inp_b2"][:, 64:], b["bc4_1"]))))
    out.append(("post_inp", POST_INP["WPN"], "w64", wc))
    out.append(("post_inp", POST_INP["WPG"], "w64", Fold(wc.exact[G], wc.A[G], wc.n)))
    for pack, proj in [("score_b", "bc4_1"), ("score_f", "fc4_2")]:
        out.append((pack, SCORE["W1"], "w64", mm(W["fnode"], W[proj])))
        out.append((pack, SCORE["V1"], "pair", pairs(mv(W["fnode"], b[proj]))))
    out.append(("prop", PROP["W2T"] + 4096, "trans", mm(W["out2"][:, 64:], W["fc4_2"])))
    out.append(("prop", PROP["V2"], "row", mv(W["out2"][:, 64:], b["fc4_2"])))
    return out


# (pack, fp32 block, its column half or None, bf16 x 3 block): the three-piece forms of folded blocks
BF3_OF_FOLDS = ([(p, UPD["WAS"], None, UPD["WAS3"]) for p in PACK_NAMES[5:10]] + [(p, UPD["WCB"], None, UPD["WCB3"]) for p in PACK_NAMES[5:10]] +
                [(p, UPD["WA"], 1, UPD["WA1S3"]) for p in ["upd_fwd_e", "upd_fwd_i", "upd_fwd_f", "upd_bwd_b"]] +
                [("pre_fwd", PRE_FWD["W2"], None, PRE_FWD["W23"]), ("pre_bwd", PRE_BWD["W5"], None, PRE_BWD["W53"]),
                 ("pre_inp", PRE_INP["W2"], None, PRE_INP["W23"]), ("post_inp", POST_INP["WPN"], None, POST_INP["WPN3"]),
                 ("post_inp", POST_INP["WPG"], None, POST_INP["WPG3"])])


def region_in_layout(layout, M):
    """The (64, .) or (64,) array M as the floats of its region."""
    if layout in ("w64", "w64x2"):
        row, col = w64_map(2 if layout == "w64x2" else 1)
        return M[row, col]
    if layout == "vec64":
        return M[vec64_map()]
    if layout == "pair":
        row, col = pair_map()
        return M[row, col]
    if layout == "trans":
        return M.T.reshape(-1)
    return M.reshape(-1)


def folded_masks(blob, new):
    """pack -> bool mask of its folded floats (fp32 regions and the bf16 forms of folded blocks)."""
    mask = {p: np.zeros(new[p].size, bool) for p in PACK_NAMES}
    for pack, off, layout, f in folded_regions(blob, new):
        mask[pack][off:off + f.exact.size] = True
    for pack, _, _, off3 in BF3_OF_FOLDS:
        mask[pack][off3:off3 + 6144] = True
    return mask


def ordered(x):
    """fp32 -> integers in value order (adjacent floats differ by 1; -0 and +0 coincide)."""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def cancellation(f):
    with np.errstate(invalid="ignore"):
        return f.A > LD(2.0) ** 20 * np.abs(f.exact)


def reached(f):
    return ~np.isfinite(f.A.astype(np.float64)) | ~np.isfinite(f.exact.astype(np.float64)) | np.isnan(f.A)


def test_segments_cover_every_pack_once(libs):
    _, new = libs
    for which in range(14):
        written, twice = C.c_size_t(), C.c_size_t()
        new.gnnb_pt_repack_cover(which, C.byref(written), C.byref(twice))
        n = new.gnnb_pt_repack(None, which, None, 0)
        assert (written.value, twice.value) == (n, 0), PACK_NAMES[which]


@pytest.mark.parametrize("name", BLOBS)
def test_copied_and_permuted_values_are_bit_equal(built, name):
    blob, old, new = built[name]
    mask = folded_masks(blob, new)
    for p in PACK_NAMES:
        assert old[p].size == new[p].size
        keep = ~mask[p]
        assert np.array_equal(old[p].view(np.uint32)[keep], new[p].view(np.uint32)[keep]), p
    assert sum(int((~m).sum()) for m in mask.values()) == 76680      # of the image's 301 704 floats


def check_folds(blob, packs, new, against=None):
    """The fold rule on `packs` (`new`: where B2 / B5 take their bcb from).  Returns (entries, cancellation entries)."""
    total = cancel = 0
    for pack, off, layout, f in folded_regions(blob, new):
        exact, A = region_in_layout(layout, f.exact), region_in_layout(layout, f.A)
        g = Fold(exact, A, f.n)
        got = packs[pack][off:off + exact.size]
        bad = reached(g)
        want32 = np.zeros(exact.size, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            want32[~bad] = exact[~bad].astype(np.float32)
        can = cancellation(g) & ~bad
        plain = ~can & ~bad
        total += int((~bad).sum())
        cancel += int(can.sum())
        where = "%s+%d" % (pack, off)
        assert np.all(np.abs(ordered(got[plain]) - ordered(want32[plain])) <= 1), where
        err = np.abs(got[can].astype(LD) - exact[can])
        assert np.all(err <= LD(2.0) ** -40 * A[can] + LD(2.0) ** -150), where
        if against is not None:
            ref = against[pack][off:off + exact.size]
            assert np.all(np.abs(ordered(got[plain]) - ordered(ref[plain])) <= 1), where
            assert np.array_equal(np.isnan(got[bad]), np.isnan(ref[bad])), where
            both = bad.copy()
            both[bad] = ~np.isnan(ref[bad])
            assert np.array_equal(got[both], ref[both]), where      # +-inf, or a value the inf did not reach after all
    return total, cancel


@pytest.mark.parametrize("name", BLOBS)
def test_old_builder_meets_the_fold_rule_and_cancellation_is_rare(built, name):
    blob, old, new = built[name]
    total, cancel = check_folds(blob, old, old)
    assert total > 100000
    assert cancel <= 0.001 * total, (cancel, total)


@pytest.mark.parametrize("name", BLOBS)
def test_folded_entries(built, name):
    blob, old, new = built[name]
    total, cancel = check_folds(blob, new, new, against=old)
    assert total > 100000 and cancel <= 0.001 * total


@pytest.mark.parametrize("name", BLOBS)
def test_bf16_pieces_of_folded_blocks(built, name):
    blob, old, new = built[name]
    row, col, piece = bf3_map()
    for pack, off, half, off3 in BF3_OF_FOLDS:
        r, c = w64_map(1 if half is None else 2)
        M = np.zeros((64, r.size // 64), np.float32)
        M[r, c] = new[pack][off:off + r.size]
        if half is not None:
            M = M[:, 64 * half:64 * half + 64]
        want = bf16_pieces(M)[piece, row, col]
        got = new[pack][off3:off3 + 6144].view(np.uint16)
        assert np.array_equal(got, want), (pack, off3)


def test_crafted_blob_holds_its_special_values(built):
    blob, old, new = built["crafted"]
    bits = set(blob.view(np.uint32).tolist())
    for v in [0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F7FFFFF, 0x7F800000, 0xFF800000]:
        assert v in bits
    assert np.isnan(blob).sum() == 2
    # the carry into the exponent: 0x3F7FFFFF rounds to bf16 1.0, and the second piece is negative
    p = bf16_pieces(np.array([f32(0x3F7FFFFF)], np.float32))[:, 0]
    assert p[0] == 0x3F80 and p[1] & 0x8000
