"""The PAIR walk of the block-form tiles (gnnb_k_gather.h gather_pair16_block / _embed, gnnb_k_fusedq.h fusedq_gather_pairs), emulated in numpy
lane for lane on top of the instruction model of tests/test_blocktap_cpu.py:

  * the tiles (y, xp) and (y + 1, xp) walk their 3 x 6 window rows together, each row fetched once: the upper tile takes window row wy as
    ky = wy (wy < 4), the lower tile as ky = wy - 2 (wy >= 2), out of the same rows of the tap image;
  * the placement: the 32 nodes of the pair take ring rows in ballot order, and the column lanes write their accumulators into the ring row of the
    node the column stands for (blk_dst, per tile half).

Every live node's row must equal block_form_aggregate's bit for bit -- the one-tile walk, which the library keeps in k_gather16 -- and must have
been written exactly once, whole.  Geometries: a 5 x 6 output (the last row is a pair without a lower tile) and an 8 x 4 output; the live masks
put 0, 1, 4, 5 and 8 live channels at positions of upper tiles, lower tiles and the unpaired row.  (Every group of a position is issued: packing
the live channels into groups was measured slower and is not in the library)"""
import numpy as np
import pytest

from tests.test_blocktap_cpu import block_form_aggregate, btlib, host_image, make, mfma_4x4x1_16b      # noqa: F401  (btlib: fixture)

KH, WY, STRIDE, PAD = 4, 6, 2, 1
LANE = np.arange(64)


def live_mask(h_out, w_out, seed, forced):
    """(8, h_out, w_out) bool: random, then the positions of `forced` {(y, x): number of live channels} overwritten (the lowest / a spread set)."""
    rng = np.random.default_rng(seed)
    live = rng.random((8, h_out, w_out)) < 0.55
    spread = {0: [], 1: [6], 4: [0, 3, 5, 6], 5: [1, 2, 4, 5, 7], 8: list(range(8))}
    for (y, x), n in forced.items():
        live[:, y, x] = False
        live[spread[n], y, x] = True
    return live


def pair_walk(image, mu, live, by, bx):
    """One pair of tiles: {(channel, y, x): row of 64 float32} of its live nodes, the way the gather wave computes and places them."""
    c_in, h_in, w_in, _ = mu.shape
    _, h_out, w_out = live.shape
    jn = LANE & 31
    hf, cl, px = jn >> 4, (jn & 15) >> 1, jn & 1
    y, x = by + hf, 2 * bx + px
    valid = (y < h_out) & (x < w_out)
    need = valid & live[cl, np.minimum(y, h_out - 1), np.minimum(x, w_out - 1)]
    bal = int(sum(1 << int(i) for i in range(32) if need[i]))
    if bal == 0:
        return {}
    popc = lambda v: bin(v & 0xffffffff).count("1")      # noqa: E731
    # column c of group k of position q = 2 hf + p stands for channel 4 k + c, i.e. pair lane 16 hf + blk_dst(2 p + k, lane)
    off = [[4 * k + (LANE & 3) for k in range(2)] for q in range(4)]
    # ---- the walk: 3 x 6 window rows, each fetched once ----
    acc = [[np.zeros((64, 4), np.float32) for k in range(2)] for q in range(4)]
    wy0, wx0 = by * STRIDE - PAD, 2 * bx * STRIDE - PAD
    issued = 0
    for cs in range(c_in):
        for wy in range(WY):
            iy = wy0 + wy
            r = [mu[cs, iy, wx0 + xx] if 0 <= iy < h_in and 0 <= wx0 + xx < w_in else np.zeros(64, np.float32) for xx in range(6)]
            for h in range(2):
                if not (wy >= 2 if h else wy < 4):
                    continue
                taps = image[0, cs * KH + (wy - 2 if h else wy)].reshape(16, 4)      # the 16-byte pieces of an image row: piece = channel (position 0's half)
                for p in range(2):
                    q = 2 * h + p
                    for k in range(2):
                        for kx in range(4):
                            acc[q][k] = mfma_4x4x1_16b(r[kx + 2 * p], taps[off[q][k], kx], acc[q][k])
                            issued += 1
    # ---- the placement: ring rows in ballot order, written by the column lanes ----
    pos = np.array([popc(bal & ((1 << int(jn[i])) - 1)) for i in range(64)])
    mypos = np.where(need, pos, -1)
    ring = np.full((popc(bal), 64), np.nan, np.float32)
    written = np.zeros((popc(bal), 64), int)
    for q in range(4):
        for k in range(2):
            dst = 16 * (q >> 1) + 2 * off[q][k] + (q & 1)
            pd = mypos[dst]
            for lane in range(64):
                if pd[lane] >= 0:
                    ring[pd[lane], 4 * (lane >> 2):4 * (lane >> 2) + 4] = acc[q][k][lane]
                    written[pd[lane], 4 * (lane >> 2):4 * (lane >> 2) + 4] += 1
    assert np.all(written == 1), "every ring row written once, whole"
    assert issued == 12 * 4 * 8, issued
    return {(int(cl[i]), int(y[i]), int(x[i])): ring[pos[i]] for i in range(32) if need[i]}


GEOMS = {
    # output h x w: (input h, w, forced live counts: upper tile / lower tile / the unpaired last row)
    "5x6": (10, 12, {(0, 0): 0, (0, 1): 1, (2, 2): 4, (2, 3): 5, (0, 5): 8, (1, 0): 0, (1, 1): 1, (3, 2): 4, (3, 3): 5, (1, 4): 8,
                      (4, 0): 0, (4, 1): 1, (4, 2): 4, (4, 3): 5, (4, 5): 8}),
    "8x4": (16, 8, {(0, 0): 0, (2, 1): 1, (4, 2): 4, (6, 3): 5, (0, 3): 8, (1, 0): 0, (3, 1): 1, (5, 2): 4, (7, 3): 5, (1, 2): 8}),
}


@pytest.mark.parametrize("geom", list(GEOMS))
def test_pair_walk_reproduces_the_one_tile_walk_bit_for_bit(btlib, geom):
    h_in, w_in, forced = GEOMS[geom]
    w, mu = make(3, h_in, w_in, 8, 4, 7)
    mu[1, 3, 2, :5] = np.float32(1e-42)                                                  # subnormal rows ride through unflushed
    taken, g, image = host_image(btlib, w, h_in, w_in, STRIDE, PAD)
    assert taken == 1 and (g["lanes"], g["CT"], g["PY"], g["PX"], g["WX"], g["ncy"]) == (16, 8, 1, 2, 6, 12)
    h_out, w_out = h_in // 2, w_in // 2
    live = live_mask(h_out, w_out, 3, forced)
    counts = live.sum(0)
    for (y, x), n in forced.items():
        assert counts[y, x] == n
    want = block_form_aggregate(w, mu, STRIDE, PAD, image=image)
    got = {}
    for by in range(0, h_out, 2):
        for bx in range(w_out // 2):
            rows = pair_walk(image, mu, live, by, bx)
            assert not set(rows) & set(got)
            got.update(rows)
    assert set(got) == {(int(c), int(y), int(x)) for c, y, x in np.argwhere(live)}
    for (c, y, x), row in got.items():
        assert np.array_equal(row.view(np.uint32), want[c, y, x].view(np.uint32)), (c, y, x)
