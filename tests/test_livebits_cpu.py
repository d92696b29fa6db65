"""The live bitmap of a ReLU layer and how a sparse table build reads it (gnnb_k_mlp.h classify_block, gnnb_k_gather.h BitsLive), emulated
in numpy.

k_classify writes one 64-bit word per wave: the ballot of [r0 != 0] over the nodes [64 i, 64 i + 64) of the flat index g = b N + n, invalid
lanes 0.  A gather wave reads the region as 32-bit words: lane l of register w holds word w0 + 64 w + l with w0 = (b N) >> 5, and the build
finds node `row` of sample b at bit = ((b N) & 31) + row: register bit >> 11, lane (bit >> 5) & 63, bit position bit & 31.  The region ends
with LIVEBITS_PAD words nobody writes so that the lane load needs no guard.  The emulation takes the number of registers NBW as a parameter;
the library binds NBW = 1 (livebits_ok), wider layers keep the bounds."""
import os
import re

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn_branching_amd", "csrc")
POISON = 0xFFFFFFFF


def pad_words():
    """LIVEBITS_PAD of gnnb_k_gather.h."""
    src = open(os.path.join(CSRC, "gnnb_k_gather.h")).read()
    return int(re.search(r"#define LIVEBITS_PAD (\d+)", src).group(1))


def eligible(N, nbw=1):
    """livebits_ok: a sample's bit range [(bN) & 31, (bN) & 31 + N) fits NBW * 64 words for every b."""
    return (N if N % 32 == 0 else N + 31) <= 2048 * nbw


def bitmap_region(live, pad):
    """(B, N) bool -> the region as the gathers see it: uint32 words, the unwritten padding poisoned."""
    flat = live.reshape(-1)
    nwords = (flat.size + 63) // 64
    bits = np.zeros(nwords * 64, dtype=np.uint64)
    bits[:flat.size] = flat                                         # invalid lanes of the last wave ballot 0
    words = (bits.reshape(nwords, 64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)     # one ballot per wave
    return np.concatenate([words.view("<u4"), np.full(pad, POISON, dtype=np.uint32)])


def lookup(region, b, N, row, nbw):
    """BitsLive on sample b: the lane loads (counted against the region's size), then the permute lookup of `row`."""
    w0 = (b * N) >> 5
    idx = w0 + np.arange(64 * nbw)
    assert idx.max() < region.size, (b, N, int(idx.max()), region.size)      # the unguarded load stays inside the region
    regs = region[idx].reshape(nbw, 64)
    bit = ((b * N) & 31) + row
    assert (bit >> 11) < nbw, (b, N, row)
    word = regs[bit >> 11, (bit >> 5) & 63]
    return (int(word) >> (bit & 31)) & 1


@pytest.mark.parametrize("N,B", [(100, 3), (2048, 2), (2047, 3), (240, 5)])
def test_every_row_of_every_sample_finds_its_bit(N, B):
    rng = np.random.RandomState(N + B)
    nbw = 1 if eligible(N, 1) else 2
    assert eligible(N, nbw)
    pad = pad_words() * nbw
    for live in (rng.uniform(size=(B, N)) < 0.54, np.ones((B, N), dtype=bool), np.zeros((B, N), dtype=bool)):
        live = live.copy()
        live[B - 1, N - 1] = not live[B - 1, N - 2]                 # the very last node differs from its neighbour
        region = bitmap_region(live, pad)
        assert region.size == 2 * ((B * N + 63) // 64) + pad
        for b in range(B):
            got = np.array([lookup(region, b, N, row, nbw) for row in range(N)], dtype=bool)
            assert np.array_equal(got, live[b]), (N, B, b, np.flatnonzero(got != live[b])[:8])


def test_padding_is_what_the_last_sample_needs():
    """Without the padding words the last sample's load would leave the region: the layout's padding is needed, and it is enough."""
    pad = pad_words()
    assert pad == 64
    N, B = 100, 3
    region = bitmap_region(np.ones((B, N), dtype=bool), 0)
    with pytest.raises(AssertionError):
        lookup(region, B - 1, N, 0, 1)
    lookup(bitmap_region(np.ones((B, N), dtype=bool), pad), B - 1, N, N - 1, 1)


def test_eligibility_at_its_boundaries():
    """N % 32 == 0: every sample starts a word, N <= 2048 NBW bits fit.  Otherwise a sample can start at bit 31: N + 31 <= 2048 NBW."""
    assert eligible(2048) and not eligible(2049) and not eligible(2080)
    assert eligible(2017) and not eligible(2018) and not eligible(2047)
    assert eligible(2047, 2) and eligible(4096, 2) and not eligible(4097, 2) and eligible(4065, 2) and not eligible(4066, 2)
    assert eligible(1) and eligible(32) and eligible(240)
    # the rule never admits a layer whose highest bit leaves the registers, and is exact where N is odd (a sample can start at any bit) or a
    # multiple of 32 (every sample starts at bit 0)
    for N in (31, 100, 240, 2016, 2017, 2018, 2019, 2047, 2048, 2049, 2080):
        fits = (max(((b * N) & 31) + N - 1 for b in range(64)) >> 5) < 64
        assert fits or not eligible(N), N
        if N % 2 == 1 or N % 32 == 0:
            assert eligible(N) == fits, N
    src = open(os.path.join(CSRC, "gnnb_k_gather.h")).read()
    assert "return (Ns % 32 == 0 ? Ns : Ns + 31) <= 2048;" in src      # the rule the host binds by, as emulated here
