"""The block form of the forward tiles of edge 1 (tap products on v_mfma_f32_4x4x1_16b_f32, gnnb_k_gather.h gather_tile16_block) computes,
per destination node, the fma chain of the 16-column form without its structurally zero links: scores, decisions and the rows of layer 1
after the first forward half-pass are BIT-IDENTICAL to what the library computed before the block form existed.

tests/golden/blocktap_parent.npz was recorded once with that library (tools/blocktap_record.py, which imports the cases and the run from
this file).  It holds, per case and weight family: the fp32 scores, the decisions, and one 64-bit signature per row of layer 1 (the rows
themselves are 0.5 - 1.5 MB per case; the signature is a position-weighted sum of a row's 64 bit patterns, so any changed bit of any
channel changes it) -- of an inspection run limited to the first half-pass, with and without the fused half-pass kernel (fuse = 0).

The cases: cifar_base_kw (B = 2) and fwg_tiny (kernel larger than the image: every tile is a border tile) get the tile [8, 1, 2] and take
the block form; fwg_tall (17 x 5 outputs, tile [8, 2, 1]) and fwg_rect (5 x 5, stride 1) keep the 16-column form and pin that nothing
moved there.  Both weight families: the shipped forward weights are subnormal, the seeded random ones are not.  The block form issues
every channel group of a tile (dead groups are not skipped yet), so a position without a live node is no path of its own in it; the
batches still hold one (fwg_tall), beside partly and fully live positions and border tiles (test_batches_hold_every_kind_of_position)."""
from functools import lru_cache
import os

import numpy as np
import pytest
import torch

from gnn_branching_amd import synth
from tests.common import FWD_ARCHS, GOLDEN, FAMILIES, register_fwd_archs, state_of

gpu = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "blocktap_parent.npz")
PROPS = [(3, 5), (1, 7), (0, 2)]
# name -> (B, seed, eps, input shape); the seeds: test_batches_hold_every_kind_of_position
CASES = {"cifar_base_kw": (2, 11, 0.02, (3, 32, 32)), "fwg_tall": (3, 5, 0.002, FWD_ARCHS["fwg_tall"][0]),
         "fwg_rect": (3, 5, 0.005, FWD_ARCHS["fwg_rect"][0]), "fwg_tiny": (3, 6, 0.02, FWD_ARCHS["fwg_tiny"][0])}
FIRST_CONV_421 = ("cifar_base_kw", "fwg_tall", "fwg_tiny")      # first convolution 3 -> 8 channels, 4 x 4, stride 2, pad 1
PATHS = {"default": {}, "fuse0": {"fuse": 0}}
SIG_WEIGHTS = (2 * np.arange(64, dtype=np.uint64) + 1) * np.uint64(0x9E3779B97F4A7C15)


@lru_cache(None)
def batch_of(name):
    register_fwd_archs()
    B, seed, eps, shape = CASES[name]
    return synth.make_batch(name, B, seed=seed, eps=eps, props=PROPS[:B], input_shape=shape)


def row_signatures(rows):
    """(B, N, 64) float32 -> (B, N) uint64: sum over the channels of bit pattern x odd 64-bit weight (mod 2^64)."""
    bits = np.ascontiguousarray(rows, dtype=np.float32).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        return (bits * SIG_WEIGHTS).sum(-1, dtype=np.uint64)


def run_case(name, fam, options):
    """{scores, decisions, row_sig} of one case on the library in use."""
    from gnn_branching_amd.engine import ScorerEngine
    batch = batch_of(name)
    eng = ScorerEngine(state_of(fam), options=options)
    with torch.no_grad():
        res = eng.forward(*batch.forward_args()).check()
        assert int(res.status.cpu()[0]) == 0
        out = {"scores": res.scores.cpu().numpy(), "decisions": res.decisions.cpu().numpy()}
        eng.set_halfpass_limit(1)
        try:
            eng.forward(*batch.forward_args()).check()
            out["row_sig"] = row_signatures(eng.mu(batch.batch_size, 1).numpy())
        finally:
            eng.set_halfpass_limit(0)
    return out


def live_channels(name):
    """(B, H, W) int: live nodes (not blocked: ub > 0 or lb >= 0, node_is_live of gnnb_k_gather.h) among the channels of each position of layer 1."""
    batch = batch_of(name)
    lb, ub = batch.lower_bounds_all[1].numpy(), batch.upper_bounds_all[1].numpy()
    return ((ub > 0) | (lb >= 0)).sum(1)


def test_batches_hold_every_kind_of_position():
    """A condition on the inputs (CPU): among the cases with a 4/2/1 first convolution there is a position of layer 1 with no live node, a
    partly live and a fully live one, and tiles whose window leaves the image (pad 1: every tile of the first and last rows and columns)."""
    dead = part = full = 0
    for name in FIRST_CONV_421:
        live = live_channels(name)
        C = batch_of(name).lower_bounds_all[1].shape[1]
        assert C == 8
        counts = (int((live == 0).sum()), int(((live > 0) & (live < C)).sum()), int((live == C).sum()))
        print(f"{name}: positions with no / some / every channel live: {counts}; live nodes {int(live.sum())} of {live.size * C}")
        dead, part, full = dead + counts[0], part + counts[1], full + counts[2]
        if name in FWD_ARCHS:
            assert FWD_ARCHS[name][1][0] == ("conv", 3, 8, 4, 2, 1)                 # pad 1: the windows of the outermost tiles leave the image
    assert dead > 0 and part > 0 and full > 0, (dead, part, full)


@gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("name", list(CASES))
def test_bit_identical_to_the_recorded_parent(name, fam, path):
    want = np.load(FIXTURE)
    got = run_case(name, fam, PATHS[path])
    for what in ("scores", "decisions", "row_sig"):
        w = want[f"{name}/{fam}/{path}/{what}"]
        if what == "row_sig" and not np.array_equal(got[what], w):
            bad = np.argwhere(got[what] != w)
            print(f"{name} {fam} {path}: {len(bad)} rows of layer 1 differ, first (sample, node): {bad[:8].tolist()}")
        assert np.array_equal(got[what], w), (name, fam, path, what)
