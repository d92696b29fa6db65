"""The fused half-pass over edge 1 walks its block-form tiles in ROW PAIRS (gnnb_k_fusedq.h fusedq_gather_pairs, gnnb_k_gather.h
gather_pair16_block / _embed): the tiles (y, xp) and (y + 1, xp) of a sample together, every window row fetched or embedded once.  Per
destination node the tap products still run in (cs, ky, kx) order from a zero accumulator, so scores, decisions and the rows of layer 1 after
the first forward half-pass are BIT-IDENTICAL to what the library computed when every tile walked its own window.

tests/golden/blockpair_parent.npz was recorded once with that library (tools/blockpair_record.py, which imports the cases and the run from
this file): fp32 scores, decisions and one 64-bit signature per row of layer 1 (row_signatures of tests/test_gpu_blocktap.py), with and without
the fused half-pass kernel (fuse = 0: the stand-alone k_gather16 keeps the one-tile walk and is an on-device cross-check of the pair walk).

The cases: bpg_odd (layer 1 is 5 x 6: the last row is a pair without a lower tile), bpg_even (8 x 4), cifar_base_kw at B = 1 and B = 3 (rounds
of 8 pairs that end inside a sample and that span samples).  The seeded batches hold positions with 1 to 8 live channels but none without;
force_live_counts overwrites the layer-1 bounds of a few positions so that 0, exactly 4, exactly 5 and all 8 channels are live, each once in
an upper tile, once in a lower tile and (bpg_odd) once in the unpaired last row."""
from functools import lru_cache
import os

import numpy as np
import pytest
import torch

from gnn_branching_amd import nets, synth
from tests.common import FAMILIES, GOLDEN, state_of
from tests.test_gpu_blocktap import PATHS, PROPS, row_signatures

gpu = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "blockpair_parent.npz")
# (bpg_odd's second convolution is 3/1/1: a 4/2/1 one leaves a remainder on 5 x 6, which bind refuses)
ARCHS = {"bpg_odd": ((3, 10, 12), [("conv", 3, 8, 4, 2, 1), ("relu",), ("conv", 8, 8, 3, 1, 1), ("relu",), ("flatten",), ("linear", 240, 10)]),
         "bpg_even": ((3, 16, 8), [("conv", 3, 8, 4, 2, 1), ("relu",), ("conv", 8, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 64, 10)])}
# case -> (network, B, seed, input shape, {(sample, y, x) of layer 1: live channels forced})
_COUNTS = (0, 4, 5, 8)
CASES = {
    "bpg_odd": ("bpg_odd", 3, 3, ARCHS["bpg_odd"][0],
                {**{(i % 3, 0 + 2 * (i % 2), i): n for i, n in enumerate(_COUNTS)},               # upper tiles (rows 0, 2)
                 **{(i % 3, 1 + 2 * (i % 2), 5 - i): n for i, n in enumerate(_COUNTS)},           # lower tiles (rows 1, 3)
                 **{((i + 1) % 3, 4, 1 + i): n for i, n in enumerate(_COUNTS)}}),                 # the unpaired last row
    "bpg_even": ("bpg_even", 3, 5, ARCHS["bpg_even"][0],
                 {**{(i % 3, 2 * i, i): n for i, n in enumerate(_COUNTS)}, **{((i + 2) % 3, 2 * i + 1, 3 - i): n for i, n in enumerate(_COUNTS)}}),
    "base_B1": ("cifar_base_kw", 1, 7, (3, 32, 32),
                {**{(0, 4 * i, 3 + 3 * i): n for i, n in enumerate(_COUNTS)}, **{(0, 4 * i + 3, 14 - 3 * i): n for i, n in enumerate(_COUNTS)}}),
    "base_B3": ("cifar_base_kw", 3, 7, (3, 32, 32),
                {**{(i % 3, 4 * i + 2, 2 + 4 * i): n for i, n in enumerate(_COUNTS)}, **{((i + 1) % 3, 4 * i + 1, 15 - 4 * i): n for i, n in enumerate(_COUNTS)}}),
}
_SPREAD = {0: [], 4: [0, 3, 5, 6], 5: [1, 2, 4, 5, 7], 8: list(range(8))}


def register_archs():
    for i, (name, (_, spec)) in enumerate(ARCHS.items()):
        nets.register_arch(name, spec, seed=700 + i)


def is_live(lb, ub):
    """node_is_live of gnnb_k_gather.h: not blocked."""
    return (ub > 0) | (lb >= 0)


def force_live_counts(batch, forced):
    """Overwrite the bounds of layer 1 at the positions of `forced`: the channels of _SPREAD[n] keep their bounds when live and become
    ambiguous otherwise, every other channel becomes blocked; the ambiguity masks of the batch follow."""
    lb, ub = batch.lower_bounds_all[1], batch.upper_bounds_all[1]
    for (b, y, x), n in forced.items():
        for c in range(8):
            if c in _SPREAD[n]:
                if not bool(is_live(lb[b, c, y, x], ub[b, c, y, x])):
                    lb[b, c, y, x], ub[b, c, y, x] = -0.5, 0.25
            else:
                lb[b, c, y, x], ub[b, c, y, x] = -1.0, -0.25
    B = batch.batch_size
    for k, m in enumerate(batch.bab_masks):
        l2, u2 = batch.lower_bounds_all[k + 1].reshape(B, -1), batch.upper_bounds_all[k + 1].reshape(B, -1)
        m.zero_()
        m[(l2 < 0) & (u2 > 0)] = -1
        m[l2 >= 0] = 1
    batch.masks = torch.cat([(m == -1).float() for m in batch.bab_masks], 1)
    return batch


@lru_cache(None)
def batch_of(case):
    register_archs()
    net, B, seed, shape, forced = CASES[case]
    return force_live_counts(synth.make_batch(net, B, seed=seed, eps=0.02, props=PROPS[:B], input_shape=shape), forced)


def run_case(case, fam, options):
    """{scores, decisions, row_sig, status, describe} of one case on the library in use."""
    from gnn_branching_amd.engine import ScorerEngine
    batch = batch_of(case)
    eng = ScorerEngine(state_of(fam), options=options)
    with torch.no_grad():
        res = eng.forward(*batch.forward_args()).check()
        out = {"scores": res.scores.cpu().numpy(), "decisions": res.decisions.cpu().numpy(), "status": int(res.status.cpu()[0])}
        eng.set_halfpass_limit(1)
        try:
            r1 = eng.forward(*batch.forward_args()).check()
            out["status"] |= int(r1.status.cpu()[0])
            out["row_sig"] = row_signatures(eng.mu(batch.batch_size, 1).numpy())
        finally:
            eng.set_halfpass_limit(0)
    out["describe"] = eng.describe()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_batches_hold_the_forced_positions(case):
    """Conditions on the inputs (CPU): layer 1 has 8 channels; the forced positions exist, hold 0 / 4 / 5 / 8 live channels in an upper tile
    (even row), in a lower tile (odd row) and, for bpg_odd, in the unpaired last row; the rest of the batch keeps partly live positions."""
    batch = batch_of(case)
    lb, ub = batch.lower_bounds_all[1].numpy(), batch.upper_bounds_all[1].numpy()
    assert lb.shape[1] == 8
    H = lb.shape[2]
    live = is_live(lb, ub).sum(1)
    forced = CASES[case][4]
    where = {"upper": set(), "lower": set(), "last": set()}
    for (b, y, x), n in forced.items():
        assert live[b, y, x] == n, (b, y, x, n)
        where["last" if (H % 2 == 1 and y == H - 1) else "lower" if y % 2 else "upper"].add(n)
    assert where["upper"] == set(_COUNTS) and where["lower"] == set(_COUNTS)
    if case == "bpg_odd":
        assert H == 5 and where["last"] == set(_COUNTS)
    print(f"{case}: positions by live channels {np.bincount(live.ravel(), minlength=9).tolist()}")
    assert ((live > 0) & (live < 8)).sum() > len(forced)


@gpu
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_the_recorded_parent(case, fam):
    want = np.load(FIXTURE)
    runs = {path: run_case(case, fam, opts) for path, opts in PATHS.items()}
    fwd1 = [u for u in runs["default"]["describe"]["updates"] if u["update"] == "fwd" and u["layer"] == 1][0]
    # edge 1 takes the block form (blocktap_ok): tile [8, 1, 2] over a [4, 6] window, in the fused half-pass kernel
    assert fwd1["tile"] == [8, 1, 2] and fwd1["window"] == [4, 6] and fwd1["kernel"] == "k_gather_update" and fwd1["gather_ksteps"] == 20, fwd1
    for path, got in runs.items():
        assert got["status"] == 0, (case, fam, path)
        for what in ("scores", "decisions", "row_sig"):
            w = want[f"{case}/{fam}/{path}/{what}"]
            if what == "row_sig" and not np.array_equal(got[what], w):
                bad = np.argwhere(got[what] != w)
                print(f"{case} {fam} {path}: {len(bad)} rows of layer 1 differ, first (sample, node): {bad[:8].tolist()}")
            assert np.array_equal(got[what], w), (case, fam, path, what)
    # the pair walk of the fused kernel against the one-tile walk of the stand-alone gather, on the tree under test
    for what in ("scores", "decisions", "row_sig"):
        assert np.array_equal(runs["default"][what], runs["fuse0"][what]), (case, fam, what)
