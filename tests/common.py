"""Shared helpers for the parity tests: golden fixtures -> batches, tolerances."""
import os
from functools import lru_cache

import numpy as np
import torch

from gnn_branching_amd import nets, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_CASES = ["cifar_base_kw_B3", "cifar_wide_kw_B2", "cifar_deep_kw_B2"]
FAMILIES = ["shipped", "random"]
STAGES = ["r0_fwd", "r0_bwd", "r1_fwd", "r1_bwd"]

# north_star: scores within 1e-4 (fp32, absolute) of the reference CPU forward.  The shipped checkpoint produces scores of
# magnitude 5..50 (the reference's own fp32-vs-fp64 noise there is ~1e-5), so 1e-4 is its bar.
SCORE_ATOL = 1e-4
# The seeded random weight set is the one that exercises the forward half-pass (the shipped checkpoint's forward weights are
# all subnormal); its scores lie in about [-1, 0.05] and the reference's own fp32 noise is 2..4e-7 there, so it gets a bar
# 20x tighter: 5e-6 absolute, or 1e-5 of the score range where scores are larger (other networks).
RANDOM_ATOL = 5e-6


def score_tol(fam, want=None):
    """Absolute tolerance for a weight family; `want`: the finite reference scores (for the range rule)."""
    if fam == "shipped":
        return SCORE_ATOL
    rng = float(np.max(want) - np.min(want)) if want is not None and np.size(want) else 0.0
    return max(RANDOM_ATOL, 1e-5 * rng)


@lru_cache(None)
def shipped_state():
    d = dict(np.load(os.path.join(nets.ASSETS, "cifar_trained_gnn.npz")))
    order = [str(k) for k in d.pop("__order__")]
    return {k: d[k] for k in order}


@lru_cache(None)
def random_state(seed=20240917):
    from oracle.gnn_oracle import random_gnn_state
    return random_gnn_state(seed)


def state_of(fam):
    return shipped_state() if fam == "shipped" else random_state()


@lru_cache(None)
def load_golden(case):
    g = dict(np.load(os.path.join(GOLDEN, case + ".npz")))
    net = str(g["net"])
    B = int(g["B"])
    props = [tuple(int(v) for v in pr) for pr in g["props"]]
    base = nets.build_net(net)
    cache = {}
    prop_layers = []
    for pr in props:
        if pr not in cache:
            cache[pr] = nets.fold_property(base, *pr)[-1]
        prop_layers.append(cache[pr])
    nl = sum(1 for k in g if k.startswith("lb"))
    lbs = [torch.from_numpy(g[f"lb{i}"]) for i in range(nl)]
    ubs = [torch.from_numpy(g[f"ub{i}"]) for i in range(nl)]
    duals = [torch.from_numpy(g[f"dual{i}"]) for i in range(nl - 2)]
    npm = sum(1 for k in g if k.startswith("primal") and k != "primal_input")
    primals = [torch.from_numpy(g[f"primal{i}"]) for i in range(npm)]
    bab = [torch.from_numpy(g[f"bab{i}"].astype(np.int64)) for i in range(nl - 2)]
    batch = synth.SubproblemBatch(lbs, ubs, duals, primals, torch.from_numpy(g["primal_input"]),
                                  {"fixed_layers": base[:-1], "prop_layers": prop_layers},
                                  torch.from_numpy(g["masks"].astype(np.float32)), bab)
    return g, batch


def relu_sizes(batch):
    return [int(np.prod(t.shape[1:])) for t in batch.lower_bounds_all[1:-1]]


# Networks other than the three CIFAR models (tests/test_gpu_generic_nets.py): each takes some of the engine's other kernels.
ARCHS = {
    # all-dense network: Flatten first, Linear edges only, top layer through k_top
    "toy_mlp": [("flatten",), ("linear", 3 * 32 * 32, 128), ("relu",), ("linear", 128, 64), ("relu",), ("linear", 64, 10)],
    # 3x3 stride-1 first conv (8192-node layer), stride-2 second conv, narrow Linear head
    "toy_conv3": [("conv", 3, 8, 3, 1, 1), ("relu",), ("conv", 8, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 8 * 16 * 16, 48),
                  ("relu",), ("linear", 48, 10)],
    # last ReLU layer with 200 nodes: too wide for k_top, separate dense / update / property kernels
    "toy_widehead": [("conv", 3, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 8 * 16 * 16, 200), ("relu",), ("linear", 200, 10)],
    # channel counts the VALU fallback kernels are not compiled for (12, 6): MFMA gather tables only
    "toy_oddch": [("conv", 3, 12, 3, 1, 1), ("relu",), ("conv", 12, 6, 4, 2, 1), ("relu",), ("flatten",), ("linear", 6 * 16 * 16, 32),
                  ("relu",), ("linear", 32, 10)],
    # kernel sizes / strides without a compile-time stencil in the bias-sum pass: 5x5 stride 1 pad 2, 2x2 stride 2 pad 0
    "toy_k5": [("conv", 3, 8, 5, 1, 2), ("relu",), ("conv", 8, 8, 2, 2, 0), ("relu",), ("flatten",), ("linear", 8 * 16 * 16, 40),
               ("relu",), ("linear", 40, 10)],
    # a 32768-node layer under the Linear head: too long for k_top's live-row list (LDS), so its forward edge walks every row
    "toy_longk": [("conv", 3, 32, 3, 1, 1), ("relu",), ("flatten",), ("linear", 32 * 32 * 32, 72), ("relu",), ("linear", 72, 10)],
    # a single ReLU layer (L = 1)
    "toy_single": [("conv", 3, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 8 * 16 * 16, 10)],
}


def register_toy_archs():
    """Register ARCHS with nets (seeded random weights; the seeds are fixed by their order)."""
    for i, (name, spec) in enumerate(ARCHS.items()):
        nets.register_arch(name, spec, seed=100 + i)


# Networks for the limits of the online-learning step (tests/test_online_gradients.py).  A dict of their own, registered with seeds of
# their own: ARCHS parametrises other test files, and its seeds follow its order.
ONLINE_ARCHS = {
    # 4x4 stride-1 conv over 32 -> 32 channels: an interior node lists 4 * 4 * 32 = 512 taps in either direction, exactly what
    # the training conv kernel's tap lists hold (TCONV_MAXTAPS)
    "toy_taps512": [("conv", 3, 32, 4, 4, 0), ("relu",), ("conv", 32, 32, 4, 1, 1), ("relu",), ("flatten",), ("linear", 32 * 7 * 7, 24),
                    ("relu",), ("linear", 24, 10)],
    # 5x5 stride-1 conv over 32 channels: 800 taps, past the limit -- the online step refuses it
    "toy_taps800": [("conv", 3, 32, 4, 4, 0), ("relu",), ("conv", 32, 8, 5, 1, 2), ("relu",), ("flatten",), ("linear", 8 * 8 * 8, 24),
                    ("relu",), ("linear", 24, 10)],
}


def register_online_archs():
    for i, (name, spec) in enumerate(ONLINE_ARCHS.items()):
        nets.register_arch(name, spec, seed=300 + i)


# Networks at the clamped tap bound of the learning step (tests/test_online_geometry.py): name -> (input shape, spec).  gnnb_online_step
# admits a conv edge whose largest tap list, min(k, extent) per axis forward and min(ceil(k / s), extent) transposed, is at most 512.
ONLINE_GEOM_ARCHS = {
    # 5x5 stride 1 over a 4x4 layer of 32 channels: 25 * 32 = 800 unclamped, 4 * 4 * 32 = 512 clamped in both directions, and the four
    # centre nodes list all 512; only the min(k, extent) clamp admits it
    "onl_clamp512": ((3, 16, 16), [("conv", 3, 32, 4, 4, 0), ("relu",), ("conv", 32, 32, 5, 1, 2), ("relu",), ("flatten",), ("linear", 512, 24),
                                   ("relu",), ("linear", 24, 10)]),
    # 8x8 stride 2 pad 3, 8 -> 32 channels on 16x16: forward 8 * 8 * 8 = 512, transposed ceil(8 / 2)^2 * 32 = 512, both reached by interior
    # nodes; only the ceil(k / s) term admits it
    "onl_s2_512": ((3, 16, 16), [("conv", 3, 8, 3, 1, 1), ("relu",), ("conv", 8, 32, 8, 2, 3), ("relu",), ("flatten",), ("linear", 2048, 24),
                                 ("relu",), ("linear", 24, 10)]),
    # the same 5x5 edge over a 5x4 layer: clamped bound 5 * 4 * 32 = 640, which node (y = 2, x = 2) really lists -- refused
    "onl_clamp640": ((3, 20, 16), [("conv", 3, 32, 4, 4, 0), ("relu",), ("conv", 32, 32, 5, 1, 2), ("relu",), ("flatten",), ("linear", 640, 24),
                                   ("relu",), ("linear", 24, 10)]),
}


def register_online_geom_archs():
    """Register ONLINE_GEOM_ARCHS with nets (seeds 700 + i, fixed by their order)."""
    for i, (name, (_, spec)) in enumerate(ONLINE_GEOM_ARCHS.items()):
        nets.register_arch(name, spec, seed=700 + i)


def _mlp_deep8():
    spec, n = [("flatten",)], 3 * 8 * 8
    for _ in range(8):
        spec += [("linear", n, 32), ("relu",)]
        n = 32
    return spec + [("linear", 32, 10)]


# Geometries for the Wong-Kolter bounds and BaBSR kernels (tests/test_gpu_kw_geometry.py, tests/test_gpu_babsr_geometry.py):
# name -> (input shape, spec).  Channel counts in {3, 8, 16, 32} (bind accepts them without MFMA gather tables); the widest ReLU
# layer stays at or below the 4096 nodes of the Wong-Kolter LDS limit except in kwg_over.
KW_ARCHS = {
    # Linear first layer: the input is a flat layer
    "kwg_mlp": ((3, 8, 8), [("flatten",), ("linear", 192, 64), ("relu",), ("linear", 64, 48), ("relu",), ("linear", 48, 10)]),
    # stride-1 support boxes that grow through two layers; L = 4
    "kwg_s1": ((3, 16, 16), [("conv", 3, 8, 3, 1, 1), ("relu",), ("conv", 8, 8, 3, 1, 1), ("relu",), ("conv", 8, 16, 4, 2, 1), ("relu",),
                             ("flatten",), ("linear", 1024, 32), ("relu",), ("linear", 32, 10)]),
    # non-square input, 5x5 kernel, pad 0
    "kwg_rect": ((3, 12, 20), [("conv", 3, 8, 5, 1, 2), ("relu",), ("conv", 8, 16, 2, 2, 0), ("relu",), ("flatten",), ("linear", 960, 24),
                               ("relu",), ("linear", 24, 10)]),
    # stride larger than the kernel (pixels no window reads), 1x1 conv (a one-pixel support box)
    "kwg_gap": ((3, 20, 14), [("conv", 3, 8, 2, 3, 0), ("relu",), ("conv", 8, 16, 1, 1, 0), ("relu",), ("flatten",), ("linear", 560, 16),
                              ("relu",), ("linear", 16, 10)]),
    # L = 1: graph layer 1 and the property node only
    "kwg_single": ((3, 16, 16), [("conv", 3, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 512, 10)]),
    # L = 8 = MAXL, the deepest network bind accepts
    "kwg_deep8": ((3, 8, 8), _mlp_deep8()),
    # a 4096-node ReLU layer: exactly the Wong-Kolter LDS limit (2 x 4096 doubles = 64 KiB) / one node past it
    "kwg_cap": ((3, 8, 8), [("flatten",), ("linear", 192, 4096), ("relu",), ("linear", 4096, 16), ("relu",), ("linear", 16, 10)]),
    "kwg_over": ((3, 8, 8), [("flatten",), ("linear", 192, 4097), ("relu",), ("linear", 4097, 16), ("relu",), ("linear", 16, 10)]),
}


def register_kw_archs():
    """Register KW_ARCHS with nets (seeded random weights; the seeds are fixed by their order)."""
    for i, (name, (_, spec)) in enumerate(KW_ARCHS.items()):
        nets.register_arch(name, spec, seed=200 + i)


# Input shapes and conv geometries for the forward scorer (tests/test_gpu_forward_geometry.py): name -> (input shape, spec).  A dict of
# its own, registered with seeds of its own: ARCHS' seeds follow its order and parametrise golden files.  What each one covers:
FWD_ARCHS = {
    # H != W, 5x5, pad 0, a tile map with NBY = 6, NBX = 10
    "fwg_rect": KW_ARCHS["kwg_rect"],
    # stride > kernel on edge 1 (not normalised, so legal): input pixels no window reads; edge 1 has no transposed tables, so the
    # VALU k_convT_bwd + k_input_update run behind a conv; 1x1 windows
    "fwg_gap": KW_ARCHS["kwg_gap"],
    # L = 4, odd extents (17x5, 9x3), widths below every tile width, origin -1 on the transposed 4/2/1
    "fwg_tall": ((3, 34, 10), [("conv", 3, 8, 4, 2, 1), ("relu",), ("conv", 8, 8, 3, 1, 1), ("relu",), ("conv", 8, 16, 3, 2, 1), ("relu",),
                               ("flatten",), ("linear", 432, 32), ("relu",), ("linear", 32, 10)]),
    # kernel larger than the image (2x2, then 1x1), one mostly-masked tile per sample, a conv as the last edge
    "fwg_tiny": ((3, 4, 4), [("conv", 3, 8, 4, 2, 1), ("relu",), ("conv", 8, 8, 4, 2, 1), ("relu",), ("flatten",), ("linear", 8, 10)]),
    # inner edge with forward MFMA tables and NO transposed tables: the normalised VALU transposed conv, tap counts 16..49
    "fwg_k7": ((3, 8, 8), [("conv", 3, 8, 3, 1, 1), ("relu",), ("conv", 8, 8, 7, 1, 3), ("relu",), ("flatten",), ("linear", 512, 20),
                           ("relu",), ("linear", 20, 10)]),
    # inner edge with no tables in either direction, between MFMA neighbours
    "fwg_valu": ((3, 6, 6), [("conv", 3, 16, 3, 1, 1), ("relu",), ("conv", 16, 32, 5, 1, 2), ("relu",), ("flatten",), ("linear", 1152, 24),
                             ("relu",), ("linear", 24, 10)]),
    # L = 8 = MAXL, Linear first layer
    "fwg_deep8": KW_ARCHS["kwg_deep8"],
    # a flat input that is not 3072 wide through k_embed and the dense kernels
    "fwg_mlp": KW_ARCHS["kwg_mlp"],
    # L = 1 at 16x16
    "fwg_single": KW_ARCHS["kwg_single"],
}
# An inner conv with stride > kernel: pixels of layer 1 that no window of edge 2 reads have a tap count of 0, by which the reference
# divides (0/0).  The scoring entry points refuse it; bind, kw_bounds and babsr accept it.
ZERO_TAP_ARCH = ("fwg_zerotap", (3, 18, 12), [("conv", 3, 8, 4, 2, 1), ("relu",), ("conv", 8, 8, 2, 3, 1), ("relu",), ("flatten",),
                                              ("linear", 96, 16), ("relu",), ("linear", 16, 10)])


def register_fwd_archs():
    """Register FWD_ARCHS (seeds 500 + i, fixed by their order) and the zero-tap network (seed 599) with nets."""
    for i, (name, (_, spec)) in enumerate(FWD_ARCHS.items()):
        nets.register_arch(name, spec, seed=500 + i)
    nets.register_arch(ZERO_TAP_ARCH[0], ZERO_TAP_ARCH[2], seed=599)
