"""The online-learning step (gnnb_step.h gnnb_online_step, on the tape of gnnb_train.h) tensor by tensor against fp64 autograd.

tests/test_online.py bounds the gradient error by 2e-4 of the largest entry of the whole 52-tensor blob, which leaves every tensor whose
own entries are smaller than that unchecked (the input-layer chains, on some networks all twelve inp_* tensors).  Here each tensor
is held to the reference arithmetic's own error on THAT tensor:

    scale_t = max |g64_t|,  e_ref_t = max |g32_t - g64_t|,  e_hip_t = max |ghip_t - g64_t|
    e_hip_t <= K_BAR * max(e_ref_t, 2^-23 * scale_t)          (K_BAR = 4, see there; ReLU kinks: see KINK)

with g64 / g32 the autograd oracle (oracle/online_oracle.py) in fp64 / fp32 on the same inputs.  A tensor whose true gradient is below
fp32's range (scale_t < 1e-30) must come out finite and at most subnormal (<= 1.18e-38); which tensors may fall under that rule is
asserted per case, so it cannot swallow a tensor the kernels zeroed by mistake.

The cases reach every tile form of the chain kernels (4, 8 and 32 rows per block, both sides of both thresholds on a 256-CU device), the
networks that never took a step, T = 1, 2, 3, degenerate losses, masks and LP-like inputs.  The second half checks k_tadam against
the closed form of torch.optim.Adam in fp64 fed the kernel's own gradients, and the two limits gnnb_online_step guards."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_branching_amd import synth
from oracle.online_oracle import OnlineOracle, split_blob
from tests import margins
from tests.common import ARCHS, FAMILIES, load_golden, register_online_archs, register_toy_archs, score_tol, state_of

# Factor on the reference arithmetic's own error.  2 (what tests/test_gpu_stress.py uses for fp32 against fp64) is not enough for two
# fp32 summation orders: measured on the MI355X the worst ratio of a case without a ReLU-kink flip (below) was 3.57, on inp_b2.bias
# of cifar_wide_kw B = 8 (3.08 on base T = 3, 3.01 under the all-ones mask, 1.5 .. 2.7 elsewhere).  Worst times 1.5 would be 5.4;
# the bar stops at 4 because nothing past 4 may be waved through without knowing where the bits went.
K_BAR = 4.0
# What is past 4 has so far been one thing: the GNN is piecewise linear, a few of the ~10^7 ReLU pre-activations of a step lie within
# fp32 rounding of zero, and there the gate an fp32 evaluation takes depends on its summation order.  One such flip moves every
# tensor upstream of it by a whole gradient entry (toy_k5 B = 2: 1e-4 of scale on fc3 and the twelve inp_* tensors, 450 times the fp32
# oracle's error there; the fp32 oracle has such flips of its own, e.g. 4.5e-5 of scale on inp_f.weight of toy_conv3).  Both one-sided
# derivatives are right.  A case that misses the bar is therefore re-examined: the gates whose fp64 pre-activation is within KINK of
# its tensor's largest may flip, and the HIP gradient has to meet the SAME bar on every tensor against the fp64 gradient with a subset
# of them flipped.  KINK: a 192-term fp32 dot product is off by about sqrt(192) * 2^-24 of the size of its terms, 2^-20.
KINK = 2.0 ** -20
KINK_CANDIDATES = 64
EPS32 = 2.0 ** -23
BELOW_RANGE = 1e-30          # a tensor whose fp64 gradient is smaller everywhere is below what fp32 holds
FP32_MIN_NORMAL = 1.18e-38
FSCORE_BIAS = "ComputeFinalScore.fscore.bias"          # its gradient is exactly +1 - 1
INP_B = tuple(f"EmbedUpdates.update.{n}.{w}" for n in ("inp_b", "inp_b_1", "inp_b2", "inp_b2_2") for w in ("weight", "bias"))
PROPS = [(3, 5), (1, 7), (0, 2), (8, 4), (6, 9)]


def tile_rows(nrows, n_cu):
    """Rows per block Trainer::chain / chain_multi pick (gnnb_train.h tile_rows)."""
    return 4 if nrows <= 16 * n_cu else (8 if nrows <= 128 * n_cu else 32)


def make(net, B, seed):
    register_toy_archs()
    register_online_archs()
    return synth.make_batch(net, B, seed=seed, props=[PROPS[b % len(PROPS)] for b in range(B)])


def scored(mask_row):
    return mask_row.nonzero().view(-1)


def middle_kw(masks, shift=0):
    """A scored node from the middle of every sample's mask (the reference side asserts it is not the arg-max where that matters)."""
    out = []
    for b in range(masks.shape[0]):
        idx = scored(masks[b])
        out.append(int(idx[(len(idx) // 2 + shift) % len(idx)]))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Ref:
    """Both oracles on one set of inputs: named gradients, losses, padded scores, the arg-max node per sample."""

    def __init__(self, state, args, kws, imps, T=2):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.state, self.args, self.kws, self.imps, self.T = state, args, kws, imps, T
        masks = args[6]
        self.g, self.loss, self.scores = {}, {}, {}
        for dt in (torch.float64, torch.float32):
            o = OnlineOracle(state, T=T, dtype=dt)
            loss, ragged = o.step(args, kws, imps, apply=False)
            self.g[dt] = split_blob(o.grad_blob().astype(np.float64), state)
            self.loss[dt] = np.asarray(loss, np.float64)
            pad = np.full(tuple(masks.shape), -np.inf)
            for b, s in enumerate(ragged):
                pad[b, scored(masks[b]).numpy()] = s.double().numpy()
            self.scores[dt] = pad
        self.argmax = [int(np.argmax(self.scores[torch.float64][b])) for b in range(masks.shape[0])]      # first maximum

    def below_range(self):
        return [k for k, v in self.g[torch.float64].items() if float(np.abs(v).max()) < BELOW_RANGE]


def tensor_ratios(ref, ghip, g64):
    """name -> e_hip / max(e_ref, 2^-23 scale) for the tensors in fp32's range (e_ref always against the unflipped fp64 gradient)."""
    out = {}
    for name in ref.state:
        scale = float(np.abs(ref.g[torch.float64][name]).max())
        if scale >= BELOW_RANGE:
            yard = max(float(np.abs(ref.g[torch.float32][name] - ref.g[torch.float64][name]).max()), EPS32 * scale)
            h = ghip[name].astype(np.float64)
            out[name] = float(np.abs(h - g64[name]).max()) / yard if np.isfinite(h).all() else float("inf")
    return out


def explained_by_relu_kinks(case, ref, ghip, k_bar):
    """See KINK.  Greedy: the candidate gates in order of the gradient entry they pass, each kept if it brings the worst ratio down.
    Returns (worst ratio reached, the flips kept)."""
    from oracle.online_oracle import ReluTap

    def grad_with(flips):
        o = OnlineOracle(ref.state, T=ref.T, dtype=torch.float64)
        tap = ReluTap(flips)
        o.step(ref.args, ref.kws, ref.imps, apply=False, relu_tap=tap)
        return split_blob(o.grad_blob().astype(np.float64), ref.state), tap

    g0, tap = grad_with({})
    cands = []
    for i, (z, y) in enumerate(tap.calls):
        if y.grad is None:
            continue
        near = ((z.abs() <= KINK * float(z.abs().max())) & (y.grad != 0)).reshape(-1).nonzero().view(-1)
        cands += [(abs(float(y.grad.reshape(-1)[j])), i, int(j)) for j in near]
    cands.sort(reverse=True)
    flips, best = {}, max(tensor_ratios(ref, ghip, g0).values())
    for gy, i, j in cands[:KINK_CANDIDATES]:
        if best <= k_bar:
            break
        trial = {k: list(v) for k, v in flips.items()}
        trial.setdefault(i, []).append(j)
        w = max(tensor_ratios(ref, ghip, grad_with(trial)[0]).values())
        if w < 0.9 * best:
            flips, best = trial, w
            print(f"  {case}: ReLU call {i} entry {j} (|gy| {gy:.3e}) on the other side of its kink: worst ratio {best:.2f}")
    return best, flips


def check_gradient(case, ref, ghip_blob, zero_ok, k_bar=K_BAR):
    """The per-tensor rule of the module docstring.  zero_ok: names that may fall under the below-range rule, or "all".
    Prints every figure, records the worst ratio, then asserts."""
    g64 = ref.g[torch.float64]
    g32 = ref.g[torch.float32]
    ghip = split_blob(np.asarray(ghip_blob, np.float32), ref.state)
    bad, worst, worst_t, under = [], 0.0, None, []
    for name in ref.state:
        h = ghip[name].astype(np.float64)
        scale = float(np.abs(g64[name]).max())
        if scale < BELOW_RANGE:
            under.append(name)
            big = float(np.abs(h).max()) if np.isfinite(h).all() else float("inf")
            if zero_ok != "all" and name not in zero_ok:
                bad.append(f"{name}: true gradient below fp32's range (scale {scale:.3e}), not expected for this case")
            if not big <= FP32_MIN_NORMAL:
                bad.append(f"{name}: true gradient below fp32's range (scale {scale:.3e}) but max |ghip| = {big:.3e}")
            continue
        e_ref = float(np.abs(g32[name] - g64[name]).max())
        e_hip = float(np.abs(h - g64[name]).max()) if np.isfinite(h).all() else float("inf")
        yard = max(e_ref, EPS32 * scale)
        ratio = e_hip / yard
        if ratio > worst:
            worst, worst_t = ratio, name
        print(f"  {case} {name}: scale {scale:.3e} e_ref {e_ref:.3e} ({e_ref / scale:.1e} of scale) e_hip {e_hip:.3e} ratio {ratio:.2f}")
        if not e_hip <= k_bar * yard:
            bad.append(f"{name}: e_hip {e_hip:.3e} > {k_bar} * max(e_ref {e_ref:.3e}, 2^-23 * scale {scale:.3e}) (ratio {ratio:.2f})")
    print(f"{case}: worst e_hip / max(e_ref, 2^-23 scale) = {worst:.2f} on {worst_t}; below fp32's range: {under}")
    margins.record("online_gradients", case, worst_ratio=worst, worst_tensor=worst_t, below_range=",".join(under), k_bar=k_bar)
    if bad and all("e_hip" in b for b in bad) and np.isfinite(worst):
        after, flips = explained_by_relu_kinks(case, ref, ghip, k_bar)
        print(f"{case}: with {sum(len(v) for v in flips.values())} ReLU gate(s) within 2^-20 of zero flipped in the fp64 oracle: worst ratio {after:.2f}")
        margins.record("online_gradients", case, worst_ratio_after_kink_flips=after, n_kink_flips=sum(len(v) for v in flips.values()))
        assert after <= k_bar, f"{case}: {after:.2f} after the kink flips {flips}; before:\n" + "\n".join(bad)
        return worst
    assert not bad, f"{case}:\n" + "\n".join(bad)
    return worst


def check_loss_and_argmax(case, ref, loss_hip, scores_hip, k_bar=K_BAR):
    s64, s32 = ref.scores[torch.float64], ref.scores[torch.float32]
    got = scores_hip.cpu().numpy()
    worst = 0.0
    for b in range(s64.shape[0]):
        fin = np.isfinite(s64[b])
        assert np.array_equal(np.isfinite(got[b]), fin), (case, b)
        yard = max(abs(ref.loss[torch.float32][b] - ref.loss[torch.float64][b]), EPS32 * float(np.abs(s64[b][fin]).max()))
        err = abs(float(loss_hip[b]) - ref.loss[torch.float64][b])
        worst = max(worst, err / yard)
        print(f"  {case} loss[{b}]: hip {loss_hip[b]:.7g} fp64 {ref.loss[torch.float64][b]:.7g} err {err:.3e} yard {yard:.3e}")
        assert err <= k_bar * yard, (case, b, err, yard)
        e_ref = float(np.abs(s32[b][fin] - s64[b][fin]).max())
        top = np.sort(s64[b][fin])[::-1]
        if len(top) == 1 or top[0] - top[1] > 4 * e_ref:
            assert int(np.argmax(got[b])) == ref.argmax[b], (case, b, "arg-max node differs from the oracle's")
    margins.record("online_gradients", case, worst_loss_ratio=worst)


def hip_step(state, args, kws, imps, T=2, eng=None):
    from gnn_branching_amd.engine import ScorerEngine
    if eng is None:
        eng = ScorerEngine(state, T=T)
        eng.online_create()
    w0 = eng.get_weights()
    loss, scores = eng.online_step(args, kws, imps, apply=False, want_scores=True)
    np.testing.assert_array_equal(eng.get_weights(), w0)
    return eng, loss, scores, eng.online_grad()


def run_case(case, fam, args, kws, imps, T=2, zero_ok=(FSCORE_BIAS,), kw_is_argmax=False):
    state = state_of(fam)
    ref = Ref(state, args, kws, imps, T)
    for b, kw in enumerate(kws):
        assert (kw == ref.argmax[b]) == kw_is_argmax, (case, b, kw, ref.argmax[b])
    if fam == "random" and zero_ok != "all":           # the below-range rule is a condition, not a waiver
        assert sorted(ref.below_range()) == sorted(zero_ok), (case, ref.below_range())
    _, loss, scores, g = hip_step(state, args, kws, imps, T)
    check_loss_and_argmax(case, ref, loss, scores)
    check_gradient(case, ref, g, zero_ok if fam == "random" else "all")
    return ref, g


def imps_for(B):
    return [(0.3, 0.01, 0.0, 0.12)[b % 4] for b in range(B)]


# ---- A: the two forms of the oracle are the same function (runs anywhere) -------------------------------------------------
def test_fp64_oracle_is_the_fp32_oracle():
    """cifar_base_kw_B3, random family: per tensor the fp32 autograd gradient is within 1e-6 of the tensor's scale of the fp64 one
    (measured 6.9e-7 at worst), and only fscore.bias (+1 - 1) is below fp32's range."""
    _, batch = load_golden("cifar_base_kw_B3")
    args = batch.forward_args()
    ref = Ref(state_of("random"), args, middle_kw(batch.masks), [0.05, 0.2, 0.0])
    assert ref.below_range() == [FSCORE_BIAS]
    for name, g64 in ref.g[torch.float64].items():
        scale = float(np.abs(g64).max())
        if scale >= BELOW_RANGE:
            assert float(np.abs(ref.g[torch.float32][name] - g64).max()) <= 1e-6 * scale, name
    np.testing.assert_allclose(ref.loss[torch.float32], ref.loss[torch.float64], rtol=0, atol=1e-5)


def test_split_blob_follows_checkpoint_order():
    state = state_of("random")
    blob = np.concatenate([np.asarray(v).reshape(-1) for v in state.values()])
    parts = split_blob(blob, state)
    assert list(parts) == list(state) and len(parts) == 52
    for k, v in state.items():
        np.testing.assert_array_equal(parts[k], np.asarray(v))


# ---- B: per-tensor gradient parity -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_tile_form_in_one_step():
    """cifar_base_kw B = 17: input chains 52 224 rows and layer 1 34 816 (32-row tiles), layer 2 17 408 (8-row), layer 3 1 700 (4-row)
    on a 256-CU device."""
    batch = make("cifar_base_kw", 17, seed=31)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = [17 * t[0].numel() for t in batch.lower_bounds_all[:-1]]
    assert rows == [52224, 34816, 17408, 1700]
    if n_cu == 256:
        assert [tile_rows(r, n_cu) for r in rows] == [32, 32, 8, 4]
    run_case("base_B17", "random", batch.forward_args(), middle_kw(batch.masks), imps_for(17))


@pytest.mark.gpu
def test_long_dense_sums():
    """toy_longk B = 2: the 32-row form under dense edges, k_tdense over 32 768 source rows.  fp32 autograd itself is ~1e-3 of scale off
    fp64 on fc3.weight here (sums over 32 768 rows), the yardstick follows it."""
    batch = make("toy_longk", 2, seed=11)
    run_case("toy_longk_B2", "random", batch.forward_args(), middle_kw(batch.masks), imps_for(2))


@pytest.mark.gpu
@pytest.mark.parametrize("B,layer1_rows,form", [(1, 4096, 4), (2, 8192, 8), (8, 32768, 8), (9, 36864, 32)])
def test_both_sides_of_both_tile_thresholds(B, layer1_rows, form):
    """cifar_wide_kw: layer 1 has 4096 nodes, so B = 1 / 2 sit on either side of the 4-row threshold (16 rows per CU) and B = 8 / 9 on
    either side of the 8-row one (128 per CU) of a 256-CU device."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if n_cu != 256:
        pytest.skip(f"the tile thresholds are 16 and 128 rows per CU: {n_cu} CUs put them elsewhere than 4096 / 32768 rows")
    batch = make("cifar_wide_kw", B, seed=40 + B)
    assert batch.lower_bounds_all[1][0].numel() * B == layer1_rows and tile_rows(layer1_rows, n_cu) == form
    run_case(f"wide_B{B}", "random", batch.forward_args(), middle_kw(batch.masks), imps_for(B))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in ARCHS if n != "toy_longk"] + ["cifar_base_kw", "cifar_wide_kw", "cifar_deep_kw"])
def test_every_network_at_B2(name):
    """All of ARCHS (toy_longk B = 2 is test_long_dense_sums) and the three CIFAR networks with the per-tensor bar."""
    batch = make(name, 2, seed=11)
    run_case(f"{name}_B2", "random", batch.forward_args(), middle_kw(batch.masks), imps_for(2))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_shipped_golden_inputs(fam):
    """cifar_base_kw_B3 golden inputs.  With the shipped checkpoint (forward weights subnormal) about half of the tensors have true
    gradients below fp32's range: they must come out finite and at most subnormal."""
    _, batch = load_golden("cifar_base_kw_B3")
    run_case(f"golden_B3_{fam}", fam, batch.forward_args(), middle_kw(batch.masks), [0.05, 0.2, 0.0])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3])
def test_rounds(T):
    """T = 1 has no input-layer update: the eight inp_b* gradients are exactly zero on both sides."""
    batch = make("cifar_base_kw", 2, seed=21)
    zero_ok = (FSCORE_BIAS,) + (INP_B if T == 1 else ())
    run_case(f"base_B2_T{T}", "random", batch.forward_args(), middle_kw(batch.masks), imps_for(2), T=T, zero_ok=zero_ok)


@pytest.mark.gpu
def test_kw_is_the_argmax():
    """loss = improvement; +1 - 1 cancel exactly in ds and in k_tscore_bwd_w, so every gradient entry is a zero; apply=True then
    moves the parameters by weight decay alone."""
    from gnn_branching_amd.engine import ScorerEngine
    batch = make("cifar_base_kw", 2, seed=21)
    args, state = batch.forward_args(), state_of("random")
    kws = Ref(state, args, middle_kw(batch.masks), [0.0, 0.0]).argmax
    imps = [0.25, 0.5]
    ref, g = run_case("base_B2_kw_argmax", "random", args, kws, imps, zero_ok="all", kw_is_argmax=True)
    assert len(ref.below_range()) == 52 and not g.any()
    lr, wd = 1e-3, 1e-2
    eng = ScorerEngine(state)
    eng.online_create(lr, wd)
    w0 = eng.get_weights()
    loss, _ = eng.online_step(args, kws, imps)
    np.testing.assert_array_equal(loss, np.asarray(imps, np.float32))
    # Adam's first step on g = wd p alone is p - lr g / (|g| + eps).  The bar is 1e-4 of the step plus the rounding of p: a dozen fp32
    # operations of 2^-23 relative error each stay far below it (the precise check of k_tadam is test_adam_matches_closed_form)
    w1 = eng.get_weights().astype(np.float64)
    p = w0.astype(np.float64)
    want = p - lr * (wd * p) / (np.abs(wd * p) + 1e-8)
    excess = np.abs(w1 - want) - (1e-4 * lr + np.spacing(np.abs(w0)))
    assert excess.max() <= 0, (int(excess.argmax()), float(w0[excess.argmax()]), float(w1[excess.argmax()]), float(want[excess.argmax()]))


@pytest.mark.gpu
def test_same_subproblem_twice_and_zero_improvement():
    """Two samples that are the same subproblem: the gradient is twice the single one.  Improvement 0 on both."""
    one = make("cifar_base_kw", 1, seed=23)
    B2 = synth.SubproblemBatch([torch.cat([t, t]) for t in one.lower_bounds_all], [torch.cat([t, t]) for t in one.upper_bounds_all],
                               [torch.cat([t, t]) for t in one.dual_vars], [torch.cat([t, t]) for t in one.primals],
                               torch.cat([one.primal_inputs] * 2),
                               {"fixed_layers": one.layers["fixed_layers"], "prop_layers": one.layers["prop_layers"] * 2},
                               torch.cat([one.masks] * 2))
    kw = middle_kw(one.masks)
    ref, _ = run_case("base_same_twice", "random", B2.forward_args(), kw * 2, [0.0, 0.0])
    single = Ref(state_of("random"), one.forward_args(), kw, [0.0])
    for name, g in ref.g[torch.float64].items():
        np.testing.assert_allclose(g, 2 * single.g[torch.float64][name], rtol=1e-9, atol=1e-12 * float(np.abs(g).max()))


@pytest.mark.gpu
def test_all_ones_mask():
    """Dead and decided nodes scored too."""
    batch = make("cifar_base_kw", 2, seed=25)
    args = list(batch.forward_args())
    args[6] = torch.ones_like(batch.masks)
    run_case("base_B2_all_ones_mask", "random", args, middle_kw(args[6]), imps_for(2))


@pytest.mark.gpu
def test_one_scored_node_per_sample():
    """The only scored node is the arg-max and the KW node: a zero gradient, loss = improvement."""
    batch = make("cifar_base_kw", 2, seed=25)
    args = list(batch.forward_args())
    kws = middle_kw(batch.masks)
    args[6] = torch.zeros_like(batch.masks)
    for b, kw in enumerate(kws):
        args[6][b, kw] = 1.0
    run_case("base_B2_one_scored", "random", args, kws, imps_for(2), zero_ok="all", kw_is_argmax=True)


@pytest.mark.gpu
def test_lp_like_inputs():
    """Decided nodes with bounds clamped to exactly 0, signed duals of magnitude up to 1, compact lists of odd lengths."""
    from tests.test_gpu_stress import lp_like
    batch = make("cifar_base_kw", 2, seed=7)
    args = lp_like(batch, np.random.RandomState(1007), 1.0)
    run_case("base_B2_lp_like", "random", args, middle_kw(args[6]), imps_for(2))


@pytest.mark.gpu
def test_conv_exactly_at_the_tap_limit():
    """toy_taps512: the interior nodes of its 4x4 stride-1 32 -> 32 convolution list 512 taps in both directions."""
    batch = make("toy_taps512", 2, seed=13)
    run_case("toy_taps512_B2", "random", batch.forward_args(), middle_kw(batch.masks), imps_for(2))


# ---- properties --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_additivity():
    """The gradient of a B = 3 step is the sum of the three B = 1 gradients: both against the fp64 sum, with the fp32 oracle's
    error on that sum as the yardstick."""
    _, batch = load_golden("cifar_base_kw_B3")
    state = state_of("random")
    kws, imps = middle_kw(batch.masks), [0.05, 0.2, 0.0]
    ones = [Ref(state, batch.slice(b, b + 1).forward_args(), kws[b:b + 1], imps[b:b + 1]) for b in range(3)]
    ref = Ref(state, batch.forward_args(), kws, imps)
    for dt in (torch.float64, torch.float32):
        ref.g[dt] = {k: sum(o.g[dt][k] for o in ones) for k in state}
    eng, _, _, g3 = hip_step(state, batch.forward_args(), kws, imps)
    check_gradient("additivity_B3", ref, g3, (FSCORE_BIAS,))
    gsum = np.zeros(g3.size, np.float64)
    for b in range(3):
        gsum += hip_step(state, batch.slice(b, b + 1).forward_args(), kws[b:b + 1], imps[b:b + 1], eng=eng)[3]
    check_gradient("additivity_sum_of_B1", ref, gsum.astype(np.float32), (FSCORE_BIAS,))


@pytest.mark.gpu
def test_no_state_carried_between_steps():
    """B = 17, then B = 1 on the same engine: gradient, loss and scores bit-equal to a fresh engine's.  Then another network
    (the trainer caches the edge weights of the bound one), and back."""
    state = state_of("random")
    big, one, mlp = make("cifar_base_kw", 17, seed=31), make("cifar_base_kw", 1, seed=33), make("toy_mlp", 2, seed=11)
    kw1 = middle_kw(one.masks)
    _, loss0, scores0, g0 = hip_step(state, one.forward_args(), kw1, [0.1])
    eng, _, _, _ = hip_step(state, big.forward_args(), middle_kw(big.masks), imps_for(17))
    for other in (None, mlp):
        if other is not None:
            _, _, _, gm = hip_step(state, other.forward_args(), middle_kw(other.masks), imps_for(2), eng=eng)
            np.testing.assert_array_equal(bits(gm), bits(hip_step(state, other.forward_args(), middle_kw(other.masks), imps_for(2))[3]))
        _, loss, scores, g = hip_step(state, one.forward_args(), kw1, [0.1], eng=eng)
        np.testing.assert_array_equal(bits(g), bits(g0))
        np.testing.assert_array_equal(bits(loss), bits(loss0))
        np.testing.assert_array_equal(bits(scores.cpu().numpy()), bits(scores0.cpu().numpy()))


@pytest.mark.gpu
def test_step_is_deterministic():
    """gnnb_k_train.h promises fixed-order sums: the same step twice gives bit-equal gradients."""
    state = state_of("random")
    batch = make("cifar_base_kw", 17, seed=31)
    kws, imps = middle_kw(batch.masks), imps_for(17)
    eng, loss_a, _, ga = hip_step(state, batch.forward_args(), kws, imps)
    _, loss_b, _, gb = hip_step(state, batch.forward_args(), kws, imps, eng=eng)
    np.testing.assert_array_equal(bits(ga), bits(gb))
    np.testing.assert_array_equal(bits(loss_a), bits(loss_b))


# ---- C: Adam against its closed form -----------------------------------------------------------------------------------
ADAM_STEPS = 5
ADAM_SEED = 33          # the fp64 oracle's five Adam steps stay finite at every (lr, wd) below (test_adam_case_stays_finite)


def adam_case():
    one = make("cifar_base_kw", 1, seed=ADAM_SEED)
    return one, middle_kw(one.masks), [0.1]


@pytest.mark.parametrize("lr", [1e-4, 1e-2])
@pytest.mark.parametrize("wd", [0.0, 1e-4, 1e-2])
def test_adam_case_stays_finite(lr, wd):
    """A case whose loss stops being finite would be a bad case, not a pass: five fp64 steps of the oracle stay finite (CPU)."""
    one, kw, imp = adam_case()
    o = OnlineOracle(state_of("random"), lr=lr, wd=wd, dtype=torch.float64)
    for _ in range(ADAM_STEPS):
        loss, _ = o.step(one.forward_args(), kw, imp)
        assert np.isfinite(loss).all() and np.isfinite(o.blob()).all() and np.isfinite(o.grad_blob()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lr", [1e-4, 1e-2])
@pytest.mark.parametrize("wd", [0.0, 1e-4, 1e-2])
def test_adam_matches_closed_form(lr, wd):
    """Five steps; after each the kernel's own gradient g and the parameters p.  fp64: torch.optim.Adam's rule written out, from the
    same start, fed g.  Yardstick: torch.optim.Adam itself on fp32 tensors fed g.  Every parameter:
    |p_hip - p64| <= 2 * max over its tensor |p32 - p64| + ulp32(p).
    Measured on the MI355X: at most 0.76 of that bar (lr = 1e-2, wd = 0, step 3).  Before 1 - b1 and 1 - b2 reached the kernel rounded
    once from double it was 9.9 at lr = 1e-2 from step 1 on: 1.0f - 0.999f is 1.3e-5 off 0.001, every step 6e-6 too long."""
    from gnn_branching_amd.engine import ScorerEngine
    from oracle.gnn_oracle import oracle_forward, padded_scores
    one, kw, imp = adam_case()
    state = state_of("random")
    eng = ScorerEngine(state)
    eng.online_create(lr, wd)
    w0 = eng.get_weights()
    p64, m64, v64 = w0.astype(np.float64), np.zeros(w0.size), np.zeros(w0.size)
    p32 = [torch.nn.Parameter(torch.from_numpy(np.array(v, np.float32))) for v in split_blob(w0, state).values()]
    opt = torch.optim.Adam(p32, lr=lr, weight_decay=wd)
    b1, b2, eps = 0.9, 0.999, 1e-8
    worst = 0.0
    for t in range(1, ADAM_STEPS + 1):
        loss, _ = eng.online_step(one.forward_args(), kw, imp)
        assert np.isfinite(loss).all()
        g, p_hip = eng.online_grad(), eng.get_weights()
        assert np.isfinite(g).all() and np.isfinite(p_hip).all()
        gd = g.astype(np.float64) + wd * p64
        m64 = b1 * m64 + (1 - b1) * gd
        v64 = b2 * v64 + (1 - b2) * gd * gd
        p64 = p64 - lr / (1 - b1 ** t) * m64 / (np.sqrt(v64) / np.sqrt(1 - b2 ** t) + eps)
        for p, gt in zip(p32, split_blob(g, state).values()):
            p.grad = torch.from_numpy(np.array(gt, np.float32))
        opt.step()
        ref32 = np.concatenate([p.detach().numpy().reshape(-1) for p in p32]).astype(np.float64)
        e_ref = split_blob(np.abs(ref32 - p64), state)
        yard = np.concatenate([np.full(v.size, float(v.max())) for v in e_ref.values()])
        e_hip = np.abs(p_hip.astype(np.float64) - p64)
        bar = 2 * yard + np.spacing(np.abs(p_hip)).astype(np.float64)
        ratio = float((e_hip / bar).max())
        worst = max(worst, ratio)
        i = int(np.argmax(e_hip / bar))
        print(f"  adam lr {lr:g} wd {wd:g} step {t}: worst |p_hip - p64| / bar = {ratio:.3f} (e_hip {e_hip[i]:.3e}, tensor yardstick {yard[i]:.3e}, p {p_hip[i]:.3e})")
        margins.record("online_adam", f"lr{lr:g}_wd{wd:g}", worst_ratio_to_bar=ratio)
        assert ratio <= 1.0, (lr, wd, t, ratio)
    # the fused scorer runs with the parameters the step left
    now = {k: torch.from_numpy(np.array(v, np.float32)) for k, v in split_blob(eng.get_weights(), state).items()}
    with torch.no_grad():
        want = padded_scores(oracle_forward(now, *one.forward_args()), one.masks).numpy()
    got = eng.forward(*one.forward_args()).check().scores.cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert float(np.abs(got[fin] - want[fin]).max()) <= score_tol("random", want[fin])


@pytest.mark.gpu
def test_gradient_only_steps_leave_the_step_counter_alone():
    from gnn_branching_amd.engine import ScorerEngine
    one, kw, imp = adam_case()
    state = state_of("random")
    fresh = ScorerEngine(state)
    fresh.online_create(1e-3, 1e-4)
    fresh.online_step(one.forward_args(), kw, imp)
    eng = ScorerEngine(state)
    eng.online_create(1e-3, 1e-4)
    w0 = eng.get_weights()
    for _ in range(3):
        eng.online_step(one.forward_args(), kw, imp, apply=False)
        np.testing.assert_array_equal(bits(eng.get_weights()), bits(w0))
    eng.online_step(one.forward_args(), kw, imp)
    np.testing.assert_array_equal(bits(eng.get_weights()), bits(fresh.get_weights()))      # bias correction of step 1, zero moments


@pytest.mark.gpu
def test_online_create_resets_and_set_weights_is_differentiated():
    from gnn_branching_amd.engine import ScorerEngine
    one, kw, imp = adam_case()
    state = state_of("random")
    eng = ScorerEngine(state)
    eng.online_create(1e-3, 1e-4)
    for _ in range(2):
        eng.online_step(one.forward_args(), kw, imp)
    w2 = eng.get_weights()
    assert np.abs(w2 - np.concatenate([np.asarray(v).reshape(-1) for v in state.values()])).max() > 1e-4
    fresh = ScorerEngine({k: np.array(v, np.float32) for k, v in split_blob(w2, state).items()})
    fresh.online_create(1e-3, 1e-4)
    np.testing.assert_array_equal(bits(fresh.get_weights()), bits(w2))
    eng.online_create(1e-3, 1e-4)              # moments and counter back to zero: the next step is a first step from w2
    la, _ = eng.online_step(one.forward_args(), kw, imp)
    lb, _ = fresh.online_step(one.forward_args(), kw, imp)
    np.testing.assert_array_equal(bits(la), bits(lb))
    np.testing.assert_array_equal(bits(eng.online_grad()), bits(fresh.online_grad()))
    np.testing.assert_array_equal(bits(eng.get_weights()), bits(fresh.get_weights()))
    # set_weights between steps: the next step differentiates what was set
    w0 = np.concatenate([np.asarray(v).reshape(-1) for v in state.values()]).astype(np.float32)
    eng.set_weights(w0)
    _, _, _, g = hip_step(state, one.forward_args(), kw, imp, eng=eng)
    np.testing.assert_array_equal(bits(g), bits(hip_step(state, one.forward_args(), kw, imp)[3]))


# ---- D: the two limits of the step -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_conv_past_the_tap_limit_is_refused():
    """toy_taps800 (5x5 stride 1 over 32 channels: 800 taps): the scorer takes it, the online step refuses it before anything is
    launched, and the handle goes on working."""
    from gnn_branching_amd.engine import ScorerEngine
    from oracle.gnn_oracle import oracle_forward, padded_scores
    state = state_of("random")
    big, one = make("toy_taps800", 2, seed=13), make("cifar_base_kw", 1, seed=33)
    eng = ScorerEngine(state)
    eng.online_create()
    with torch.no_grad():
        want = padded_scores(oracle_forward(state, *big.forward_args()), big.masks).numpy()
    got = eng.forward(*big.forward_args()).check().scores.cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and fin.any()
    assert float(np.abs(got[fin] - want[fin]).max()) <= score_tol("random", want[fin])
    with pytest.raises(Exception, match="ReLU layer 2"):
        eng.online_step(big.forward_args(), middle_kw(big.masks), [0.1, 0.2], apply=False)
    kw1 = middle_kw(one.masks)
    _, loss, _, g = hip_step(state, one.forward_args(), kw1, [0.1], eng=eng)
    _, loss0, _, g0 = hip_step(state, one.forward_args(), kw1, [0.1])
    np.testing.assert_array_equal(bits(g), bits(g0))
    np.testing.assert_array_equal(bits(loss), bits(loss0))


@pytest.mark.gpu
def test_sample_with_an_empty_mask():
    """Through the C entry point (ScorerEngine.online_step refuses a KW node outside the mask): B = 2, sample 1's mask empty.
    loss[1] is NaN; loss[0] and the gradient are bit-equal to sample 0 stepped alone."""
    from gnn_branching_amd import _lib
    from gnn_branching_amd.engine import ScorerEngine, make_batch
    state = state_of("random")
    batch = make("cifar_base_kw", 2, seed=21)
    kws = middle_kw(batch.masks)
    _, loss0, _, g0 = hip_step(state, batch.slice(0, 1).forward_args(), kws[:1], [0.1])
    args = list(batch.forward_args())
    args[6] = batch.masks.clone()
    args[6][1] = 0
    eng = ScorerEngine(state)
    eng.online_create()
    m = eng._marshal(*args)
    B = m.B
    kw = np.asarray(kws, np.int32)
    imp = np.asarray([0.1, 0.2], np.float32)
    loss = np.zeros(B, np.float32)
    cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
    with torch.cuda.device(eng.device):
        rc = eng.lib.gnnb_online_step(eng.h, C.byref(cb), B, kw.ctypes.data_as(C.c_void_p), imp.ctypes.data_as(C.c_void_p),
                                      loss.ctypes.data_as(C.c_void_p), None, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "gnnb_online_step")
    assert np.isnan(loss[1])
    np.testing.assert_array_equal(bits(loss[:1]), bits(loss0))
    np.testing.assert_array_equal(bits(eng.online_grad()), bits(g0))
