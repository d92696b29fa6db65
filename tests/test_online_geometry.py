"""The learning step (csrc/gnnb_step.h: gnnb_online_step, gnnb_online_step_rows, gnnb_imitation_step_rows) on input shapes and conv
geometries other than 3x32x32.  The training kernels work out layer extents, tap lists, tap counts and row offsets on their own, apart
from the forward scorer's plan, so the networks tests/test_gpu_forward_geometry.py added for the scorer (tests/common.py FWD_ARCHS: stride >
kernel on edge 1, a 1x1 convolution, odd extents with origin -1 on a transposed 4/2/1, windows larger than the image, a convolution as
the last edge, a 7x7 kernel, L = 1 at 16x16, L = 8 = T_MAXL) are run here through the step, per tensor against fp64 autograd under
tests/test_online_gradients.py's yardstick:

    e_hip_t <= K_BAR * max(e_ref_t, 2^-23 * scale_t),   K_BAR = 4, with that file's ReLU-kink re-examination

and three networks of their own (tests/common.py ONLINE_GEOM_ARCHS) sit on the clamps of gnnb_online_step's tap bound, min(k, extent)
per axis forward and min(ceil(k / s), extent) transposed: two with a clamped bound of exactly 512 = TCONV_MAXTAPS that a node reaches,
one at 640, which is refused.

The tests without the `gpu` mark are conditions on the inputs and hold for the reference alone: the cases are well-posed (the fp32
oracle flips no ReLU gate of its own: e_ref <= 1e-5 of every tensor's scale), the bar sees the smallest indexing error one can make,
the tap counts behind every acceptance and refusal are what plain loops over the positions count, and the imitation cases are decided
by no hinge gate."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from gnn_branching_amd import synth
from oracle.online_oracle import OnlineOracle, split_blob
from tests import margins, test_gpu_imitation as tgi, test_online_gradients as tog
from tests.common import FWD_ARCHS, ONLINE_GEOM_ARCHS, ZERO_TAP_ARCH, register_fwd_archs, register_online_geom_archs, state_of
from tests.imitation_twin import ImitationOracle
from tests.test_gpu_forward_geometry import PROPS, _mutations, conv_edges
from tests.test_gpu_imitation import MARGIN, NEAR_ZERO, new_engine, seeded_table, step_rows
from tests.test_online_gradients import (FSCORE_BIAS, INP_B, K_BAR, Ref, check_gradient, check_loss_and_argmax,      # noqa: F401  (run_case calls it)
                                          hip_step, imps_for, middle_kw, run_case)

gpu = pytest.mark.gpu
ALL_ARCHS = {**FWD_ARCHS, **ONLINE_GEOM_ARCHS, ZERO_TAP_ARCH[0]: ZERO_TAP_ARCH[1:]}
# network -> (batch seed, eps, B, shift of the KW node from the middle of the mask).  Chosen so that test_cases_are_well_posed holds: the seeds
# of tests/test_gpu_forward_geometry.py do not (the fp32 oracle flips ReLU gates of its own on fwg_rect, fwg_gap and fwg_single there, 2e-3
# to 5e-3 of a tensor's scale, which would widen the yardstick to about 1 % of scale).
CASES = {"fwg_rect": (1, 0.005, 3, 0), "fwg_gap": (1, 0.02, 3, 0), "fwg_tall": (5, 0.002, 3, 0), "fwg_tiny": (4, 0.02, 3, 0),
         "fwg_k7": (5, 0.003, 3, 0), "fwg_deep8": (377, 0.0001, 3, 0), "fwg_mlp": (5, 0.02, 3, 0), "fwg_single": (1, 0.02, 3, 0),
         "onl_clamp512": (1, 0.02, 3, 0), "onl_s2_512": (1, 0.005, 2, 0)}
# refused by the step: batches only for the refusal itself
REFUSED = {"onl_clamp640": (1, 0.005, 2, 0), "fwg_valu": (5, 0.003, 2, 0), ZERO_TAP_ARCH[0]: (5, 0.02, 2, 0)}
NAMES = list(CASES)
E_REF_CAP = 1e-5            # of a tensor's scale: a kink flip of the fp32 oracle is 1e-4 and more; measured 8.8e-7 .. 2.2e-6
# index (in the layer list) of the convolution whose last kernel column is zeroed; fwg_gap's second convolution is 1 wide (its last
# column is the whole kernel), so its first one stands in
MUTATED_CONV = {"fwg_rect": 2, "fwg_gap": 0, "fwg_tall": 4, "fwg_tiny": 0, "fwg_k7": 2, "fwg_deep8": None, "fwg_mlp": None, "fwg_single": 0,
                "onl_clamp512": 2, "onl_s2_512": 2}
E = "EmbedUpdates.update."
both = lambda names: tuple(E + n + w for n in names for w in (".weight", ".bias"))      # noqa: E731
# The chains that read edge k directly: the forward update of layer k gathers A mu[k-1] into fc3 (fc3_2, fc4, fc4_2 behind it); the backward
# update of layer k-1 gathers A^T mu[k] into bc3 (bc3_1, bc4, bc4_1 behind it), or, for edge 1, the input update into inp_b2 (inp_b2_2).
# The property layer is read by out1 / out2 / out3 forward and by the backward chains of the last ReLU layer.
UPDATE_CHAINS = both(["fc3", "fc3_2", "fc4", "fc4_2"])
BACKWARD_CHAINS = both(["bc3", "bc3_1", "bc4", "bc4_1"])
INPUT_CHAINS = both(["inp_b2", "inp_b2_2"])
PROPERTY_CHAINS = both(["out1", "out2", "out3"])


def register():
    register_fwd_archs()
    register_online_geom_archs()


@lru_cache(None)
def batch_of(name, B=None):
    """The case's batch (B: another batch size from the same seed, for the row forms)."""
    register()
    seed, eps, b, _ = {**CASES, **REFUSED}[name]
    B = b if B is None else B
    return synth.make_batch(name, B, seed=seed, eps=eps, props=PROPS[:B], input_shape=ALL_ARCHS[name][0])


def kws_of(name, batch=None):
    return middle_kw((batch or batch_of(name)).masks, CASES[name][3])


@lru_cache(None)
def ref_of(name, T=2):
    """Both oracles on the case, computed once, shared by every test and never written to."""
    batch = batch_of(name)
    ref = Ref(state_of("random"), batch.forward_args(), kws_of(name), imps_for(batch.batch_size), T)
    for g in ref.g.values():
        for v in g.values():
            v.setflags(write=False)
    return ref


def yardsticks(ref):
    """name -> (scale, max(e_ref, 2^-23 scale)) for the tensors in fp32's range."""
    out = {}
    for name in ref.state:
        g64, g32 = ref.g[torch.float64][name], ref.g[torch.float32][name]
        scale = float(np.abs(g64).max())
        if scale >= tog.BELOW_RANGE:
            out[name] = (scale, max(float(np.abs(g32 - g64).max()), tog.EPS32 * scale))
    return out


# ---- CPU: the cases are well-posed, the bar sees an indexing error, the tap counts ---------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cases_are_well_posed(name):
    """Every sample has at least two scored nodes, no KW node is the fp64 arg-max, only fscore.bias (+1 - 1) is below fp32's range, the
    FWD_ARCHS batches have every node class in every ReLU layer, and the fp32 oracle is within 1e-5 of every tensor's scale of the fp64
    one: it flipped no ReLU gate of its own, so the yardstick is fp32 rounding and nothing wider."""
    batch, ref = batch_of(name), ref_of(name)
    assert int(batch.n_ambiguous().min()) >= 2
    for b, kw in enumerate(ref.kws):
        assert kw != ref.argmax[b], (name, b, kw)
    assert ref.below_range() == [FSCORE_BIAS]
    if name in FWD_ARCHS:
        for r, m in enumerate(batch.bab_masks):
            assert bool((m == -1).any()) and bool((m == 1).any()) and bool((m == 0).any()), (name, r)
    rel = {t: (yard / scale, float(np.abs(ref.g[torch.float32][t] - ref.g[torch.float64][t]).max()) / scale) for t, (scale, yard) in yardsticks(ref).items()}
    worst = max(rel, key=lambda t: rel[t][1])
    print(f"{name}: worst e_ref / scale = {rel[worst][1]:.2e} on {worst}; scored nodes per sample {batch.n_ambiguous().tolist()}")
    assert len(rel) == 51 and rel[worst][1] <= E_REF_CAP, (worst, rel[worst])


def mutated_gradients(name):
    """(what, chains that must move, {tensor: |g_mut - g64| / yardstick}) per mutation, from the fp64 oracle on mutated `layers`."""
    batch, ref = batch_of(name), ref_of(name)
    yard = yardsticks(ref)
    for what, layers in _mutations(name, batch, conv=-1 if MUTATED_CONV[name] is None else MUTATED_CONV[name], archs=ALL_ARCHS):
        args = list(batch.forward_args())
        args[5] = layers
        o = OnlineOracle(ref.state, T=ref.T, dtype=torch.float64)
        o.step(args, ref.kws, ref.imps, apply=False)
        g = split_blob(o.grad_blob().astype(np.float64), ref.state)
        if what.startswith("property"):
            chains = PROPERTY_CHAINS + BACKWARD_CHAINS
        else:
            chains = UPDATE_CHAINS + (INPUT_CHAINS if MUTATED_CONV[name] == 0 else BACKWARD_CHAINS)
        yield what, chains, {t: float(np.abs(g[t] - ref.g[torch.float64][t]).max()) / y for t, (_, y) in yard.items()}


@pytest.mark.parametrize("name", NAMES)
def test_the_bar_sees_an_indexing_error(name):
    """The last kernel column of one convolution zeroed, or the property layers of samples 0 and 1 exchanged (the two mutations of
    tests/test_gpu_forward_geometry.py), in the fp64 oracle against the unmutated fp64 gradient: at least half of the tensors move by more
    than 10 bars, among them every tensor of the chains that read the mutated edge."""
    n_mut = 0
    for what, chains, ratio in mutated_gradients(name):
        past = [t for t, r in ratio.items() if r > 10 * K_BAR]
        print(f"{name}: {what}: {len(past)} of {len(ratio)} tensors past {10 * K_BAR:g}, median ratio {np.median(list(ratio.values())):.3g}, "
              f"least of the chains {min(ratio[t] for t in chains):.3g}")
        assert 2 * len(past) >= len(ratio), (name, what, len(past))
        assert not [t for t in chains if t not in past], (name, what, [(t, ratio[t]) for t in chains if t not in past])
        n_mut += 1
    assert n_mut == (1 if MUTATED_CONV[name] is None else 2)


def tap_counts(c_in, c_out, k, s, pad, h_in, w_in):
    """(largest forward tap list, largest transposed tap list) of one conv edge, counted position by position."""
    h_out, w_out = (h_in + 2 * pad - k) // s + 1, (w_in + 2 * pad - k) // s + 1
    fwd = bwd = 0
    for oy in range(h_out):
        for ox in range(w_out):
            n = sum(1 for ky in range(k) for kx in range(k) if 0 <= oy * s - pad + ky < h_in and 0 <= ox * s - pad + kx < w_in)
            fwd = max(fwd, n * c_in)
    for y in range(h_in):
        for x in range(w_in):
            n = 0
            for ky in range(k):
                for kx in range(k):
                    ty, tx = y + pad - ky, x + pad - kx
                    n += ty % s == 0 and tx % s == 0 and 0 <= ty // s < h_out and 0 <= tx // s < w_out
            bwd = max(bwd, n * c_out)
    return fwd, bwd


def test_tap_limit_arithmetic():
    """The largest tap list of every conv edge of every network of this file, forward and transposed, counted in plain loops: 512 / 512 on
    the two networks at the limit, 640 and 800 on the two refused ones, at most 512 everywhere else.  (Edge 1 is in the count although its
    transposed form is never normalised: the step runs it in both directions.)"""
    got = {}
    for name in ALL_ARCHS:
        for i, ci, co, k, s, pad, h, w in conv_edges(name, ALL_ARCHS):
            got[(name, i)] = tap_counts(ci, co, k, s, pad, h, w)
            print(name, f"conv {ci} -> {co} {k}x{k}/{s}/{pad} on {h}x{w}:", got[(name, i)])
    assert got.pop(("onl_clamp512", 2)) == (512, 512)
    assert got.pop(("onl_s2_512", 2)) == (512, 512)
    assert got.pop(("onl_clamp640", 2)) == (640, 640)
    assert got.pop(("fwg_valu", 2)) == (400, 800)
    assert len(got) >= 14 and all(max(v) <= 512 for v in got.values()), got


# ---- A: the online step, per tensor ---------------------------------------------------------------------------------------------------
def record_as_geometry(monkeypatch):
    """What check_gradient and check_loss_and_argmax put on record (before they assert) goes to the section "online_geometry"."""
    record = margins.record
    monkeypatch.setattr(margins, "record", lambda section, key, **f: record("online_geometry" if section == "online_gradients" else section, key, **f))


def online_case(name, T, monkeypatch):
    """run_case on the case, with the shared reference in place of a second evaluation of both oracles."""
    batch, ref = batch_of(name), ref_of(name, T)
    monkeypatch.setattr(tog, "Ref", lambda state, args, kws, imps, T_: ref if (T_ == T and kws == ref.kws) else Ref(state, args, kws, imps, T_))
    record_as_geometry(monkeypatch)
    zero_ok = (FSCORE_BIAS,) + (INP_B if T == 1 else ())
    case = f"{name}_B{batch.batch_size}" + ("" if T == 2 else f"_T{T}")
    run_case(case, "random", batch.forward_args(), kws_of(name), imps_for(batch.batch_size), T=T, zero_ok=zero_ok)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_online_step_per_tensor(name, monkeypatch):
    """T = 2, random family: loss and arg-max (check_loss_and_argmax) and every gradient tensor (check_gradient).  onl_clamp512 and
    onl_s2_512 are the two networks that only the clamps of the tap bound admit: their nodes list exactly 512 taps.
    Measured on the MI355X: worst ratio 0.44 (fwg_deep8) .. 0.74 (fwg_k7); 0.63 on onl_clamp512, 0.72 on onl_s2_512 (1.63 .. 3.29 with
    fp32 accumulators in the training kernels, fwg_rect at 6.57 before one ReLU kink flip)."""
    online_case(name, 2, monkeypatch)


@gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("name", ["fwg_gap", "fwg_tall"])
def test_online_step_rounds(name, T, monkeypatch):
    """T = 1 has no input-layer update (the eight inp_b* gradients are exactly zero on both sides); at T = 3 edge 1 runs transposed and
    unnormalised twice.

    Measured on the MI355X: worst ratio 0.55 / 0.73 at T = 1 and 0.49 / 0.59 at T = 3 (fwg_gap / fwg_tall).  With fp32 accumulators in
    the training kernels both T = 3 cases missed the bar on one tensor, EmbedUpdates.update.inp_f.bias, with no ReLU gate within 2^-20
    of zero to explain it:

        fwg_gap_B3_T3   scale 5.358e-15  e_ref 1.602e-21 (3.0e-7 of scale)  e_hip 6.671e-21 (1.2e-6 of scale)  ratio 4.16
        fwg_tall_B3_T3  scale 1.215e-20  e_ref 1.055e-26 (8.7e-7 of scale)  e_hip 4.471e-26 (3.7e-6 of scale)  ratio 4.24

    inp_f enters the scores through the longest path of the step (mu[0] of round 0, then every sweep of all three rounds in sequence),
    and the error was the rounding inside every sum of products on that path: an fp32 oracle with its Linears evaluated in fp64 and
    rounded once has a tenth to a quarter of the plain fp32 oracle's error on these tensors, one whose Linears merely add in another
    order has the same error.  The kernels now accumulate every such sum in fp64 and round once (csrc/gnnb_k_train.h, "Precision")."""
    online_case(name, T, monkeypatch)


# ---- B: the imitation step, per tensor ------------------------------------------------------------------------------------------------
# (network, candidates per sample or None for every undecided node, table seed): the table seeds were chosen so that
# test_the_imitation_cases_are_decided_by_no_hinge_gate holds
IMIT_CASES = [("fwg_gap", 16, 1), ("fwg_gap", None, 1), ("fwg_tall", 16, 1), ("fwg_tall", None, 1), ("fwg_k7", 16, 1), ("fwg_k7", None, 1),
              ("fwg_single", 16, 1), ("fwg_single", None, 1), ("fwg_deep8", 16, 1), ("fwg_deep8", None, 1), ("onl_clamp512", 16, 1),
              ("onl_clamp512", None, 1)]
IMIT_IDS = [f"{n}_{'all' if m is None else 'M%d' % m}" for n, m, _ in IMIT_CASES]


@lru_cache(None)
def imit_case(case):
    name, M, tseed = IMIT_CASES[IMIT_IDS.index(case)]
    batch = batch_of(name)
    table = seeded_table(batch.masks.numpy(), M, tseed)
    return batch, table, tgi.Ref(state_of("random"), batch.forward_args(), table, MARGIN, 2)


@pytest.mark.parametrize("case", IMIT_IDS)
def test_the_imitation_cases_are_decided_by_no_hinge_gate(case):
    """The precondition of test_imitation_step_per_tensor, on the CPU (tests/test_gpu_imitation.py states why): the fp32 and the fp64 twin
    have the same violators, no fp64 term lies within 1e-3 of zero, every sample has a violator, only fscore.bias has a zero gradient."""
    _, _, ref = imit_case(case)
    assert ref.violators[torch.float32] == ref.violators[torch.float64]
    near = min(abs(v) for terms in ref.terms[torch.float64] for v in terms.values())
    print(case, "violators", [len(v) for v in ref.violators[torch.float64]], "of", [len(t) + 1 for t in ref.terms[torch.float64]], "closest term", near)
    assert near >= NEAR_ZERO, near
    assert all(len(v) >= 1 for v in ref.violators[torch.float64])
    assert ref.below_range() == [FSCORE_BIAS]
    yard = yardsticks(ref)          # and, as for the online cases, no ReLU kink flip of the fp32 twin in the yardstick (measured <= 5.2e-6)
    assert len(yard) == 51 and all(float(np.abs(ref.g[torch.float32][t] - ref.g[torch.float64][t]).max()) <= E_REF_CAP * s for t, (s, _) in yard.items())


@gpu
@pytest.mark.parametrize("case", IMIT_IDS)
def test_imitation_step_per_tensor(case, monkeypatch):
    """As tests/test_gpu_imitation.py test_gradient_per_tensor_against_fp64: violator and candidate counts, the loss, fscore.bias == [0.0],
    and every tensor under the yardstick with the kink re-examination (the imitation twin in OnlineOracle's place)."""
    batch, table, ref = imit_case(case)
    eng = new_engine(T=2)
    w0 = eng.get_weights()
    loss, report, regret = eng.imitation_step(batch.forward_args(), table, MARGIN, apply=False)
    np.testing.assert_array_equal(eng.get_weights(), w0)
    g = eng.online_grad()
    assert report[:, 3].tolist() == [len(v) for v in ref.violators[torch.float64]]
    assert report[:, 2].tolist() == [len(t) + 1 for t in ref.terms[torch.float64]]
    for b in range(len(loss)):
        yard = max(abs(ref.loss[torch.float32][b] - ref.loss[torch.float64][b]), tog.EPS32 * sum(abs(v) for v in ref.terms[torch.float64][b].values()))
        print(f"  {case} loss[{b}]: hip {loss[b]:.7g} fp64 {ref.loss[torch.float64][b]:.7g} yard {yard:.3e}")
        assert abs(float(loss[b]) - ref.loss[torch.float64][b]) <= K_BAR * yard
    assert split_blob(g, ref.state)[FSCORE_BIAS].tolist() == [0.0]
    monkeypatch.setattr(tog, "OnlineOracle", ImitationOracle)
    record_as_geometry(monkeypatch)
    worst = check_gradient("imitation_" + case, ref, g, (FSCORE_BIAS,))
    margins.record("imitation_geometry", case, worst_ratio=worst, k_bar=K_BAR, margin=MARGIN,
                   violators=",".join(str(len(v)) for v in ref.violators[torch.float64]))


# ---- C: the row forms at the layer limit ----------------------------------------------------------------------------------------------
ROW_K = 5
ROW_LISTS = [[3], [3, 0, 4], [0, 1, 2, 3, 4]]


@gpu
@pytest.mark.parametrize("rows", ROW_LISTS)
@pytest.mark.parametrize("name", ["fwg_deep8", "fwg_tall"])
def test_online_step_rows_equals_the_compact_batch(name, rows):
    """gnnb_online_step_rows on rows of a K = 5 device batch against gnnb_online_step on the same rows as a batch of their own: loss,
    gradient and post-step parameters bit for bit, status 0, the source tensors unchanged.  At L = 8 k_trows_gather copies 50 of its
    52 tensors and TPrepMulti, TCompactMulti and TScoreMulti are full."""
    from tests.test_gpu_frontier_online import KB, DeviceBatch, bits, reference_step
    assert KB == ROW_K
    batch = batch_of(name, ROW_K)
    kws = middle_kw(batch.masks[torch.tensor(rows)])
    imps = [(0.0, 1.0, 0.25)[i % 3] for i in range(len(rows))]
    for apply in (False, True):
        want_loss, want_g, want_w = reference_step(batch, rows, kws, imps, apply)
        d = DeviceBatch(batch)
        w0 = d.eng.get_weights()
        loss, status = d.step(rows, kws, imps, apply)
        assert status == 0
        np.testing.assert_array_equal(bits(loss), bits(want_loss))
        np.testing.assert_array_equal(bits(d.eng.online_grad()), bits(want_g))
        np.testing.assert_array_equal(bits(d.eng.get_weights()), bits(want_w))
        assert np.isfinite(loss).all() and float(np.abs(want_g).max()) > 0
        assert (bits(d.eng.get_weights()) != bits(w0)).any() == apply
        assert d.unchanged()


@gpu
@pytest.mark.parametrize("rows", ROW_LISTS)
@pytest.mark.parametrize("name", ["fwg_deep8", "fwg_tall"])
def test_imitation_step_rows_equals_the_compact_batch(name, rows):
    """gnnb_imitation_step_rows likewise: loss, report, regret, gradient and post-step parameters bit for bit."""
    from tests.test_online_gradients import bits
    batch = batch_of(name, ROW_K)
    table = seeded_table(batch.masks.numpy(), 16, 3)
    for apply in (False, True):
        loss, report, regret, status, g, w, same = step_rows(new_engine(lr=1e-3), batch, table, rows, apply)
        eng = new_engine(lr=1e-3)
        w0 = eng.get_weights()
        closs, creport, cregret = eng.imitation_step(tgi.take(batch, rows).forward_args(), table[rows], 1.0, apply=apply)
        assert same and status == 0
        assert bits(loss).tolist() == bits(closs).tolist() and report.tolist() == creport.tolist() and regret.tolist() == cregret.tolist()
        assert bits(g).tolist() == bits(eng.online_grad()).tolist() and np.abs(g).max() > 0
        assert bits(w).tolist() == bits(eng.get_weights()).tolist()
        assert (bits(w) != bits(w0)).any() == apply


# ---- D: no state across geometries ----------------------------------------------------------------------------------------------------
def grad_only(name, eng=None):
    batch = batch_of(name)
    return hip_step(state_of("random"), batch.forward_args(), kws_of(name), imps_for(batch.batch_size), eng=eng)


@gpu
def test_no_state_across_geometries():
    """One engine rebound fwg_deep8 -> fwg_tiny -> fwg_rect -> fwg_deep8 with a gradient-only step on each: every gradient is bit-equal to
    a fresh engine's, so the arena, the descriptor slots (24 of 64 taken at L = 8) and the edge_w copies carry nothing across a rebind."""
    from tests.test_online_gradients import bits
    order = ["fwg_deep8", "fwg_tiny", "fwg_rect", "fwg_deep8"]
    fresh = {name: grad_only(name) for name in set(order)}
    eng, got = None, []
    for name in order:
        eng, loss, scores, g = grad_only(name, eng)
        got.append(g)
        np.testing.assert_array_equal(bits(g), bits(fresh[name][3]), err_msg=name)
        np.testing.assert_array_equal(bits(loss), bits(fresh[name][1]), err_msg=name)
        np.testing.assert_array_equal(bits(scores.cpu().numpy()), bits(fresh[name][2].cpu().numpy()), err_msg=name)
    np.testing.assert_array_equal(bits(got[0]), bits(got[3]))
    assert float(np.abs(got[0]).max()) > 0


# ---- E: the limits --------------------------------------------------------------------------------------------------------------------
def refused_call(eng, batch, who):
    """The entry point `who` on the batch, gradient only (the two row forms on rows [1, 0]).  Marshalling binds the batch's network."""
    from gnn_branching_amd.engine import make_batch
    if who == "gnnb_online_step":
        return eng.online_step(batch.forward_args(), middle_kw(batch.masks), imps_for(batch.batch_size), apply=False)
    dev, B = eng.device, batch.batch_size
    m = eng._marshal(*batch.forward_args())
    cb, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
    rows = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    if who == "gnnb_online_step_rows":
        kw = torch.tensor(middle_kw(batch.masks[[1, 0]]), dtype=torch.int32, device=dev)
        return eng.online_step_rows(cb, B, rows, kw, torch.tensor([0.1, 0.2], dtype=torch.float32, device=dev), apply=False)
    assert who == "gnnb_imitation_step_rows"
    return eng.imitation_step_rows(cb, B, rows, torch.from_numpy(seeded_table(batch.masks.numpy(), 16, 1)).to(dev), 1.0, apply=False)


STEP_FORMS = ["gnnb_online_step", "gnnb_online_step_rows", "gnnb_imitation_step_rows"]


def still_works(eng):
    """After a refusal the same engine takes an fwg_mlp step whose gradient, loss and scores are a fresh engine's, bit for bit."""
    from tests.test_online_gradients import bits
    _, loss, scores, g = grad_only("fwg_mlp", eng)
    _, loss0, scores0, g0 = grad_only("fwg_mlp")
    np.testing.assert_array_equal(bits(g), bits(g0))
    np.testing.assert_array_equal(bits(loss), bits(loss0))
    np.testing.assert_array_equal(bits(scores.cpu().numpy()), bits(scores0.cpu().numpy()))
    assert float(np.abs(g0).max()) > 0


@gpu
@pytest.mark.parametrize("name,edge,taps", [("onl_clamp640", "5x5 stride 1, 32 -> 32 channels", 640), ("fwg_valu", "5x5 stride 1, 16 -> 32 channels", 800)])
def test_conv_past_the_clamped_tap_limit_is_refused(name, edge, taps):
    """GNNB_E_INVALID (-1) from every form of the step, naming the edge and the taps a node really lists (test_tap_limit_arithmetic), before
    anything is launched (a step begins by zeroing the gradient: the last step's is still there); the forward scorer takes the same
    network; the handle goes on working."""
    from tests.test_online_gradients import bits
    batch = batch_of(name)
    eng, _, _, g_before = grad_only("fwg_mlp")
    with torch.no_grad():
        res = eng.forward(*batch.forward_args()).check()
    assert int(res.status.cpu()[0]) == 0 and bool(torch.isfinite(res.scores.cpu()[batch.masks != 0]).all())
    text = rf" failed \(-1\).*the convolution into ReLU layer 2 \({edge}\) gives a node up to {taps} taps, the training kernels hold 512"
    for who in STEP_FORMS:
        with pytest.raises(RuntimeError, match=who + text):
            refused_call(eng, batch, who)
        np.testing.assert_array_equal(bits(eng.online_grad()), bits(g_before))
    still_works(eng)


@gpu
def test_zero_tap_network_is_refused_by_every_form_of_the_step():
    """fwg_zerotap (inner 2x2 stride 3: pixels of layer 1 no window reads) through gnnb_online_step, gnnb_online_step_rows and
    gnnb_imitation_step_rows: refuse_zero_taps' text from each, and after each the engine steps fwg_mlp as a fresh one does."""
    batch = batch_of(ZERO_TAP_ARCH[0])
    eng = new_engine()
    text = r" failed \(-1\).*the convolution into ReLU layer 2 \(2x2 stride 3 pad 1 on 9x6\) reads no tap of pixel \(1, 1\) of layer 1"
    for who in STEP_FORMS:
        with pytest.raises(RuntimeError, match=who + text):
            refused_call(eng, batch, who)
        still_works(eng)
