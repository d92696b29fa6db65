"""The forward scorer (gnnb_forward) on input shapes and conv geometries other than 3x32x32: the networks of tests/common.py FWD_ARCHS
(non-square inputs, 5x5 / 7x7 / 1x1 / 2x2 kernels, stride > kernel on the first edge, windows larger than the image, conv edges without
MFMA gather tables in one or both directions, L = 1 and L = 8) against the oracle in float64.

Bars: scores score_tol("random", want64) = max(5e-6, 1e-5 x score range); embeddings 2e-5 x max(1, max|rows|) (tests/test_gpu_parity.py).
Every comparison records its worst error, the bar and the ratio of the error to the fp32 oracle's own error against float64
(tests/margins.py section "forward_geometry"; profiles/forward_geometry_margins.json is a copy of one run on the MI355X).

The tests without the `gpu` mark run on the CPU: they show that the batches are well-posed (every node class in every ReLU layer, a decision
gap of more than 4 bars, the fp32 oracle inside the bar) and that the bar sees the smallest indexing error one can make (a zeroed kernel
column, two samples' property layers exchanged: more than 10 bars).  When a score test fails, read test_embeddings_after_every_halfpass
first: it names the half-pass and the graph layer."""
import copy
from functools import lru_cache

import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import nets, synth
from tests import margins
from tests.common import FWD_ARCHS, SCORE_ATOL, STAGES, ZERO_TAP_ARCH, random_state, register_fwd_archs, score_tol, shipped_state

gpu = pytest.mark.gpu
NAMES = list(FWD_ARCHS)
PROPS = [(3, 5), (1, 7), (0, 2), (4, 3), (9, 0)]
# (seed, eps) of every network's batch: chosen so that test_batches_are_well_posed holds
BATCH = {"fwg_rect": (5, 0.005), "fwg_gap": (5, 0.02), "fwg_tall": (5, 0.002), "fwg_tiny": (6, 0.02), "fwg_k7": (5, 0.003),
         "fwg_valu": (5, 0.003), "fwg_deep8": (377, 0.0001), "fwg_mlp": (5, 0.02), "fwg_single": (5, 0.02)}
# index (in the layer list) of the convolution whose last kernel column test_the_bar_sees_a_shape_bug zeroes
MUTATED_CONV = {"fwg_rect": 2, "fwg_gap": 2, "fwg_tall": 4, "fwg_tiny": 0, "fwg_k7": 2, "fwg_valu": 2, "fwg_deep8": None, "fwg_mlp": None,
                "fwg_single": 0}
BIT_IDENTICAL = ("top_split=1", "top_fuse_upd=0", "tail_max_b=0", "clspre_max_b=0")
# (arch, setting) -> text of the GNNB_E_INVALID bind refuses it with.  None: every channel count of FWD_ARCHS is one the VALU conv
# kernels are compiled for, so "gather=0" binds everywhere.
BIND_REFUSALS = {}


@pytest.fixture(scope="module", autouse=True)
def _register():
    register_fwd_archs()


def shape_of(name):
    return ZERO_TAP_ARCH[1] if name == ZERO_TAP_ARCH[0] else FWD_ARCHS[name][0]


@lru_cache(None)
def batch_of(name, B=3):
    register_fwd_archs()
    seed, eps = BATCH.get(name, (5, 0.02))
    return synth.make_batch(name, B, seed=seed, eps=eps, props=PROPS[:B], input_shape=shape_of(name))


def relu_sizes(batch):
    return [int(np.prod(t.shape[1:])) for t in batch.lower_bounds_all[1:-1]]


def run_oracle(state, batch, dtype, layers=None, stages=None):
    """(B, R) padded scores (numpy) of the oracle on the batch, optionally with another `layers` argument."""
    from oracle import gnn_oracle
    args = list(batch.forward_args())
    if layers is not None:
        args[5] = layers
    with torch.no_grad():
        ragged = gnn_oracle.oracle_forward(state, *args, dtype=dtype, stages=stages)
    return gnn_oracle.padded_scores(ragged, batch.masks).numpy()


@lru_cache(None)
def reference(name, fam="random"):
    """{want64, want32, stages64, stages32, bar, noise}: computed once per network, shared by every test, never written to."""
    batch = batch_of(name)
    state = random_state() if fam == "random" else shipped_state()
    s64, s32 = {}, {}
    want64 = run_oracle(state, batch, torch.float64, stages=s64)
    want32 = run_oracle(state, batch, torch.float32, stages=s32)
    fin = np.isfinite(want64)
    out = {"want64": want64, "want32": want32, "fin": fin, "stages64": s64, "stages32": s32,
           "bar": score_tol(fam, want64[fin]) if fam == "random" else SCORE_ATOL,
           "noise": float(np.abs(want32[fin].astype(np.float64) - want64[fin]).max())}
    for v in (want64, want32):
        v.setflags(write=False)
    return out


def decisions_of(scores, batch):
    from oracle import gnn_oracle
    sizes = relu_sizes(batch)
    return [gnn_oracle.decision_from_scores(torch.from_numpy(scores[b][batch.masks[b].numpy() != 0]), batch.masks[b], sizes)
            for b in range(batch.batch_size)]


def conv_edges(name, archs=FWD_ARCHS):
    """[(layer index, c_in, c_out, k, stride, pad, h_in, w_in)] of the network's convolutions (archs: name -> (input shape, spec))."""
    shape, spec = (ZERO_TAP_ARCH[1], ZERO_TAP_ARCH[2]) if name == ZERO_TAP_ARCH[0] else archs[name]
    out, (_, h, w) = [], shape
    for i, s in enumerate(spec):
        if s[0] == "conv":
            _, ci, co, k, st, pad = s
            out.append((i, ci, co, k, st, pad, h, w))
            h, w = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    return out


# ---- CPU: the batches are well-posed, the bar sees a shape bug ---------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_batches_are_well_posed(name):
    """A condition on the inputs, not a measurement: every ReLU layer of the batch has an ambiguous, a passing and a blocked node, every
    sample at least two ambiguous nodes; the float64 oracle's two best scores of every sample lie more than 4 bars apart (so the
    decision is the oracle's outright); and the fp32 oracle itself meets the bar."""
    batch, ref = batch_of(name), reference(name)
    for r, m in enumerate(batch.bab_masks):
        assert bool((m == -1).any()) and bool((m == 1).any()) and bool((m == 0).any()), (name, r)
    assert int(batch.n_ambiguous().min()) >= 2
    assert np.array_equal(ref["fin"], batch.masks.numpy() != 0)
    gaps = []
    for b in range(batch.batch_size):
        s = np.sort(ref["want64"][b][ref["fin"][b]])
        gaps.append(float(s[-1] - s[-2]))
    print(f"{name}: {int(ref['fin'].sum())} scores in [{ref['want64'][ref['fin']].min():.3g}, {ref['want64'][ref['fin']].max():.3g}], bar {ref['bar']:.1e}, "
          f"fp32 oracle error {ref['noise']:.2e}, smallest decision gap {min(gaps):.2e}")
    assert min(gaps) > 4 * ref["bar"], gaps
    assert ref["noise"] <= ref["bar"]


def _mutations(name, batch, every=False, conv=None, archs=FWD_ARCHS):
    """(what, layers) with one smallest indexing error each: the last kernel column of one convolution zeroed (MUTATED_CONV names it,
    or `conv`; the two networks without a convolution have no such mutation), and the property layers of samples 0 and 1 exchanged."""
    fixed, props = batch.layers["fixed_layers"], batch.layers["prop_layers"]
    for i, _, _, k, st, pad, _, w in conv_edges(name, archs):
        if every or i == (MUTATED_CONV[name] if conv is None else conv):
            mut = [copy.deepcopy(l) if j == i else l for j, l in enumerate(fixed)]
            with torch.no_grad():
                mut[i].weight[..., -1] = 0
            yield f"conv {k}x{k}/{st}/{pad} at layer {i}: last column zeroed", {"fixed_layers": mut, "prop_layers": props}
    yield "property layers of samples 0 and 1 exchanged", {"fixed_layers": fixed, "prop_layers": [props[1], props[0]] + list(props[2:])}


@pytest.mark.parametrize("name", NAMES)
def test_the_bar_sees_a_shape_bug(name):
    """Bounds and primals unchanged, `layers` mutated: every mutation moves some finite float64 score by more than 10 bars."""
    batch, ref = batch_of(name), reference(name)
    for what, layers in _mutations(name, batch):
        got = run_oracle(random_state(), batch, torch.float64, layers=layers)
        moved = float(np.abs(got[ref["fin"]] - ref["want64"][ref["fin"]]).max())
        print(f"{name}: {what}: a score moves by {moved:.2e} = {moved / ref['bar']:.0f} bars")
        assert moved > 10 * ref["bar"], (what, moved, ref["bar"])


def test_the_oracle_cannot_score_a_zero_tap_network():
    """Inner conv with stride > kernel: the reference divides the transposed aggregate by a tap count of 0 (graph_conv.py:306-312)."""
    with pytest.raises(FloatingPointError):
        run_oracle(random_state(), batch_of(ZERO_TAP_ARCH[0], 2), torch.float64)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def new_engine(options=None, fam="random"):
    from gnn_branching_amd.engine import ScorerEngine
    return ScorerEngine(random_state() if fam == "random" else shipped_state(), options=options)


@pytest.fixture(scope="module")
def engine():
    return new_engine()


def forward(eng, batch):
    with torch.no_grad():
        return eng.forward(*batch.forward_args()).check()


def check_scores(name, test, got, ref, key=None):
    """-inf pattern of the mask, finite scores within the bar of the float64 oracle; the margin goes on record."""
    fin = ref["fin"]
    assert np.array_equal(np.isneginf(got), ~fin), (name, test)
    err = float(np.abs(got[fin].astype(np.float64) - ref["want64"][fin]).max())
    ratio = err / max(ref["noise"], 1e-30)
    print(f"{name} {test}: max|score - oracle64| = {err:.3e} (bar {ref['bar']:.1e}; {ratio:.2f} x the fp32 oracle's {ref['noise']:.2e})")
    margins.record("forward_geometry", key or f"{name}_{test}", worst_err=err, bar=float(ref["bar"]), max_ratio=ratio)
    assert err <= ref["bar"], (name, test, err, ref["bar"])


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_scores_and_decisions(name, engine):
    batch, ref = batch_of(name), reference(name)
    res = forward(engine, batch)
    assert int(res.status.cpu()[0]) == 0
    got = res.scores.cpu().numpy()
    check_scores(name, "scores", got, ref)
    assert res.decisions.cpu().tolist() == decisions_of(ref["want64"], batch)
    engine.workspace(batch.batch_size).view(torch.float32).fill_(float("nan"))       # nothing may read what the call did not write
    again = forward(engine, batch)
    assert np.array_equal(again.scores.cpu().numpy(), got) and torch.equal(again.decisions, res.decisions)


@gpu
@pytest.mark.parametrize("name", ["fwg_rect", "fwg_tall"])
def test_shipped_checkpoint_scores(name):
    batch, ref = batch_of(name), reference(name, "shipped")
    res = forward(new_engine(fam="shipped"), batch)
    check_scores(name, "shipped", res.scores.cpu().numpy(), ref)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_embeddings_after_every_halfpass(name, engine):
    """mu of EVERY node of every graph layer after r0_fwd, r0_bwd, r1_fwd, r1_bwd."""
    batch, ref = batch_of(name), reference(name)
    B = batch.batch_size
    failures = []
    try:
        for n, st in enumerate(STAGES, 1):
            engine.set_halfpass_limit(n)
            forward(engine, batch)
            for k in range(len(batch.lower_bounds_all)):
                want, want32 = ref["stages64"][st][k].numpy(), ref["stages32"][st][k].numpy()
                got = engine.mu(B, k).numpy().astype(np.float64)
                bar = 2e-5 * max(1.0, float(np.abs(want).max()))
                err = float(np.abs(got - want).max())
                noise = float(np.abs(want32 - want).max())
                margins.record("forward_geometry", f"{name}_mu_{st}_layer{k}", worst_err=err, bar=bar, max_ratio=err / max(noise, 1e-30))
                if not err <= bar:
                    node = np.unravel_index(int(np.nanargmax(np.abs(got - want).max(-1))), got.shape[:2])
                    failures.append((st, k, err, bar, f"sample {node[0]} node {node[1]}"))
    finally:
        engine.set_halfpass_limit(0)
    for f in failures:
        print(f"{name}: after {f[0]} graph layer {f[1]}: max|mu - oracle64| = {f[2]:.3e} (bar {f[3]:.1e}) at {f[4]}")
    assert not failures, failures[0]


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_option_path(name, engine):
    from tests.test_gpu_launch_plan import SETTINGS
    batch, ref = batch_of(name), reference(name)
    default = forward(engine, batch).scores.cpu().numpy()
    for setting, opts in SETTINGS.items():
        if setting == "default":
            continue
        eng = new_engine(opts)                                                       # ("gather" and "dense_lds" shape the bind)
        if (name, setting) in BIND_REFUSALS:
            with pytest.raises(RuntimeError, match=r"gnnb_bind_network failed \(-1\).*" + BIND_REFUSALS[(name, setting)]):
                forward(eng, batch)
            continue
        got = forward(eng, batch).scores.cpu().numpy()
        check_scores(name, setting, got, ref, key=f"{name}_options")
        if setting in BIT_IDENTICAL:
            assert np.array_equal(got, default), (name, setting)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_rows_of_a_batch_equal_their_own_runs(name, engine):
    batch = batch_of(name, 5)
    full = forward(engine, batch)
    for b in range(5):
        one = forward(engine, batch.slice(b, b + 1))
        assert torch.equal(one.scores[0], full.scores[b]), (name, b)
        assert torch.equal(one.decisions[0], full.decisions[b]), (name, b)


def transposed(name, batch):
    """The batch with H and W exchanged: every conv weight, the input, the bounds, duals, primals and masks transposed in their last two
    axes, the first Linear's columns permuted to match.  Returns (batch, index): score [b, j] of the new batch is score [b, index[j]]
    of the old one."""
    fixed = batch.layers["fixed_layers"]
    B = batch.batch_size
    shapes, _ = nets.graph_layout(fixed + [batch.layers["prop_layers"][0]], shape_of(name))

    def perm(sh):
        n = int(np.prod(sh))
        return torch.arange(n).reshape(sh).transpose(-1, -2).reshape(-1) if len(sh) == 3 else torch.arange(n)

    def tr(t, sh):                                   # a (B, *sh) tensor or its flat (B * n) form
        if len(sh) != 3:
            return t
        v = t.reshape((B,) + tuple(sh)).transpose(-1, -2).contiguous()
        return v.reshape(-1) if t.dim() == 1 else v
    new_fixed, cur, prim_shapes = [], tuple(shape_of(name)), []
    for l in fixed:
        l2 = copy.deepcopy(l)
        with torch.no_grad():
            if isinstance(l, nn.Conv2d):
                l2.weight.copy_(l.weight.transpose(-1, -2))
                cur = tuple(l(torch.zeros((1,) + cur)).shape[1:])
            elif isinstance(l, nn.Linear):
                if len(cur) == 3:
                    l2.weight.copy_(l.weight[:, perm(cur)])
                cur = (l.out_features,)
        new_fixed.append(l2)
        prim_shapes.append(cur)                      # (a flattened activation keeps its 3-D meaning until the Linear)
    assert len(shapes[-2]) == 1, "the property layer would need its columns permuted too"
    lbs = [tr(t, sh) for t, sh in zip(batch.lower_bounds_all, shapes)]
    ubs = [tr(t, sh) for t, sh in zip(batch.upper_bounds_all, shapes)]
    duals = [d.reshape(B, -1, 3)[:, perm(sh)].reshape(d.shape).contiguous() for d, sh in zip(batch.dual_vars, shapes[1:-1])]
    prims = [tr(p, sh) for p, sh in zip(batch.primals[:-1], prim_shapes)] + [batch.primals[-1]]
    index = torch.cat([perm(sh) + off for sh, off in zip(shapes[1:-1], np.cumsum([0] + relu_sizes(batch))[:-1])])
    out = synth.SubproblemBatch(lbs, ubs, duals, prims, tr(batch.primal_inputs, shapes[0]),
                                {"fixed_layers": new_fixed, "prop_layers": batch.layers["prop_layers"]}, batch.masks[:, index].contiguous(),
                                [m[:, perm(sh)] for m, sh in zip(batch.bab_masks, shapes[1:-1])])
    return out, index


@pytest.mark.parametrize("name", ["fwg_rect", "fwg_tall"])
def test_the_oracle_agrees_with_itself_transposed(name):
    """The construction of the exchanged batch is right: in float64 it scores as the original does, up to summation order."""
    batch, ref = batch_of(name), reference(name)
    tb, index = transposed(name, batch)
    got = np.full_like(ref["want64"], -np.inf)
    got[:, index.numpy()] = run_oracle(random_state(), tb, torch.float64)
    assert np.array_equal(np.isfinite(got), ref["fin"])
    assert float(np.abs(got[ref["fin"]] - ref["want64"][ref["fin"]]).max()) <= 1e-12


@gpu
@pytest.mark.parametrize("name", ["fwg_rect", "fwg_tall"])
def test_height_and_width_exchanged(name, engine):
    """A kernel that exchanges H and W consistently is right on one orientation only: both must meet the bar."""
    batch, ref = batch_of(name), reference(name)
    tb, index = transposed(name, batch)
    a = forward(engine, batch).scores.cpu().numpy()
    t = forward(engine, tb).scores.cpu().numpy()
    b = np.full_like(a, np.nan)
    b[:, index.numpy()] = t
    check_scores(name, "hw_original", a, ref)
    check_scores(name, "hw_exchanged", b, ref)
    diff = float(np.abs(a[ref["fin"]].astype(np.float64) - b[ref["fin"]]).max())
    margins.record("forward_geometry", f"{name}_hw_difference", worst_err=diff, bar=float(2 * ref["bar"]), max_ratio=diff / max(ref["noise"], 1e-30))
    print(f"{name}: max|scores - scores of the exchanged network| = {diff:.3e}")


@gpu
def test_zero_tap_network_is_refused_by_the_scoring_entry_points():
    """Inner conv 2x2 stride 3: pixels of layer 1 that no window reads.  gnnb_forward, gnnb_forward_host and gnnb_online_step return
    GNNB_E_INVALID (-1) before any launch and name the layer; bind, gnnb_kw_bounds and gnnb_babsr take the network (they divide by no
    tap count); the handle goes on working."""
    from tests.test_gpu_kw_geometry import Net, compare, device_row, run_device, seeded_domain
    name = ZERO_TAP_ARCH[0]
    zb, ok = batch_of(name, 2), batch_of("fwg_single")
    eng = new_engine()
    eng.online_create()
    before = forward(eng, ok).scores.cpu().numpy()
    text = r" failed \(-1\).*the convolution into ReLU layer 2 \(2x2 stride 3 pad 1 on 9x6\) reads no tap of pixel \(1, 1\) of layer 1"
    with pytest.raises(RuntimeError, match="gnnb_forward" + text):
        eng.forward(*zb.forward_args())
    with pytest.raises(RuntimeError, match="gnnb_forward_host" + text):
        eng.forward_host(*zb.forward_args())
    kw = [int(torch.nonzero(zb.masks[b])[0]) for b in range(2)]
    with pytest.raises(RuntimeError, match="gnnb_online_step" + text):
        eng.online_step(zb.forward_args(), kw, [0.1, 0.2], apply=False)
    # accepted: bind (by every call above), BaBSR, Wong-Kolter bounds (against the host, per domain)
    res = eng.babsr(zb.lower_bounds_all, zb.upper_bounds_all, zb.layers, zb.masks)
    torch.cuda.synchronize()
    sc = res.scores.cpu()
    assert sc.shape == zb.masks.shape and bool(torch.isfinite(sc).all()) and bool((sc[zb.masks == 0] == 0).all()) and bool((sc != 0).any())
    net = Net(name)
    net.shape = ZERO_TAP_ARCH[1]
    doms = [seeded_domain(net, i) for i in range(2)]
    kwres = run_device(eng, doms)
    for b, d in enumerate(doms):
        compare(d.lp, device_row(kwres, b), d.host(), (name, b))
    # the handle stays usable: the same bits as before the refusals
    assert np.array_equal(forward(eng, ok).scores.cpu().numpy(), before)
    loss, _ = eng.online_step(ok.forward_args(), [int(torch.nonzero(ok.masks[b])[0]) for b in range(3)], [0.1, 0.2, 0.3], apply=False)
    assert np.isfinite(loss).all()
