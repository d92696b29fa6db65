"""The BaBSR fallback scorer on the MI355X (k_babsr via ScorerEngine.babsr / BabsrScorer) against oracle/babsr_oracle.py in fp64 on every
geometry of tests/common.py KW_ARCHS and ARCHS, degenerate bounds (0/0 slopes, NaN reaching the layer below, subnormal and huge widths),
the LDS limit of its ratio buffers and large batches.

Bar per layer (the rule of the dual <= 30 stress): |HIP - oracle64| <= FACTOR max|oracle32 - oracle64|, at least 4 ulp of
the layer's largest |value|; worst error, bar and their ratio are recorded under margins "babsr_geometry".  FACTOR is 3, not 2: k_babsr sums
W^T ratio with one sequential fmaf chain per node (up to 200 terms on toy_widehead's Linear edge, three edges deep on cifar_deep_kw), while the
fp32 oracle's matmul / conv_transpose2d add in blocks; measured 2.2 x the oracle's own fp32 error on those two, at most 1.2 x elsewhere."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import synth
from gnn_branching_amd.plnn import kw_score_conv as kw
from oracle import babsr_oracle
from tests import margins
from tests.common import ARCHS, KW_ARCHS, register_kw_archs, register_toy_archs
from tests.test_babsr import babsr_golden
from tests.test_gpu_kw_geometry import Net, force_nodes, graph_index, run_device, seeded_domain

pytestmark = pytest.mark.gpu

FACTOR = 3.0
# (sparsest_layer, icp_score_counter, decision_threshold): the SETTINGS rows of oracle/make_golden_babsr.py, as its golden files hold them
SETTINGS = [(int(sp), int(cnt), float(thr)) for sp, cnt, thr in babsr_golden("cifar_base_kw_B3")["settings"]]


@pytest.fixture(scope="module")
def engine():
    from gnn_branching_amd.engine import ScorerEngine
    register_kw_archs()
    register_toy_archs()
    return ScorerEngine(None)


class Inputs:
    """A BaBSR batch: graph-layer bounds (B, ...) fp32 with the input first and the property node last, per-ReLU-layer BaB masks
    (B, N_k) in {-1, 0, 1}, and the layers dict of GraphNet.forward."""

    def __init__(self, lbs, ubs, bab, fixed, props):
        self.lbs, self.ubs, self.bab = lbs, ubs, bab
        self.layers = {"fixed_layers": fixed, "prop_layers": props}

    @property
    def B(self):
        return int(self.lbs[0].shape[0])

    def relu_shapes(self):
        shapes = []
        x = torch.zeros((1,) + tuple(self.lbs[0].shape[1:]))
        with torch.no_grad():
            for l in self.layers["fixed_layers"]:
                if type(l) is nn.ReLU:
                    shapes.append(tuple(x.shape[1:]))
                x = l(x)
        return shapes

    def undecided(self):
        return [(m == -1).double() for m in self.bab]

    def rows(self, idx):
        sl = lambda ts: [t[idx] for t in ts]       # noqa: E731
        return Inputs(sl(self.lbs), sl(self.ubs), sl(self.bab), self.layers["fixed_layers"], [self.layers["prop_layers"][i] for i in idx])


def oracle(inp, dtype):
    """babsr_oracle.babsr_scores in `dtype` -> (scores, intercepts), per ReLU layer (B, N_k)."""
    shapes = inp.relu_shapes()
    fixed = [copy.deepcopy(l).to(dtype) for l in inp.layers["fixed_layers"]]
    lbs = [t.reshape((inp.B,) + s).to(dtype) for t, s in zip(inp.lbs[1:-1], shapes)]
    ubs = [t.reshape((inp.B,) + s).to(dtype) for t, s in zip(inp.ubs[1:-1], shapes)]
    prop_w = torch.stack([p.weight[0] for p in inp.layers["prop_layers"]]).detach().to(dtype)
    masks = [m.to(dtype) for m in inp.undecided()]
    with torch.no_grad():
        return babsr_oracle.babsr_scores(lbs, ubs, masks, fixed, prop_w)


def run_hip(engine, inp, matrix=False):
    scorer = kw.BabsrScorer(engine)
    if matrix:
        mask = torch.cat([(m == -1).float() for m in inp.bab], 1)
        return scorer.scores(inp.lbs, inp.ubs, inp.layers, mask)
    return scorer.scores(inp.lbs, inp.ubs, inp.layers, inp.bab)


def layer_bars(o32, o64, select=None):
    """Per-layer bar: 2 max|o32 - o64| over the finite entries (`select`: a bool mask of the entries that count), at least 4 ulp of the
    largest |o64|."""
    bars = []
    for a, b, s in zip(o32, o64, select or [None] * len(o32)):
        fin = torch.isfinite(a.double()) & torch.isfinite(b)
        if s is not None:
            fin &= s
        if not bool(fin.any()):
            bars.append(0.0)
            continue
        diff = float((a.double() - b).abs()[fin].max())
        big = float(b.abs()[fin].max())
        bars.append(max(FACTOR * diff, 4 * float(np.spacing(np.float32(big)))))
    return bars


def check_within(got, o32, o64, key, select=None):
    """|got - o64| <= bar per layer on the finite entries (where `select`); records (worst error, bar, ratio).  Returns the bars."""
    bars = layer_bars(o32, o64, select)
    worst = 0.0
    for k, (g, b, bar) in enumerate(zip(got, o64, bars)):
        fin = torch.isfinite(b)
        if select is not None:
            fin &= select[k]
        err = float((g.double() - b).abs()[fin].max()) if bool(fin.any()) else 0.0
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        margins.record("babsr_geometry", f"{key}/layer{k + 1}", worst_err=err, bar=bar, max_ratio=ratio, factor=FACTOR)
        assert err <= bar, (key, k, err, bar)
    return bars


def split_rows(res, B):
    sizes = res.relu_sizes
    return ([t for t in torch.split(res.scores.cpu(), sizes, 1)], [t for t in torch.split(res.intercepts.cpu(), sizes, 1)])


def decision_margins(score, icp, sbar, ibar, thr):
    """Smallest deciding gap of one row relative to 4x its bar: the top two candidates, the top score against the threshold, the
    intercepts against -1e-4 and the two smallest intercepts of each layer the intercept branch may take.  True where a gap is too
    small for fp32 to decide."""
    flat = torch.cat([s for s in score])
    top2 = torch.topk(flat, 2).values if flat.numel() > 1 else torch.cat([flat, flat])
    eps_s = 4 * max(sbar)
    if float(top2[0] - top2[1]) <= eps_s or abs(float(top2[0]) - thr) <= eps_s:
        return True
    for t, b in zip(icp, ibar):
        lo2 = torch.topk(t, min(2, t.numel()), largest=False).values
        if abs(float(lo2[0]) + 1e-4) <= 4 * b:
            return True
        if float(lo2[0]) < -1e-4 and lo2.numel() > 1 and float(lo2[1] - lo2[0]) <= 4 * b:
            return True
    return False


def compare_decisions(engine, inp, res, o64, sbars, ibars, key, allow_skip=True):
    """BabsrScorer.decide_many on the device result against babsr_oracle.decide on the fp64 scores, under every SETTINGS row."""
    scorer = kw.BabsrScorer(engine)
    L = len(inp.bab)
    s64, i64 = o64
    masks = inp.undecided()
    skipped = 0
    for sp, cnt, thr in SETTINGS:
        dec, counters = scorer.decide_many(res, [cnt] * inp.B, list(range(L)), sp, thr)
        for b in range(inp.B):
            score, icp = [s[b] for s in s64], [t[b] for t in i64]
            if allow_skip and decision_margins(score, icp, sbars, ibars, thr):
                skipped += 1
                continue
            want, c = babsr_oracle.decide(score, icp, [m[b] for m in masks], cnt, list(range(L)), sp, thr)
            assert dec[b] == want and counters[b] == c, (key, (sp, cnt, thr), b, dec[b], want)
    n = len(SETTINGS) * inp.B
    margins.record("babsr_geometry", f"{key}/decisions", n_rows=n, n_skipped=skipped)
    assert skipped <= 0.1 * n, (key, skipped, n)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def kw_inputs(engine, name, B=64, n_domains=8):
    """Bounds of seeded domains (roots, and domains with forced nodes) on the device's Wong-Kolter bounds (which
    tests/test_gpu_kw_geometry.py holds to the host), replicated to B rows that differ in property and in which nodes are decided."""
    net = Net(name)
    rng = np.random.RandomState(3)
    doms = [seeded_domain(net, i, seed0=61) for i in range(n_domains)]
    for d in doms[n_domains // 2:]:
        force_nodes(d, rng, 3)
    res = run_device(engine, doms, want_fp32=True)
    rows = [b % n_domains for b in range(B)]
    lbs = [t.cpu()[rows] for t in res.lb32]
    ubs = [t.cpu()[rows] for t in res.ub32]
    bab = []
    for r in range(len(doms[0].mask)):
        mk = torch.stack([doms[i].mask[r] for i in rows])
        mk[torch.from_numpy(rng.uniform(size=mk.shape) < 0.05)] = 1            # more decided nodes, different in every row
        bab.append(mk)
    props = [net.prop(b % 10, (b % 10 + 1 + b // 10) % 10) for b in range(B)]        # (B <= 90: gt != cls)
    return Inputs(lbs, ubs, bab, net.fixed, props)


def synth_inputs(name, B=64, seed=5):
    props = [(b % 10, (b + 1 + b // 10) % 10) for b in range(B)]
    props = [(g, c if c != g else (g + 2) % 10) for g, c in props]
    batch = synth.make_batch(name, B, seed=seed, eps=0.03, props=props)
    return Inputs(list(batch.lower_bounds_all), list(batch.upper_bounds_all), list(batch.bab_masks), batch.layers["fixed_layers"],
                  batch.layers["prop_layers"])


def check_config(engine, inp, key, decisions=True):
    res = run_hip(engine, inp)
    res_m = run_hip(engine, inp, matrix=True)
    for a, b in ((res.scores, res_m.scores), (res.intercepts, res_m.intercepts)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    o64, o32 = oracle(inp, torch.float64), oracle(inp, torch.float32)
    got_s, got_i = split_rows(res, inp.B)
    # a forced-passing node that the bounds prove blocked (lb = 0 > ub) has the slope 0/0: NaN exactly where the fp32 reference has it
    for g, w in zip(got_s + got_i, o32[0] + o32[1]):
        assert torch.equal(torch.isnan(g), torch.isnan(w)), key
    sbars = check_within(got_s, o32[0], o64[0], key + "/score")
    ibars = check_within(got_i, o32[1], o64[1], key + "/intercept")
    if decisions:
        compare_decisions(engine, inp, res, o64, sbars, ibars, key)
    return res


KW_GEOMETRIES = list(KW_ARCHS)
TOY_FITS = [n for n in ARCHS if n != "toy_longk"]          # toy_longk: refused (test_wide_layer_is_refused_before_launch)


@pytest.mark.parametrize("name", KW_GEOMETRIES)
def test_kw_geometries_match_the_oracle(name, engine):
    if name == "kwg_over":                                 # gnnb_kw_bounds refuses it: bounds from the host
        inp = host_inputs(name)
    else:
        inp = kw_inputs(engine, name)
    check_config(engine, inp, name)


def host_inputs(name, B=64, n_domains=4):
    net = Net(name)
    rng = np.random.RandomState(4)
    doms = [seeded_domain(net, i, seed0=71) for i in range(n_domains)]
    for d in doms[n_domains // 2:]:
        force_nodes(d, rng, 3)
    hb = [d.host() for d in doms]
    rows = [b % n_domains for b in range(B)]
    gidx = [0] + graph_index(doms[0].lp)
    lbs = [torch.stack([hb[r][0][i].reshape(-1) for r in rows]).float() for i in gidx]
    ubs = [torch.stack([hb[r][1][i].reshape(-1) for r in rows]).float() for i in gidx]
    lbs[0], ubs[0] = lbs[0].reshape((B,) + net.shape), ubs[0].reshape((B,) + net.shape)
    bab = [torch.stack([doms[r].mask[k] for r in rows]) for k in range(len(doms[0].mask))]
    props = [net.prop(b % 10, (b + 1) % 10) for b in range(B)]
    return Inputs(lbs, ubs, bab, net.fixed, props)


@pytest.mark.parametrize("name", TOY_FITS + ["cifar_base_kw", "cifar_wide_kw", "cifar_deep_kw"])
def test_32x32_geometries_match_the_oracle(name, engine):
    """Includes toy_oddch, whose 12288-node layer needs 96 KiB of LDS (the attribute set at init)."""
    check_config(engine, synth_inputs(name), name)


@pytest.mark.parametrize("B", [1, 67, 1024])
def test_batch_sizes(B, engine):
    inp = synth_inputs("cifar_deep_kw", B=B, seed=9)
    res = run_hip(engine, inp)
    sample = sorted({0, B // 2, B - 1})
    sub = inp.rows(sample)
    o64, o32 = oracle(sub, torch.float64), oracle(sub, torch.float32)
    got_s, got_i = split_rows(res, B)
    check_within([s[sample] for s in got_s], o32[0], o64[0], f"cifar_deep_kw_B{B}/score")
    check_within([t[sample] for t in got_i], o32[1], o64[1], f"cifar_deep_kw_B{B}/intercept")
    for b in sample:
        one = run_hip(engine, inp.rows([b]))
        assert torch.equal(res.scores[b].cpu(), one.scores[0].cpu()) and torch.equal(res.intercepts[b].cpu(), one.intercepts[0].cpu()), b


def test_wide_layer_is_refused_before_launch(engine):
    """toy_longk's 32768-node layer needs 256 KiB for the ratio buffers, more than the 160 KiB limit: GNNB_E_INVALID before any launch,
    naming the layer and the bytes."""
    inp = synth_inputs("toy_longk", B=2)
    with pytest.raises(RuntimeError, match=r"gnnb_babsr failed \(-1\): gnnb_babsr: ReLU layer 1 of 32768 nodes needs 262144 bytes of LDS"):
        run_hip(engine, inp)


# ---- degenerate bounds -------------------------------------------------------------------------------------------------------
SPECIAL = [  # (lb, ub) written into ReLU layer 1
    (0.0, 0.7),             # lb = 0 < ub
    (-0.4, 0.0),            # lb < 0 = ub
    (-0.0, 0.3),            # lb = -0.0
    (-5e-31, 5e-31),        # width 1e-30 around 0
    (-1e-40, 2e-40),        # subnormal width
    (-1e30, 2e30),          # |bounds| near 1e30
]


def degenerate_inputs(engine, name, how):
    """Two rows of the same bounds: all nodes undecided in row 0; in row 1 the rewritten nodes and the NaN's reach are decided.
    how = "dead_filter": one conv output channel of ReLU layer 2 with zero weights and bias (lb = ub = 0 exactly, from the bounds
    kernels); how = "one_node": a single layer-2 node rewritten to lb = ub = 0."""
    base = Net(name).base
    if how == "dead_filter":
        base = copy.deepcopy(base)
        convs = [l for l in base if type(l) is nn.Conv2d]
        with torch.no_grad():
            convs[1].weight[1].zero_()
            convs[1].bias[1] = 0.0
    net = Net(name, layers=base)
    d = seeded_domain(net, 2, seed0=81)
    res = run_device(engine, [d, d], want_fp32=True)
    lbs = [t.cpu().clone() for t in res.lb32]
    ubs = [t.cpu().clone() for t in res.ub32]
    n1 = lbs[1].shape[1]
    if how == "one_node":
        n2 = lbs[2].shape[1]
        lbs[2][:, n2 // 2 + 5] = 0.0
        ubs[2][:, n2 // 2 + 5] = 0.0
    special = torch.tensor([7 + 37 * i for i in range(len(SPECIAL))]) % n1
    for j, (lo, up) in zip(special.tolist(), SPECIAL):
        lbs[1][:, j], ubs[1][:, j] = lo, up
    bab = [torch.full_like(t, -1, dtype=torch.long) for t in lbs[1:-1]]
    inp = Inputs(lbs, ubs, bab, net.fixed, [net.prop(3, 5), net.prop(3, 5)])
    # row 1: the rewritten nodes and everything the NaN reaches decided (score and intercept * 0 stay NaN in the reference)
    s64, i64 = oracle(inp, torch.float64)
    for k in range(len(bab)):
        reach = torch.isnan(s64[k][0]) | torch.isnan(i64[k][0])
        if k == 0:
            reach[special] = True
        bab[k][1][reach] = 0
    return inp, special


@pytest.mark.parametrize("name", ["kwg_s1", "cifar_base_kw"])
@pytest.mark.parametrize("how", ["dead_filter", "one_node"])
def test_degenerate_bounds(name, how, engine):
    inp, special = degenerate_inputs(engine, name, how)
    res = run_hip(engine, inp)
    o64, o32 = oracle(inp, torch.float64), oracle(inp, torch.float32)
    got = split_rows(res, inp.B)
    nan_seen = 0
    for which in (0, 1):                                   # scores, intercepts
        for k, (g, w) in enumerate(zip(got[which], o32[which])):
            assert torch.equal(torch.isnan(g), torch.isnan(w)), (name, how, which, k, torch.nonzero(torch.isnan(g) != torch.isnan(w))[:8])
            assert torch.equal(torch.isinf(g), torch.isinf(w)), (name, how, which, k)
            nan_seen += int(torch.isnan(w).sum())
        # finite values: the layer rule on the ordinary nodes, the same rule node by node on the rewritten ones
        sel = [torch.ones_like(t, dtype=torch.bool) for t in o64[which]]
        sel[0][:, special] = False
        check_within(got[which], o32[which], o64[which], f"degenerate_{name}_{how}/{'score' if which == 0 else 'intercept'}", sel)
        for j in special.tolist():
            g, a, b = got[which][0][:, j].double(), o32[which][0][:, j].double(), o64[which][0][:, j]
            fin = torch.isfinite(b)
            bar = torch.maximum(FACTOR * (a - b).abs(), 4 * torch.from_numpy(np.spacing(b.abs().float().numpy())).double())
            assert bool(((g - b).abs() <= bar)[fin].all()), (name, how, which, j, g, b)
    assert nan_seen > 0
    if how == "one_node":                                  # the NaN reaches part of layer 1 only: the rest of it stays finite
        assert bool(torch.isfinite(o32[0][0][0]).any()) and bool(torch.isnan(o32[0][0][0]).any())
    compare_decisions(engine, inp, res, o64, [0.0] * len(o64[0]), [0.0] * len(o64[1]), f"degenerate_{name}_{how}", allow_skip=False)
