"""The learning step (csrc/gnnb_step.h: struct Step on the tape of csrc/gnnb_train.h) computes, bit for bit, what the library computed while
the step was one function, `online_step_device`, under two copies of the descriptor builder and four of the tile dispatch.

Every sum of the step has a fixed order (tests/test_online_gradients.py test_step_is_deterministic; the training kernels hold no atomics), so
a restatement of its host side has nothing to move.  The anchor is tests/golden/learning_step_parent.npz, recorded once on the MI355X with the
library of the commit before the restatement (tools/learning_step_record.py, which imports the cases and the run from this file; the
library's gnnb_build_id() is in the fixture).  The cases, all built by the builders of the step's other tests (and then ``pinned``: the
tensors those builders compute through the network on the CPU are not the same bits on every machine):

  * gnnb_online_step, gradient only, on tests/test_online_geometry.py CASES with their seeds, eps and B: fwg_single (L = 1), fwg_deep8
    (L = 8 = T_MAXL: four chain_multi calls of 8 chains, 32 of the 64 descriptor slots), fwg_mlp (dense edges only), fwg_gap at T = 1 and
    T = 3 (the round loop, the skipped last input update): loss and padded scores raw, the gradient;
  * gnnb_online_step, gradient only, on cifar_wide_kw at B = 1, 2, 9 (layer 1: 4096, 8192, 36864 rows -- 4-, 8- and 32-row tiles on a
    256-CU device): the gradient;
  * gnnb_online_step_rows on rows [3, 0, 4] of K = 5 of fwg_deep8: loss, status, the gradient;
  * gnnb_imitation_step_rows on rows [3, 0, 4] of K = 5 of fwg_tall under seeded_table(M = 16): loss, report, regret, status, the gradient;
  * two applied steps: fwg_gap through gnnb_online_step in repack mode "host", fwg_tall's imitation rows in mode "device" (the step that
    returns without synchronising, its host tables through k_tput): the losses, and the parameters after the second step.

Gradients and parameters are stored as one 64-bit signature per named tensor (tests/test_gpu_net_walk_parent.py `signatures`; the naming
is oracle.online_oracle.split_blob's).  Each case also carries SHA-256 digests of its inputs, and the test asserts those first: a changed
input fails as such and never passes for a changed step."""
import copy
from functools import lru_cache
import os

import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd import synth
from oracle.online_oracle import split_blob
from tests import test_online_geometry as tgeo
from tests.common import GOLDEN, state_of
from tests.test_gpu_imitation import new_engine, seeded_table, step_rows
from tests.test_gpu_net_walk_parent import digest, same_bits, signatures
from tests.test_online_gradients import imps_for, make, middle_kw

gpu = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "learning_step_parent.npz")
ONLINE = [("fwg_single", 2), ("fwg_deep8", 2), ("fwg_mlp", 2), ("fwg_gap", 1), ("fwg_gap", 3)]
WIDE_BS = (1, 2, 9)
ROWS, ROW_K, TABLE_M, TABLE_SEED = [3, 0, 4], 5, 16, 3
ROW_IMPS = [0.0, 1.0, 0.25]
CASES = ([f"online_{n}_T{T}" for n, T in ONLINE] + [f"wide_B{B}" for B in WIDE_BS] +
         ["rows_online_fwg_deep8", "rows_imitation_fwg_tall", "applied_host_fwg_gap", "applied_device_fwg_tall"])
BUILD_ID_KEY = "library/build_id"


def snap(t):
    """fp64 -> fp32 values with a 12-bit mantissa (round to nearest)."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 4096.0) / 4096.0, e).float()


def pinned(batch):
    """The batch with what synth.make_batch computes THROUGH the network -- the bounds of the graph layers behind the input, the primals,
    and the masks that follow from the bounds -- made the same bits on every machine.  make_batch evaluates them in fp32 with torch's CPU
    convolutions, whose sums depend on the thread count and the CPU (measured: other digests at 1, 4 and 8 threads, and on the GPU box),
    and a recorded step can only be compared on identical inputs.  Here the same recipe (synth.make_batch: interval arithmetic with the
    W+ / W- split, primals = activations of x_lp) runs in fp64 from the batch's own input box, x_lp and layers, and every result is
    rounded to a 12-bit mantissa: two machines' fp64 sums differ by ~1e-14 relative, the grid is 2.4e-4, so a value that lands on
    different sides of a rounding boundary is a ~1e-10 event per element.  Signs survive the rounding, so the node classes, hence the
    masks and the KW nodes taken from them, are make_batch's.  What make_batch draws (input box, x_lp, duals, weights) is kept as it is."""
    fixed, props = batch.layers["fixed_layers"], batch.layers["prop_layers"]
    B = batch.batch_size
    with torch.no_grad():
        lb, ub, act = batch.lower_bounds_all[0].double(), batch.upper_bounds_all[0].double(), batch.primal_inputs.double()
        lbs, ubs, primals = [batch.lower_bounds_all[0]], [batch.upper_bounds_all[0]], []
        for l in fixed:
            l64 = copy.deepcopy(l).double()
            if isinstance(l, nn.ReLU):
                lbs.append(snap(lb))
                ubs.append(snap(ub))
            lb, ub = synth._interval(l64, lb, ub)
            act = l64(act)
            primals.append(snap(act.reshape(-1)))
        pw, pb = torch.stack([p.weight[0] for p in props]).double(), torch.stack([p.bias[0] for p in props]).double()
        wp, wn = pw.clamp(min=0), pw.clamp(max=0)
        lbs.append(snap(((lb * wp).sum(1) + (ub * wn).sum(1) + pb).unsqueeze(1)))
        ubs.append(snap(((ub * wp).sum(1) + (lb * wn).sum(1) + pb).unsqueeze(1)))
        primals.append(snap(((act * pw).sum(1) + pb).reshape(-1)))
    bab = []
    for k in range(1, len(lbs) - 1):
        l2, u2 = lbs[k].reshape(B, -1), ubs[k].reshape(B, -1)
        m = torch.zeros(l2.shape, dtype=torch.int64)
        m[(l2 < 0) & (u2 > 0)] = -1
        m[l2 >= 0] = 1
        bab.append(m)
    masks = torch.cat([(m == -1).float() for m in bab], 1)
    assert [tuple(a.shape) for a in lbs] == [tuple(a.shape) for a in batch.lower_bounds_all] and torch.equal(masks, batch.masks)
    assert all(float((a - b).abs().max()) <= 2.0 ** -11 * float(b.abs().max()) for a, b in zip(lbs + ubs + primals, batch.lower_bounds_all + batch.upper_bounds_all + batch.primals))
    return synth.SubproblemBatch(lbs, ubs, batch.dual_vars, primals, batch.primal_inputs, batch.layers, masks, bab)


@lru_cache(None)
def inputs_of(case):
    """The case's inputs: batch (``pinned``), and what its loss reads (kws and imps, or the table)."""
    c = built(case)
    c["batch"] = pinned(c["batch"])
    return c


def built(case):
    """The case by the builders of the step's other tests."""
    if case.startswith("online_") or case == "applied_host_fwg_gap":
        name = case[len("online_"):case.rindex("_T")] if case.startswith("online_") else "fwg_gap"
        batch = tgeo.batch_of(name)
        return {"batch": batch, "kws": tgeo.kws_of(name), "imps": imps_for(batch.batch_size), "T": int(case[-1]) if case.startswith("online_") else 2}
    if case.startswith("wide_"):
        B = int(case[len("wide_B"):])
        batch = make("cifar_wide_kw", B, seed=40 + B)
        return {"batch": batch, "kws": middle_kw(batch.masks), "imps": imps_for(B), "T": 2}
    if case == "rows_online_fwg_deep8":
        batch = tgeo.batch_of("fwg_deep8", ROW_K)
        return {"batch": batch, "kws": middle_kw(batch.masks[torch.tensor(ROWS)]), "imps": ROW_IMPS, "T": 2}
    assert case in ("rows_imitation_fwg_tall", "applied_device_fwg_tall"), case
    batch = tgeo.batch_of("fwg_tall", ROW_K)
    return {"batch": batch, "table": seeded_table(batch.masks.numpy(), TABLE_M, TABLE_SEED), "T": 2}


def input_digests(case):
    """{what: SHA-256} of the case's inputs: the GNN's parameters, the batch (its tensors and the network's and properties' weights), and
    what the loss reads."""
    c = inputs_of(case)
    lbs, ubs, duals, primals, x_lp, layers, masks = c["batch"].forward_args()
    modules = list(layers["fixed_layers"]) + list(layers["prop_layers"])
    out = {"weights": digest(*[torch.as_tensor(np.asarray(v)) for v in state_of("random").values()]),
           "batch": digest(*lbs, *ubs, *duals, *primals, x_lp, masks, *[p for m in modules for p in m.parameters()])}
    if "table" in c:
        out["loss"] = digest(torch.from_numpy(c["table"]), torch.tensor(ROWS))
    else:
        out["loss"] = digest(torch.tensor(c["kws"]), torch.tensor(c["imps"], dtype=torch.float64))
    return out


def tensor_names():
    return list(state_of("random"))


def blob_signatures(blob):
    """(52,) uint64: one signature per named tensor of a parameter or gradient blob, in checkpoint order."""
    parts = split_blob(np.ascontiguousarray(blob, dtype=np.float32), state_of("random"))
    return np.array([signatures(torch.from_numpy(np.ascontiguousarray(a).reshape(1, -1)))[0] for a in parts.values()], dtype=np.uint64)


def run_case(case):
    """{key: array} of one case on the library in use."""
    from gnn_branching_amd.engine import ScorerEngine
    c = inputs_of(case)
    batch = c["batch"]
    if case.startswith("online_") or case.startswith("wide_"):
        eng = ScorerEngine(state_of("random"), T=c["T"])
        eng.online_create()
        loss, scores = eng.online_step(batch.forward_args(), c["kws"], c["imps"], apply=False, want_scores=case.startswith("online_"))
        out = {"grad_sig": blob_signatures(eng.online_grad())}
        if case.startswith("online_"):
            out.update({"loss": np.asarray(loss, np.float32), "scores": scores.cpu().numpy()})
        return out
    if case == "rows_online_fwg_deep8":
        from tests.test_gpu_frontier_online import DeviceBatch
        d = DeviceBatch(batch)
        loss, status = d.step(ROWS, c["kws"], c["imps"], False)
        return {"loss": loss, "status": np.array([status], np.int32), "grad_sig": blob_signatures(d.eng.online_grad())}
    if case == "rows_imitation_fwg_tall":
        loss, report, regret, status, g, _, same = step_rows(new_engine(lr=1e-3), batch, c["table"], ROWS, False)
        assert same
        return {"loss": loss, "report": report, "regret": regret, "status": np.array([status], np.int32), "grad_sig": blob_signatures(g)}
    if case == "applied_host_fwg_gap":
        eng = ScorerEngine(state_of("random"), T=2)
        eng.online_create(lr=1e-2, repack="host")
        losses = [np.asarray(eng.online_step(batch.forward_args(), c["kws"], c["imps"], apply=True)[0], np.float32) for _ in range(2)]
        return {"loss0": losses[0], "loss1": losses[1], "weight_sig": blob_signatures(eng.get_weights())}
    assert case == "applied_device_fwg_tall", case
    eng = new_engine(lr=1e-3)
    eng.set_repack("device")
    steps = [step_rows(eng, batch, c["table"], ROWS, True) for _ in range(2)]
    assert all(s[6] for s in steps)
    return {"loss0": steps[0][0], "loss1": steps[1][0], "report1": steps[1][1], "regret1": steps[1][2],
            "status": np.array([steps[1][3]], np.int32), "weight_sig": blob_signatures(steps[1][5])}


@lru_cache(None)
def recorded():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def assert_inputs(case, why=""):
    want = recorded()
    for what, d in input_digests(case).items():
        assert str(want[f"{case}/inputs/{what}"]) == d, (case, what, why)


@pytest.mark.parametrize("case", CASES)
def test_inputs_are_the_recorded_ones(case):
    """No GPU needed: the digests of what the cases are built from."""
    assert_inputs(case)


def test_the_fixture_names_its_library_and_holds_every_case():
    want = recorded()
    assert len(str(want[BUILD_ID_KEY])) == 32
    assert sorted({k.split("/")[0] for k in want if k != BUILD_ID_KEY}) == sorted(CASES)


@gpu
@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_the_recorded_parent(case):
    if case.startswith("wide_"):
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        if n_cu != 256:
            pytest.skip(f"the tile thresholds are 16 and 128 rows per CU: {n_cu} CUs put them elsewhere than 4096 / 32768 rows")
    assert_inputs(case, "the case's inputs changed: the fixture does not apply")      # first, and a failure: a changed input is no changed step
    want, got = recorded(), run_case(case)
    keys = [k for k in want if k.startswith(case + "/") and "/inputs/" not in k]
    assert sorted(keys) == sorted(f"{case}/{k}" for k in got)
    for k, v in got.items():
        w = want[f"{case}/{k}"]
        if k.endswith("_sig"):
            assert same_bits(v, w), (case, k, [n for n, a, b in zip(tensor_names(), v, w) if a != b])
        else:
            assert same_bits(v, w), (case, k, v, w)
    for k in ("grad_sig", "weight_sig"):      # (what is compared is a step: some gradient, parameters that moved)
        if k in got:
            assert len(set(got[k].tolist())) > 26, (case, k)
