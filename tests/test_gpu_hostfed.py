"""Host-fed batches through the cross-batch double buffer (engine.HostFedPipeline): the copies of batch i + 1 run on a copy stream under
the forward of batch i; results are the bits of the device-resident forward.  (reference: the H2D copies of graph_score.py:26-30.)"""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import make_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("pinned", [False, True])
def test_host_fed_pipeline_is_bit_identical_and_reuses_its_buffers(pinned, compact):
    from gnn_branching_amd import engine as E, synth
    model = make_model("shipped")
    eng = model.engine()
    dev = eng.device
    batches = [synth.make_batch("cifar_base_kw", 24, seed=100 + i) for i in range(5)]      # five different batches through two buffer sets
    want = []
    with torch.no_grad():
        for b in batches:
            args = b.forward_args()
            d = [[t.to(dev) for t in g] if isinstance(g, list) else g for g in args]
            d[4], d[6] = args[4].to(dev), args[6].to(dev)
            r = eng.forward(*d).check()
            want.append((r.scores.cpu().numpy(), r.decisions.cpu().numpy(), [t.cpu().numpy() for t in r.ragged()]))
    pipe = E.HostFedPipeline(eng, compact=compact)       # compact: dual_vars / primals cross the link as records of the ambiguous nodes only
    results = []
    with torch.no_grad():
        for b in batches:
            args = list(b.forward_args())
            if pinned:
                args = [[t.pin_memory() for t in g] if isinstance(g, list) else g for g in args]
                args[4], args[6] = b.forward_args()[4].pin_memory(), b.forward_args()[6].pin_memory()
            results.append(pipe.submit(*args))              # no synchronisation between submissions
    for r, (ws, wd, wr) in zip(results, want):
        r.check()
        assert np.array_equal(r.scores.cpu().numpy(), ws, equal_nan=True)
        assert np.array_equal(r.decisions.cpu().numpy(), wd)
        # results held across more than `depth` submits keep their OWN mask (it used to be a view of the slot's buffer, which the
        # submit two calls later overwrites): the ragged score lists are cut with it
        got = [t.cpu().numpy() for t in r.ragged()]
        assert len(got) == len(wr) and all(np.array_equal(g, w) for g, w in zip(got, wr))


@pytest.mark.parametrize("net,B", [("cifar_base_kw", 40), ("cifar_deep_kw", 9)])
def test_amb_record_image_and_scatter(net, B):
    """gnnb_pack_amb_records / gnnb_scatter_amb_records (include/gnnb.h): the image holds exactly the nodes with lb < 0 < ub of every ReLU
    layer, in index order, with dual[:, 1], dual[:, 2] and the two primals of the node -- and primals[-1]; scattered into poisoned
    full-size arrays, those entries (and only those) carry the batch's values.  LP-like signed duals and decided nodes included."""
    import ctypes as C
    from gnn_branching_amd import _lib, engine as E, synth
    model = make_model("shipped")
    eng = model.engine()
    batch = synth.make_batch(net, B, seed=21)
    rng = np.random.RandomState(3)
    args = list(batch.forward_args())
    args[2] = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)) for t in args[2]]      # duals of either sign
    lbs, ubs, duals, prims, x, layers, mask = args
    eng.bind(layers["fixed_layers"], tuple(lbs[0].shape[1:]))
    nd, npr = len(duals), len(prims)
    host = [[t.float().contiguous() for t in g] for g in (lbs, ubs, duals, prims)]
    hb, keep = E.make_batch(*host, None, None)           # (the packer reads neither x_lp nor the mask nor the property rows)
    cap = int(eng.lib.gnnb_amb_records_bytes(eng.h, B))
    img = torch.zeros(cap // 4, dtype=torch.int32)
    used = C.c_size_t(0)
    _lib.check(eng.lib.gnnb_pack_amb_records(eng.h, C.byref(hb), B, img.data_ptr(), cap, C.byref(used)), "gnnb_pack_amb_records")
    words = img.numpy()
    L = nd
    nrec = int(words[2])
    assert words[1] == L and words[3] == B and used.value == 4 * (16 + 6 * nrec + ((B + 3) & ~3)) <= cap
    rec = words[16:16 + 6 * nrec].reshape(nrec, 6)
    relu_q = [i for i, l in enumerate(layers["fixed_layers"]) if isinstance(l, torch.nn.ReLU)]
    total = 0
    for k in range(L):
        lb, ub = lbs[k + 1].reshape(-1).numpy(), ubs[k + 1].reshape(-1).numpy()
        want = np.flatnonzero((lb < 0) & (ub > 0))
        mine = rec[rec[:, 0] == k]
        mine = mine[np.argsort(mine[:, 1], kind="stable")]        # (the records come in whatever order the packer's threads finished)
        assert np.array_equal(mine[:, 1], want)
        vals = mine[:, 2:].copy().view(np.float32)
        d = duals[k].numpy().reshape(-1, 3)
        assert np.array_equal(vals[:, 0], d[want, 1]) and np.array_equal(vals[:, 1], d[want, 2])
        assert np.array_equal(vals[:, 2], prims[relu_q[k] - 1].numpy()[want]) and np.array_equal(vals[:, 3], prims[relu_q[k]].numpy()[want])
        total += len(want)
    assert total == nrec
    assert np.array_equal(words[16 + 6 * nrec:16 + 6 * nrec + B].view(np.float32), prims[-1].numpy())
    # ---- scatter into NaN-poisoned arrays on the device
    dev = eng.device
    d_img = img[:used.value // 4].to(dev)
    d_dual = [torch.full(tuple(t.shape), float("nan"), device=dev) for t in duals]
    d_prim = [torch.full(tuple(t.shape), float("nan"), device=dev) for t in prims]
    dptr = (C.c_void_p * nd)(*[t.data_ptr() for t in d_dual])
    pptr = (C.c_void_p * npr)(*[t.data_ptr() for t in d_prim])
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    cur = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(eng.lib.gnnb_scatter_amb_records(eng.h, d_img.data_ptr(), B, dptr, nd, pptr, npr, st.data_ptr(), cur), "gnnb_scatter_amb_records")
    torch.cuda.synchronize()
    assert int(st.cpu()[0]) == 0
    for k in range(L):
        lb, ub = lbs[k + 1].reshape(-1), ubs[k + 1].reshape(-1)
        amb = (lb < 0) & (ub > 0)
        got = d_dual[k].cpu().reshape(-1, 3)
        assert torch.equal(got[amb][:, 1:], duals[k].reshape(-1, 3)[amb][:, 1:])
        assert torch.isnan(got[~amb]).all() and torch.isnan(got[:, 0]).all()
        for m in (relu_q[k] - 1, relu_q[k]):
            gp = d_prim[m].cpu().reshape(-1)
            assert torch.equal(gp[amb], prims[m].reshape(-1)[amb]) and torch.isnan(gp[~amb]).all()
    assert torch.equal(d_prim[-1].cpu().reshape(-1), prims[-1].reshape(-1))
    # ---- a foreign or corrupt image is refused, not scattered (status bit 2): wrong batch size in the header, a record beyond its array
    for how in ("batch", "index", "layer"):
        bad = img[:used.value // 4].clone()
        if how == "batch":
            bad[3] = B + 1
        elif how == "index":
            bad[16 + 1] = B * eng.sizes[1 + int(bad[16])] + 5          # record 0: flat node index past the end of its layer
        else:
            bad[16] = L + 3
        d_bad = bad.to(dev)
        p_dual = [torch.full(tuple(t.shape), float("nan"), device=dev) for t in duals]
        p_prim = [torch.full(tuple(t.shape), float("nan"), device=dev) for t in prims]
        dptr = (C.c_void_p * nd)(*[t.data_ptr() for t in p_dual])
        pptr = (C.c_void_p * npr)(*[t.data_ptr() for t in p_prim])
        st.zero_()
        _lib.check(eng.lib.gnnb_scatter_amb_records(eng.h, d_bad.data_ptr(), B, dptr, nd, pptr, npr, st.data_ptr(), cur), "gnnb_scatter_amb_records")
        torch.cuda.synchronize()
        assert int(st.cpu()[0]) == 4, how
        if how == "batch":                                       # header mismatch: nothing at all is written
            assert all(torch.isnan(t).all() for t in p_dual + p_prim)


def test_two_networks_alternate_through_one_engine_and_pipeline():
    """ADVICE (round 5): the compact path packs with the sizes of whatever network the HANDLE is bound to.  Two networks of equal depth
    (cifar_base_kw, cifar_wide_kw) alternating through one engine -- through the pipeline and through eng.forward between submits -- must
    each be packed under their own binding: scores equal the device-resident forward's; tensors of the wrong size raise ValueError
    before the C packer sees a pointer."""
    from gnn_branching_amd import engine as E, synth
    model = make_model("shipped")
    eng = model.engine()
    dev = eng.device
    batches = [synth.make_batch(net, 6, seed=300 + i) for i, net in enumerate(["cifar_base_kw", "cifar_wide_kw", "cifar_base_kw", "cifar_wide_kw", "cifar_wide_kw"])]
    want = []
    with torch.no_grad():
        for b in batches:
            args = b.forward_args()
            d = [[t.to(dev) for t in g] if isinstance(g, list) else g for g in args]
            d[4], d[6] = args[4].to(dev), args[6].to(dev)
            want.append(eng.forward(*d).check().scores.cpu().numpy())
    pipe = E.HostFedPipeline(eng, compact=True)
    other = synth.make_batch("cifar_deep_kw", 2, seed=9)
    got = []
    with torch.no_grad():
        for i, b in enumerate(batches):
            got.append(pipe.submit(*b.forward_args()))
            if i == 1:                                            # someone else rebinds the shared engine between two submits
                eng.forward(*other.forward_args()).check()
    for r, w in zip(got, want):
        r.check()
        assert np.array_equal(r.scores.cpu().numpy(), w, equal_nan=True)
    bad = list(batches[0].forward_args())
    bad[2] = [t[:-3] for t in bad[2]]                             # dual_vars three rows short
    with pytest.raises(ValueError):
        pipe.submit(*bad)


def device_args(batch, dev):
    args = batch.forward_args()
    d = [[t.to(dev) for t in g] if isinstance(g, list) else g for g in args]
    d[4], d[6] = args[4].to(dev), args[6].to(dev)
    return d


def test_forward_host_stages_through_the_handles_helper_threads():
    """gnnb_forward_host copies a staging block of 4 MiB or more on the handle's helper threads -- the pool gnnb_pack_amb_records also
    uses -- and a smaller one on the calling thread.  cifar_base_kw stages ~34.7k floats per sample: B = 32 is past the threshold, B = 2
    far below it.  Either way scores and decisions are the bits of the device-resident forward, on every call (the pool is reused) and
    after a compact HostFedPipeline.submit on the same engine (both users share one pool), whose own result stays bit-identical too."""
    from gnn_branching_amd import engine as E, synth
    from tests.common import shipped_state
    eng = E.ScorerEngine(shipped_state())
    big, small = synth.make_batch("cifar_base_kw", 32, seed=41), synth.make_batch("cifar_base_kw", 2, seed=42)
    want = {}
    with torch.no_grad():
        for b in (big, small):
            r = eng.forward(*device_args(b, eng.device)).check()
            want[b.batch_size] = (r.scores.cpu().numpy(), r.decisions.cpu().numpy())
    # what gnnb_forward_host stages, in 64-float slots: both bounds of every graph layer, the duals, the two primals of every ReLU layer
    # and primals[-1], the input point, the property rows and the mask (the engine's sizes: nothing of it can silently shrink)
    def staged_bytes(B):
        pad = lambda n: (n + 63) & ~63
        n = sum(2 * pad(B * s) for s in eng.sizes) + sum(pad(3 * B * s) + 2 * pad(B * s) for s in eng.sizes[1:-1]) + pad(B)
        return 4 * (n + pad(B * eng.sizes[0]) + pad(B * eng.sizes[-2]) + pad(B) + pad(B * eng.R))
    assert staged_bytes(32) > (4 << 20) > staged_bytes(2)

    def host_calls():
        for b in (big, small, big, small):
            dec, scores = eng.forward_host(*b.forward_args(), want_scores=True)
            assert np.array_equal(scores, want[b.batch_size][0], equal_nan=True) and np.array_equal(dec, want[b.batch_size][1])
    host_calls()
    with torch.no_grad():
        r = E.HostFedPipeline(eng, compact=True).submit(*big.forward_args()).check()
    assert np.array_equal(r.scores.cpu().numpy(), want[32][0], equal_nan=True) and np.array_equal(r.decisions.cpu().numpy(), want[32][1])
    host_calls()


def test_pipeline_on_an_engine_made_with_an_index_less_device():
    """ScorerEngine(state, device="cuda") keeps the device WITH its index, so the status tensor the compact pipeline allocates on it
    passes forward's device check (it used to raise: cuda != cuda:0)."""
    from gnn_branching_amd import engine as E, synth
    from tests.common import register_toy_archs, shipped_state
    register_toy_archs()
    eng = E.ScorerEngine(shipped_state(), device="cuda")
    assert eng.device == torch.device("cuda", torch.cuda.current_device())
    batch = synth.make_batch("toy_single", 2, seed=7)            # one ReLU layer: the smallest network of tests/common.py
    with torch.no_grad():
        want = eng.forward(*device_args(batch, eng.device)).check()
        got = E.HostFedPipeline(eng, compact=True).submit(*batch.forward_args()).check()
    assert torch.equal(got.scores, want.scores) and torch.equal(got.decisions, want.decisions)
