"""Host plumbing between the reference-shaped Python surface and the C-ABI (include/gnnb.h).

``ScorerEngine`` owns one gnnb handle: the packed GNN weights, the bound verified
network and a workspace per batch size.  Tensors are only carriers of device
memory here (``data_ptr()``); all arithmetic of the hot path runs in libgnnb.so.
"""
import collections
import contextlib
import ctypes as C
import time

from array import array as _array

import numpy as np
import torch
from torch import nn

from . import _lib
from .plnn.modules import Flatten


def _is_flatten(layer):
    # the caller may hand over the reference's own plnn.modules.Flatten instances
    return isinstance(layer, Flatten) or type(layer).__name__ == "Flatten"


def state_blob(state_dict):
    """The checkpoint's 52 tensors concatenated in state-dict order (host fp32 array)."""
    parts = [np.asarray(v.detach().cpu().float().numpy() if torch.is_tensor(v) else v, dtype=np.float32).reshape(-1)
             for v in state_dict.values()]
    return np.ascontiguousarray(np.concatenate(parts))


# (out, in) of the 26 Linear layers in state-dict order (graph_conv.py:26-74, :428-437)
GNN_LINEARS = [(64, 3), (64, 64), (64, 2), (64, 64), (64, 128), (64, 64), (64, 7), (64, 64), (64, 128), (64, 64), (64, 128),
               (64, 64), (64, 4), (64, 128), (64, 64), (64, 7), (64, 64), (64, 64), (64, 192), (64, 64), (64, 128), (64, 64),
               (64, 128), (64, 64), (64, 64), (1, 64)]
GNN_BLOB_FLOATS = 117825        # the 52 tensors of GraphNet(2, 64) (graph_conv.py:20-76, :281-305, :428-437)


class BabsrResult:
    """Device outputs of one batched BaBSR scoring: `score` and `intercept_tb` of kw_score_conv.py:86, :103, padded
    (B, R) over the concatenated ReLU layers (already multiplied by the mask)."""
    __slots__ = ("scores", "intercepts", "masks", "relu_sizes")

    def __init__(self, scores, intercepts, masks, relu_sizes):
        self.scores, self.intercepts, self.masks, self.relu_sizes = scores, intercepts, masks, relu_sizes

    def per_layer(self, b):
        """(score list, intercept list, mask list) of subproblem b, one 1-D tensor per ReLU layer."""
        return tuple(list(torch.split(t[b], self.relu_sizes)) for t in (self.scores, self.intercepts, self.masks))


class KwBoundsResult:
    """Device outputs of one gnnb_kw_bounds call: fp64 bounds of graph layers 1..L+1 (lists of (B, N_k) tensors, split mask applied),
    optionally their fp32 copies laid out as GraphNet.forward's lower_bounds_all / upper_bounds_all (graph layers 0..L+1, layer 0 =
    the box, in the shape x_lo was given in), and the (B,) int32 infeasible flags; counts: None, or gnnb_kw_tighten's (B, 2) int32.
    Nothing is synchronised."""
    __slots__ = ("lb", "ub", "lb32", "ub32", "infeasible", "counts")

    def __init__(self, lb, ub, lb32, ub32, infeasible, counts=None):
        self.lb, self.ub, self.lb32, self.ub32, self.infeasible, self.counts = lb, ub, lb32, ub32, infeasible, counts


class DualAscentResult:
    """Device tensors of one ``ScorerEngine.dual_ascent`` call.  bound (B,), alpha / beta (B, R): the best value of the dual and its
    point, fp64; grad_alpha / grad_beta: None, or the supergradient at the entry point; dual / primals / x_lp: None, or the scorer's
    inputs at the best point, fp32, as ``forward`` takes them (primals: one tensor per network layer; only the pre- and post-activation
    of every ReLU layer and the last one are filled, the others are one-element placeholders)."""

    def __init__(self, bound, alpha, beta, grad_alpha, grad_beta, dual, primals, x_lp):
        self.bound, self.alpha, self.beta, self.grad_alpha, self.grad_beta = bound, alpha, beta, grad_alpha, grad_beta
        self.dual, self.primals, self.x_lp = dual, primals, x_lp


def f64(t, B, n, what, device):
    """t as a contiguous (B, n) fp64 tensor on the device."""
    t = torch.as_tensor(t).to(device=device, dtype=torch.float64).contiguous()
    if t.numel() != B * n:
        raise ValueError(f"{what}: {tuple(t.shape)} does not hold {B}x{n} values")
    return t.view(B, n)


class _HostBuf:
    """address + element count of a float32 C-contiguous host buffer (a CPU tensor as it is, or a numpy copy of a python list /
    array / tensor of another layout); holds the owner alive.  (A decision is ~0.3 ms of device work: numpy views and
    ``.ctypes`` objects for two dozen small inputs were a tenth of that again.)"""
    __slots__ = ("ptr", "size", "keep")

    def __init__(self, t):
        # data_ptr() is taken as a HOST address only of a tensor that lives on the host: a device tensor slipping through
        # here would be a wild host read inside gnnb_forward_host, so it is copied back by _host instead
        if torch.is_tensor(t) and t.device.type == "cpu" and t.dtype == torch.float32 and t.is_contiguous() \
                and not t.requires_grad:
            self.ptr, self.size, self.keep = t.data_ptr(), t.numel(), t
        else:
            a = ScorerEngine._host(t)
            self.ptr, self.size, self.keep = a.ctypes.data, a.size, a


def count(t):
    """Elements of a tensor, a numpy array or a ``_HostBuf``."""
    return t.size if type(t) is _HostBuf or isinstance(t, np.ndarray) else t.numel()


def ptr(t):
    """Address of a tensor (of either side), a numpy array or a ``_HostBuf``; None stays None."""
    if t is None:
        return None
    return t.ptr if type(t) is _HostBuf else t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def table(ts):
    """A C array of the entries' addresses (None stays None); the carriers of the per-decision paths are taken without a call to ``ptr``."""
    if ts is None:
        return None
    return (C.c_void_p * len(ts))(*[t.ptr if type(t) is _HostBuf else t.data_ptr() if type(t) is torch.Tensor else ptr(t) for t in ts])


def batch_size(first, prop_layers):
    """B of the batch whose first tensor is ``first``: one property layer per subproblem."""
    B = int(first.shape[0])
    if len(prop_layers) != B:
        raise ValueError(f"{len(prop_layers)} property layers for a batch of {B}")
    return B


def check_batch(sizes, R, fixed_layers, B, lbs, ubs, duals=None, prim=None, x_lp=None, mask=None):
    """THE size rule of a scorer batch: ValueError unless every group given holds what B subproblems on the bound network hold
    (``sizes``: its graph layers, ``R``: its ReLU nodes, ``fixed_layers``: its layer list).  The groups hold tensors, numpy arrays or
    ``_HostBuf`` objects; a group that is None is not looked at (``babsr`` has neither duals nor primals).  Needs no GPU and no handle."""
    ng, npr = len(sizes), len(fixed_layers) + 1
    bounds = {k: B * n for k, n in enumerate(sizes)}
    primals, k = {npr - 1: B}, 0                      # primals[q] is the output of network layer q: read on both sides of a ReLU, and the last one
    for q, l in enumerate(fixed_layers):
        if type(l) is nn.ReLU:
            k += 1
            primals[q - 1] = primals[q] = bounds[k]
    for what, g, n, want in (("lower_bounds_all[{}]", lbs, ng, bounds), ("upper_bounds_all[{}]", ubs, ng, bounds),
                             ("dual_vars[{}]", duals, ng - 2, {k: 3 * B * n for k, n in enumerate(sizes[1:-1])}), ("primals[{}]", prim, npr, primals),
                             ("masks", None if mask is None else [mask], 1, {0: B * R}), ("primal_inputs", None if x_lp is None else [x_lp], 1, {0: bounds[0]})):
        if g is None:
            continue
        if len(g) != n:
            raise ValueError(f"{what.split('[')[0]}: {len(g)} tensors, expected {n} (a layer graph of {ng} layers, {npr - 1} network layers)")
        for k, c in want.items():
            t = g[k]                                  # (count(t), the two carriers of the per-decision paths without the call)
            if (t.size if type(t) is _HostBuf else t.numel() if type(t) is torch.Tensor else count(t)) != c:
                raise ValueError(f"{what.format(k)} holds {count(t)} values, expected {c} (a batch of {B})")


def make_batch(lbs, ubs, duals, prim, x_lp, mask, pw=None, pb=None):
    """(gnnb_batch, what must outlive the call) of the named groups: anything ``ptr`` takes, of the side the entry point reads."""
    tabs = [table(g) for g in (lbs, ubs, duals, prim)]
    return _lib.Batch(tabs[0], tabs[1], tabs[2], tabs[3], ptr(x_lp), ptr(pw), ptr(pb), ptr(mask), len(lbs), len(duals), len(prim)), tabs


_NO_CONTEXT = contextlib.nullcontext()


def _or_reduce(status):
    v = 0
    for x in status.cpu().tolist():
        v |= int(x)
    return v


def _raise_for_status(st):
    """status word of gnnb_forward: bit 0 = an embedding was NaN (the reference enters pdb there, graph_conv.py:184-186, :339-341);
    bit 1 = a wait inside a kernel (k_gather_update_q's LDS ring, or k_top's workgroup split waiting for its partner workgroups)
    ran into its iteration cap: a protocol bug, a wedged GPU, or -- for k_top -- partner workgroups kept off the chip by other work
    (handle option "top_split" = 1 turns the split off); results are invalid.  bit 2 = gnnb_scatter_amb_records refused a record image
    (not packed for this binding / batch size, or a record outside its arrays)."""
    if st & 2:
        msg = ("a wait inside a kernel (k_gather_update_q ring or k_top workgroup split) hit its iteration cap (status bit 1); "
               "results are invalid; the handle option top_split=1 disables the k_top split")
        print(f"[gnn_branching_amd] {msg}", flush=True)
        raise RuntimeError(msg)
    if st & 4:
        msg = "gnnb_scatter_amb_records refused a record image (status bit 2): packed for another network or batch size, or corrupt"
        print(f"[gnn_branching_amd] {msg}", flush=True)
        raise RuntimeError(msg)
    if st & 1:
        msg = "mu contains nan"
        print(f"[gnn_branching_amd] {msg}", flush=True)
        raise FloatingPointError(msg)


# a set of child rows given as loose tensors (ScorerEngine.frontier_commit / frontier_commit_jobs)
_ChildRows = collections.namedtuple("_ChildRows", "mask lb ub infeasible bound alpha beta ubv live")
# the tensor arguments of GraphNet.forward in check_batch's and make_batch's order; what ScorerEngine._marshal returns (inputs on the device)
_Inputs = collections.namedtuple("_Inputs", "lbs ubs duals prim x_lp mask")
_Marshalled = collections.namedtuple("_Marshalled", "B lbs ubs duals prim x_lp mask pw pb")


class ForwardResult:
    """Device outputs of one batched forward.  `ready` (BatchPipeline only): the event behind the forward on the side stream it ran on."""
    __slots__ = ("scores", "decisions", "status", "masks", "ready")

    def __init__(self, scores, decisions, status, masks, ready=None):
        self.scores, self.decisions, self.status, self.masks, self.ready = scores, decisions, status, masks, ready

    def wait(self):
        """Order the caller's current stream behind the forward (a no-op for a forward that ran on that stream)."""
        if self.ready is not None:
            cur = torch.cuda.current_stream(self.scores.device)
            cur.wait_event(self.ready)
            for t in (self.scores, self.decisions, self.status):
                t.record_stream(cur)          # (allocated on the side stream: keep the allocator from recycling them under the caller)
        return self

    def check(self):
        """Synchronises.  Raises like the reference would stop (it enters pdb on NaN embeddings,
        graph_conv.py:184-186, :339-341)."""
        if self.ready is not None:
            self.ready.synchronize()
            cur = torch.cuda.current_stream(self.scores.device)
            for t in (self.scores, self.decisions, self.status):
                t.record_stream(cur)          # (as wait(): allocated on the side stream, from here on used by the caller's)
        _raise_for_status(_or_reduce(self.status))
        return self

    def ragged(self):
        """list of B 1-D tensors: the scores of the ambiguous ReLUs of each sample (graph_conv.py:470)."""
        return [self.scores[b][self.masks[b] != 0] for b in range(self.scores.shape[0])]


def _sent(inp, compact=False):
    """The tensors of an _Inputs that cross the link whole, in copy order (compact: dual_vars / primals go as records instead)."""
    return [*inp.lbs, *inp.ubs, *([] if compact else [*inp.duals, *inp.prim]), inp.x_lp, inp.mask]


class _FedSlot:
    """One set of device input buffers of a HostFedPipeline: ``dev`` (an _Inputs of full-size device tensors), ``sent`` (those of it that
    are copied whole) and ``offs`` (per entry of ``sent`` its offset in the slot's shared small block; None: a tensor of its own).
    Tensors below ``small_bytes`` share ONE pinned staging block and ONE device block (a copy of a few KB costs ~10 us of the copy
    queue's time each, tools/hostfed_probe.py: a batch has a dozen of them).  ev_copy: behind the slot's last copies; ev_done: behind
    the forward that last read it; img_cap / pin_img / dev_img: the record image of a compact slot."""

    def __init__(self, key, host, compact, device, small_bytes):
        def padded(t):
            return (t.numel() + 63) & ~63
        tot = sum(padded(t) for t in _sent(host, compact) if t.numel() * 4 < small_bytes)
        self.key, self.used, self.offs = key, False, []
        self.dev_small = torch.empty(max(tot, 1), dtype=torch.float32, device=device)
        self.pin_small = torch.empty(max(tot, 1), dtype=torch.float32, pin_memory=True)
        self.pin_np = self.pin_small.numpy()
        at = 0

        def twin(t, whole=True):
            nonlocal at
            if not whole:                      # filled by the scatter (entries of nodes that are never ambiguous are never read: zero, not garbage)
                return torch.zeros(t.shape, dtype=torch.float32, device=device)
            if t.numel() * 4 >= small_bytes:
                self.offs.append(None)
                return torch.empty(t.shape, dtype=torch.float32, device=device)
            self.offs.append(at)
            at += padded(t)
            return self.dev_small[self.offs[-1]:self.offs[-1] + t.numel()].view(t.shape)
        self.dev = _Inputs([twin(t) for t in host.lbs], [twin(t) for t in host.ubs], [twin(t, not compact) for t in host.duals],
                           [twin(t, not compact) for t in host.prim], twin(host.x_lp), twin(host.mask))
        self.sent = _sent(self.dev, compact)
        self.ev_copy, self.ev_done = torch.cuda.Event(), torch.cuda.Event()
        self.img_cap, self.pin_img, self.dev_img = 0, None, None


class HostFedPipeline:
    """Cross-batch double buffering for batches that arrive as HOST tensors (the reference pays its host->device copies inside the
    call, graph_score.py:26-30; SURVEY 8(d): "H2D reported separately").

    ``submit(*forward_args)`` enqueues the copies of batch i + 1 on a COPY stream while the forward of batch i runs on the caller's
    stream, and returns that batch's ForwardResult without synchronising: `depth` (2) sets of device input buffers, each guarded by
    two events -- the copy stream waits for the forward that last read a set before overwriting it, the compute stream waits for the
    set's copies before its forward.  Host tensors are copied straight from where they are, in pieces of 2 MB (see `_enqueue_copies`): from
    pinned memory the copies are asynchronous DMA that hides under the running forward; from pageable memory the runtime stages them
    (the host blocks per piece, the GPU still overlaps them with the previous forward).
    ``compact`` (default): of ``dual_vars`` and ``primals`` the forward reads only the entries of AMBIGUOUS nodes (and primals[-1]), so those
    tensors do not cross the link whole: ``gnnb_pack_amb_records`` gathers, on a few host threads, {index, dual[:, 1], dual[:, 2],
    primal_pre, primal_post} of the nodes with lb < 0 < ub into a pinned image (base B = 256: 1.2 MB instead of 17 MB), the image is
    copied, and one launch (``gnnb_scatter_amb_records``) writes the records into the slot's full-size device tensors in front of the
    forward.  36.5 -> 21 MB per base batch: the copies hide under the forward again.
    Scores are bit-identical to ``engine.forward`` on device-resident inputs (tests/test_gpu_hostfed.py)."""

    PIECE = 1 << 19            # floats per copy (2 MB)
    SMALL = 1 << 20            # bytes: tensors below it are staged together

    def __init__(self, engine, depth=2, compact=True):
        self.eng, self.depth = engine, max(2, int(depth))
        self.compact = bool(compact)
        self.link_bytes = 0
        self.copy_stream = torch.cuda.Stream(device=engine.device)
        self.slots = [None] * self.depth
        self.i = 0

    @staticmethod
    def _inputs(lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, masks):
        def f32(t):
            if not torch.is_tensor(t):
                t = torch.tensor(t, dtype=torch.float32)
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            return t
        return _Inputs([f32(t) for t in lower_bounds_all], [f32(t) for t in upper_bounds_all], [f32(t) for t in dual_vars],
                       [f32(t) for t in primals], f32(primal_inputs), f32(masks))

    def _slot(self, host, compact, B):
        """The next slot, shaped for this batch and free: its staging block has left the host, the copy stream waits for its last forward."""
        eng, k = self.eng, self.i % self.depth
        self.i += 1
        key = (compact,) + tuple(tuple(t.shape) for t in _sent(host))
        sl = self.slots[k]
        if sl is None or sl.key != key:
            if sl is not None:
                sl.ev_done.synchronize()
            sl = self.slots[k] = _FedSlot(key, host, compact, eng.device, self.SMALL)
            if compact:
                sl.img_cap = int(eng.lib.gnnb_amb_records_bytes(eng.h, B))
                sl.pin_img = torch.empty(sl.img_cap // 4, dtype=torch.int32, pin_memory=True)
                sl.dev_img = torch.empty(sl.img_cap // 4, dtype=torch.int32, device=eng.device)
        if sl.used:
            sl.ev_copy.synchronize()                 # the staging block of this set is free again (its last copies have left the host)
            self.copy_stream.wait_event(sl.ev_done)  # the forward that last read this set has finished
        return sl

    def _pack(self, sl, host, B):
        """gnnb_pack_amb_records of the host batch into the slot's pinned image; returns the image's length in words."""
        eng = self.eng
        hb, keep = make_batch(*host)
        used = C.c_size_t(0)
        _lib.check(eng.lib.gnnb_pack_amb_records(eng.h, C.byref(hb), B, sl.pin_img.data_ptr(), sl.img_cap, C.byref(used)), "gnnb_pack_amb_records")
        return (used.value + 3) // 4

    @staticmethod
    def _stage(sl, src):
        """Host memcpy of the small tensors into the slot's shared staging block (< 1 MB in all)."""
        for t, o in zip(src, sl.offs):
            if o is not None and t.device.type == "cpu":
                sl.pin_np[o:o + t.numel()] = t.reshape(-1).numpy()

    def _enqueue_copies(self, sl, src, used_words, cur):
        """On the copy stream: the small block, the record image, then every big tensor, in pieces; ev_copy behind them."""
        dev_src = [t for t in src if t.device.type != "cpu"]
        if dev_src:
            # sources that already live on the device (or temporaries _inputs made from them) were produced on the caller's
            # stream: the copy stream must not read them before that work is done, nor may the allocator recycle them under it
            self.copy_stream.wait_stream(cur)
            for t in dev_src:
                t.record_stream(self.copy_stream)
        small = [(d, t) for d, t, o in zip(sl.sent, src, sl.offs) if o is not None]
        with torch.cuda.stream(self.copy_stream):
            if small:
                if any(t.device.type != "cpu" for _, t in small):
                    for d, t in small:
                        d.copy_(t, non_blocking=True)
                else:
                    sl.dev_small.copy_(sl.pin_small, non_blocking=True)
            for o in range(0, used_words, self.PIECE):                 # the record image of the ambiguous nodes
                sl.dev_img[o:min(o + self.PIECE, used_words)].copy_(sl.pin_img[o:min(o + self.PIECE, used_words)], non_blocking=True)
            for d, t, off in zip(sl.sent, src, sl.offs):
                if off is not None:
                    continue
                # pieces of at most 2 MB: measured on MI355X / ROCm 7.2 (tools/hostfed_probe.py), 21 pinned copies of 1.7 MB on a side
                # stream hide completely under the forward (0.85 ms with or without them), ONE 36.5 MB copy beside the same forward
                # takes 3.1 ms.  Pageable tensors go through the runtime's own staging (synchronous for the host, still beside the
                # previous forward on the GPU); packing them into pinned memory here first cost 10 ms per batch.
                dv, sv = d.view(-1), t.reshape(-1)
                for o in range(0, sv.numel(), self.PIECE):
                    dv[o:o + self.PIECE].copy_(sv[o:o + self.PIECE], non_blocking=True)
            sl.ev_copy.record(self.copy_stream)

    def _scatter(self, sl, B, cur):
        """Records -> the slot's full-size dual / primal tensors, one launch in front of the forward.  Returns the status words
        [forward, scatter]: the scatter raises bit 2 on a foreign / corrupt image."""
        eng, d = self.eng, sl.dev
        status = torch.zeros(2, dtype=torch.int32, device=eng.device)
        _lib.check(eng.lib.gnnb_scatter_amb_records(eng.h, sl.dev_img.data_ptr(), B, table(d.duals), len(d.duals), table(d.prim), len(d.prim),
                                                    status[1:].data_ptr(), C.c_void_p(cur.cuda_stream)), "gnnb_scatter_amb_records")
        return status

    def submit(self, lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks):
        eng = self.eng
        host = self._inputs(lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, masks)
        compact = self.compact and all(t.device.type == "cpu" for t in _sent(host))
        B = int(host.lbs[0].shape[0])
        if compact:
            # the packer walks raw host pointers with the sizes of whatever network the HANDLE is bound to: bind (cached by key) on every
            # submit -- another pipeline or eng.forward on the shared engine may have rebound it since this slot was shaped -- and check every
            # element count against that binding before the C side sees a pointer
            eng.bind(layers["fixed_layers"], tuple(host.lbs[0].shape[1:]))
            check_batch(eng.sizes, eng.R, eng._net_keepalive, B, *host)
        with torch.cuda.device(eng.device):
            cur = torch.cuda.current_stream()
            sl = self._slot(host, compact, B)
            used_words = self._pack(sl, host, B) if compact else 0
            src = _sent(host, compact)
            self._stage(sl, src)
            self._enqueue_copies(sl, src, used_words, cur)
            cur.wait_event(sl.ev_copy)
            self.link_bytes = 4 * (used_words + sum(t.numel() for t in src))      # what this submit sent over the link
            status = self._scatter(sl, B, cur) if compact else None
            d = sl.dev
            res = eng.forward(d.lbs, d.ubs, d.duals, d.prim, d.x_lp, layers, d.mask, status=status)
            # the result outlives the slot: its mask must not be a view of the slot's device buffer, which the submit `depth` calls
            # later overwrites (a held result's ragged() would then be cut with another batch's mask).  Cloned on the compute stream,
            # behind the copies it waited for and in front of ev_done.
            res.masks = res.masks.clone()
            sl.ev_done.record(cur)
            sl.used = True
        return res


class BatchPipeline:
    """`depth` (2) INDEPENDENT batches in flight: one handle (own workspace, own control blocks) and one HIP stream per slot, batches
    dealt to the slots in turn.  A forward is a chain of 11-19 dependent launches; while one batch's kernel drains or its next one
    ramps up, the other batch's kernel fills the CUs: measured per batch on MI355X (tools/two_batches_probe.py) base B=256 0.769 ->
    0.728 ms, deep B=128 0.911 -> 0.785 ms.  Throughput, not latency: a batch takes longer from submit to ready.  Scores are bit-identical to
    ``ScorerEngine.forward`` (tests/test_gpu_pipeline.py).  The handles are created with k_top's workgroup split off (handle option "top_split" = 1):
    with a second batch's kernels on the chip the partner workgroups of a split sample are not guaranteed to be resident together.

    ``submit(*forward_args)`` returns the batch's ForwardResult at once; ``result.wait()`` orders the caller's stream behind it,
    ``result.check()`` synchronises on it; ``synchronize()`` waits for everything submitted."""

    def __init__(self, state_dict, depth=2, T=2, p=64, device=None, options=None):
        self.depth = max(1, int(depth))
        opts = dict(options or {})
        opts["top_split"] = 1             # whatever the caller or the environment says: partner workgroups are not guaranteed to be co-resident here
        self.engines = [ScorerEngine(state_dict, T, p, device, options=opts) for _ in range(self.depth)]
        self.device = self.engines[0].device
        self.streams = self._overlapping_streams(self.device, self.depth)
        self.i = 0

    @staticmethod
    def _overlapping_streams(device, n):
        """n streams whose kernels really run side by side.  HIP multiplexes streams onto a few hardware queues and two streams that share
        one run their kernels in order (measured on MI355X / ROCm 7.2, tools/two_batches_probe.py: of the first nine streams torch hands out
        the pairs (#2, #3) and (#0, #5) serialise, every other pair overlaps) -- so candidates are timed against the streams already
        chosen with two 0.3-ms spin kernels and taken only if the pair finishes in well under twice one kernel's time."""
        if not hasattr(torch.cuda, "_sleep"):                   # (no spin kernel to time with: take the streams as they come)
            return [torch.cuda.Stream(device=device) for _ in range(n)]

        def spin(st):
            with torch.cuda.stream(st):
                torch.cuda._sleep(700000)

        def pair_ms(a, b):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            spin(a)
            spin(b)
            torch.cuda.synchronize(device)
            return 1e3 * (time.perf_counter() - t0)

        with torch.cuda.device(device):
            chosen = [torch.cuda.Stream(device=device)]
            pair_ms(chosen[0], chosen[0])                       # (first launch of the spin kernel)
            serial = min(pair_ms(chosen[0], chosen[0]) for _ in range(2))
            spare = []
            for _ in range(12):
                if len(chosen) == n:
                    break
                cand = torch.cuda.Stream(device=device)
                if all(min(pair_ms(cand, s), pair_ms(cand, s)) < 0.75 * serial for s in chosen):
                    chosen.append(cand)
                else:
                    spare.append(cand)
            chosen += spare[:n - len(chosen)]                    # (no overlapping candidate found: still correct, just no faster)
            while len(chosen) < n:
                chosen.append(torch.cuda.Stream(device=device))
        return chosen

    def submit(self, lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks):
        k = self.i % self.depth
        self.i += 1
        eng, st = self.engines[k], self.streams[k]
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            if not cur.query():                                  # the inputs were produced on the caller's stream: wait for it -- unless it is idle:
                st.wait_stream(cur)                              # an event recorded on the default stream orders it against every other stream's
                                                                 # work, and the two batches then run one after the other (0.94 instead of 0.78 ms)
            # Lifetime contract: the caller may drop or overwrite-by-reallocation its inputs as soon as submit returns -- every device
            # input is marked as in use by the side stream, so the caching allocator will not hand its memory out again before the
            # forward has read it.  (Writing INTO an input tensor in place before result.wait() / check() is still a race.)
            for grp in (lower_bounds_all, upper_bounds_all, dual_vars, primals, [primal_inputs, masks]):
                for t in grp:
                    if torch.is_tensor(t) and t.device.type == "cuda":
                        t.record_stream(st)
            with torch.cuda.stream(st):
                res = eng.forward(lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks)
                res.ready = torch.cuda.Event()
                res.ready.record(st)
        return res

    def synchronize(self):
        for st in self.streams:
            st.synchronize()


class ScorerEngine:
    def __init__(self, state_dict, T=2, p=64, device=None, options=None):
        """options: {name: int} of handle options (include/gnnb.h gnnb_set_option; _lib.OPTIONS), applied over the ones the
        environment names (_lib.OPTION_ENV: the tests' and bench.py's switches; the library itself reads no environment)."""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("gnn_branching_amd needs an AMD GPU (MI355X / gfx950); there is no CPU path")
        self.device = torch.device("cuda" if device is None else device)
        if self.device.index is None:             # always with its index: comparisons against a tensor's device mean what they say
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.T, self.p = T, p
        # state_dict None: a handle for the GNN-free entry points only (gnnb_babsr) -- all-zero GNN weights
        blob = state_blob(state_dict) if state_dict is not None else np.zeros(GNN_BLOB_FLOATS, dtype=np.float32)
        self._blob = blob
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gnnb_create(C.byref(h), blob.ctypes.data_as(C.c_void_p), blob.size, T, p), "gnnb_create")
        self.h = h
        self.options = dict(_lib.options_from_env())
        self.options.update(options or {})
        for name, value in self.options.items():
            self.set_option(name, value)
        self._net_key = None
        self._net_keepalive = None
        self.sizes = None
        self.R = 0
        self._ws = {}
        self._prop_cache = {}
        self._prop_host_cache = None

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.lib.gnnb_destroy(h)
            except Exception:
                pass

    # ---- handle options ---------------------------------------------------------------------
    def set_option(self, name, value):
        """gnnb_set_option: see include/gnnb.h for the table.  "gather" and "dense_lds" must be set before the first bind."""
        _lib.check(self.lib.gnnb_set_option(self.h, name.encode(), int(value)), f"gnnb_set_option({name})")
        self.options[name] = int(value)

    def get_option(self, name):
        v = C.c_int(0)
        _lib.check(self.lib.gnnb_get_option(self.h, name.encode(), C.byref(v)), f"gnnb_get_option({name})")
        return v.value

    # ---- verified network -------------------------------------------------------------------
    def bind(self, fixed_layers, input_shape):
        key = (tuple(id(l) for l in fixed_layers),
               tuple((l.weight.data_ptr(), l.weight._version) for l in fixed_layers if hasattr(l, "weight")),
               tuple(input_shape))
        if key == self._net_key:
            return
        descs = (_lib.LayerDesc * len(fixed_layers))()
        keep = []
        for d, l in zip(descs, fixed_layers):
            if type(l) is nn.Conv2d:
                if l.dilation != (1, 1) or l.groups != 1 or l.stride[0] != l.stride[1] or l.padding[0] != l.padding[1]:
                    raise NotImplementedError(f"unsupported conv geometry: {l}")
                w = np.ascontiguousarray(l.weight.detach().cpu().float().numpy())
                b = np.ascontiguousarray(l.bias.detach().cpu().float().numpy())
                keep += [w, b]
                d.kind, d.c_in, d.c_out = _lib.GNNB_CONV, l.in_channels, l.out_channels
                d.kh, d.kw, d.stride, d.pad = l.kernel_size[0], l.kernel_size[1], l.stride[0], l.padding[0]
                d.weight, d.bias = w.ctypes.data, b.ctypes.data
            elif type(l) is nn.Linear:
                w = np.ascontiguousarray(l.weight.detach().cpu().float().numpy())
                b = np.ascontiguousarray(l.bias.detach().cpu().float().numpy())
                keep += [w, b]
                d.kind, d.n_in, d.n_out = _lib.GNNB_LINEAR, l.in_features, l.out_features
                d.weight, d.bias = w.ctypes.data, b.ctypes.data
            elif type(l) is nn.ReLU:
                d.kind = _lib.GNNB_RELU
            elif _is_flatten(l):
                d.kind = _lib.GNNB_FLATTEN
            else:
                raise NotImplementedError(type(l))        # reference: graph_conv.py:191-192
        c0, h0, w0 = (tuple(input_shape) + (1, 1))[:3]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gnnb_bind_network(self.h, descs, len(fixed_layers), c0, h0, w0), "gnnb_bind_network")
        ng, R = C.c_int(), C.c_int()
        _lib.check(self.lib.gnnb_graph_info(self.h, C.byref(ng), None, C.byref(R)), "gnnb_graph_info")
        sizes = (C.c_int * ng.value)()
        _lib.check(self.lib.gnnb_graph_info(self.h, C.byref(ng), sizes, C.byref(R)), "gnnb_graph_info")
        self.sizes, self.R = list(sizes), R.value
        self._net_key = key
        self._net_keepalive = list(fixed_layers)
        self._ws.clear()

    # ---- one forward ------------------------------------------------------------------------
    def _call(self, name, *args):
        """Entry point ``name`` of the library with the handle in front of ``args`` and the current stream behind them; a failure raises."""
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(self.h, *args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, name)

    def _dev(self, t):
        if not torch.is_tensor(t):
            t = torch.tensor(t, dtype=torch.float32)       # python lists of LP primals (graph_score.py:30)
        return t.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()

    def _prop(self, prop_layers):
        """(B, N_L) weights and (B,) biases of the per-sample property layers (graph_conv.py:196-199)."""
        key = tuple(id(l) for l in prop_layers)
        vkey = tuple((l.weight.data_ptr(), l.weight._version) for l in {id(l): l for l in prop_layers}.values())
        hit = self._prop_cache.get(key)
        if hit is not None and hit[0] == vkey:
            return hit[1], hit[2]
        uniq, index = {}, []
        for l in prop_layers:
            if id(l) not in uniq:
                if l.weight.shape[0] != 1:
                    raise NotImplementedError("the property layer must be Linear(., 1)")   # graph_conv.py:80
                uniq[id(l)] = (len(uniq), l)
            index.append(uniq[id(l)][0])
        w = torch.stack([l.weight.detach()[0].float() for _, l in uniq.values()]).to(self.device)
        b = torch.stack([l.bias.detach()[0].float() for _, l in uniq.values()]).to(self.device)
        idx = torch.tensor(index, device=self.device)
        pw, pb = w[idx].contiguous(), b[idx].contiguous()
        if len(self._prop_cache) > 8:
            self._prop_cache.clear()
        self._prop_cache[key] = (vkey, pw, pb, list(prop_layers))
        return pw, pb

    def _workspace(self, key, B, sizer):
        """The cached device workspace of (key, B) for the bound network, ``sizer`` (a gnnb_*workspace_bytes) bytes long."""
        ws = self._ws.get((key, B))
        if ws is None:
            n = getattr(self.lib, sizer)(self.h, B)
            if n == 0:
                raise RuntimeError(f"{sizer} returned 0 (no network bound?)")
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            if len(self._ws) > 6:
                self._ws.clear()
            self._ws[(key, B)] = ws
        return ws

    def workspace(self, B):
        return self._workspace("forward", B, "gnnb_workspace_bytes")

    def kw_workspace(self, B):
        return self._workspace("kw", B, "gnnb_kw_workspace_bytes")

    def dual_workspace(self, B):
        return self._workspace("dual", B, "gnnb_dual_workspace_bytes")

    def _marshal(self, lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks):
        """Bind the network, move the arguments of GraphNet.forward to the device and validate their sizes: a _Marshalled."""
        fixed = layers["fixed_layers"]
        self.bind(fixed, tuple(lower_bounds_all[0].shape[1:]))
        B = batch_size(lower_bounds_all[0], layers["prop_layers"])
        m = _Marshalled(B, [self._dev(t) for t in lower_bounds_all], [self._dev(t) for t in upper_bounds_all], [self._dev(t) for t in dual_vars],
                        [self._dev(t) for t in primals], self._dev(primal_inputs), self._dev(masks), *self._prop(layers["prop_layers"]))
        check_batch(self.sizes, self.R, fixed, B, m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask)
        self._last_bounds = list(zip(m.lbs, m.ubs))           # for mu() (inspection)
        return m

    def forward(self, lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks, status=None):
        """One gnnb_forward call on the current stream.  status: optional preallocated device int32 tensor; the forward's status word
        goes to element 0, further elements (HostFedPipeline: the scatter launch's word) are left to the caller and OR-ed in by
        ForwardResult.check()."""
        m = self._marshal(lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks)
        B = m.B
        scores = torch.empty(B, self.R, dtype=torch.float32, device=self.device)
        dec = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty(1, dtype=torch.int32, device=self.device)
        elif status.numel() < 1 or status.dtype != torch.int32 or status.device != self.device:
            raise ValueError("forward: `status` must be a device int32 tensor with at least one element")
        batch, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
        ws = self.workspace(B)
        self._call("gnnb_forward", C.byref(batch), B, scores.data_ptr(), dec.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())
        return ForwardResult(scores, dec, status, m.mask.view(B, self.R))

    # ---- the reference's own call pattern: host tensors, one or two subproblems ---------------------------------
    @staticmethod
    def _host(t):
        """float32 C-contiguous numpy view / copy of a tensor (of ANY device: the reference's driver hands over `.cuda()`
        layers next to CPU bounds, relu_conv_gnnkwthreshold.py:111-117), python list or array -- always HOST memory."""
        if torch.is_tensor(t):
            t = t.detach()
            if t.device.type != "cpu":
                t = t.cpu()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            return t.numpy()
        if type(t) is list and t and type(t[0]) is float:
            # the LP primals arrive as flat python lists of floats (graph_score.py:30): array('f') walks them in C, a third faster
            # than numpy's generic sequence path (same round-to-nearest double -> float conversion)
            try:
                return np.frombuffer(_array("f", t), dtype=np.float32)
            except TypeError:
                pass
        return np.ascontiguousarray(t, dtype=np.float32)

    _HostBuf = _HostBuf

    def _prop_host(self, props):
        """(B, N_L) weights and (B,) biases of the property layers as numpy arrays, cached on the layer objects' identity + version"""
        key = tuple((id(l), l.weight.data_ptr(), l.weight._version, l.bias._version) for l in props)
        hit = self._prop_host_cache
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        for l in props:
            if l.weight.shape[0] != 1:
                raise NotImplementedError("the property layer must be Linear(., 1)")   # graph_conv.py:80
        pw = np.ascontiguousarray(np.stack([self._host(l.weight)[0] for l in props]))
        pb = np.ascontiguousarray(np.array([self._host(l.bias)[0] for l in props], dtype=np.float32))
        self._prop_host_cache = (key, pw, pb, list(props))
        return pw, pb

    def forward_host(self, lower_bounds_all, upper_bounds_all, dual_vars, primals, primal_inputs, layers, masks, want_scores=False):
        """``forward`` for CPU inputs through ``gnnb_forward_host``: every input the kernels read is packed into ONE pinned
        transfer by the library, and decisions / status (/ scores) come back in one block -- no torch device tensors, no
        per-tensor ``.cuda()`` (graph_score.py:26-30).  Synchronous.  Returns (decisions (B, 2) int32 array, scores (B, R)
        float32 array or None); raises FloatingPointError like ``ForwardResult.check``."""
        fixed = layers["fixed_layers"]
        self.bind(fixed, tuple(lower_bounds_all[0].shape[1:]))
        B = batch_size(lower_bounds_all[0], layers["prop_layers"])
        HB = self._HostBuf
        host = _Inputs([HB(t) for t in lower_bounds_all], [HB(t) for t in upper_bounds_all], [HB(t) for t in dual_vars], [HB(t) for t in primals],
                       HB(primal_inputs), HB(masks))
        check_batch(self.sizes, self.R, fixed, B, *host)
        batch, keep = make_batch(*host, *self._prop_host(layers["prop_layers"]))
        dec = np.empty((B, 2), dtype=np.int32)
        status = np.zeros(1, dtype=np.int32)
        scores = np.empty((B, self.R), dtype=np.float32) if want_scores else None
        # (no device context where the current device is already the engine's: this is the BaB loop's per-decision call)
        with _NO_CONTEXT if torch.cuda.current_device() == self.device.index else torch.cuda.device(self.device):
            rc = self.lib.gnnb_forward_host(self.h, C.byref(batch), B, scores.ctypes.data if want_scores else None, dec.ctypes.data,
                                            status.ctypes.data, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "gnnb_forward_host")
        _raise_for_status(int(status[0]))
        return dec, scores

    # ---- online learning --------------------------------------------------------
    def get_weights(self):
        """The GNN parameters as a flat float32 array in checkpoint order (see state_blob)."""
        out = np.empty(GNN_BLOB_FLOATS, dtype=np.float32)
        with torch.cuda.device(self.device):                      # (after a step in repack mode "device" it synchronises and reads the device)
            _lib.check(self.lib.gnnb_get_weights(self.h, out.ctypes.data_as(C.c_void_p), out.size), "gnnb_get_weights")
        return out

    def set_weights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gnnb_set_weights(self.h, blob.ctypes.data_as(C.c_void_p), blob.size), "gnnb_set_weights")
        self._blob = blob

    REPACK_MODES = {"host": 0, "device": 1}

    @classmethod
    def _repack_mode(cls, repack, what):
        if not isinstance(repack, str) or repack not in cls.REPACK_MODES:
            raise ValueError(f"{what}: repack = {repack!r} ('host' or 'device')")
        return cls.REPACK_MODES[repack]

    def online_create(self, lr=1e-4, wd=1e-4, repack="host"):
        """torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd) of graph_score_online.py:15.  repack: where the scorer's operand
        packs are rebuilt after a step, see ``set_repack``."""
        mode = self._repack_mode(repack, "online_create")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gnnb_online_create(self.h, lr, wd), "gnnb_online_create")
        self._online = True
        self.repack_mode = "host"
        if mode:
            self.set_repack(repack)

    def set_repack(self, mode):
        """gnnb_online_set_repack: "host" (the default) rebuilds the packs on the host after a learning step, which synchronises the
        stream; "device" builds them on the step's stream -- ``online_step_rows`` and ``imitation_step_rows`` then return without
        waiting, and a scorer call on ANOTHER stream must be ordered behind the step by the caller (the packs are rewritten in place)."""
        m = self._repack_mode(mode, "set_repack")
        if not getattr(self, "_online", False):
            raise RuntimeError("set_repack: call online_create first")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gnnb_online_set_repack(self.h, m), "gnnb_online_set_repack")
        self.repack_mode = mode

    def repack(self, stream=None):
        """gnnb_repack: the device pack builder from the trainer's parameters on ``stream`` (a torch stream; None: the current one).
        Stream-ordered, no synchronisation."""
        if not getattr(self, "_online", False):
            raise RuntimeError("repack: call online_create first")
        with torch.cuda.device(self.device):
            st = (torch.cuda.current_stream() if stream is None else stream).cuda_stream
            _lib.check(self.lib.gnnb_repack(self.h, C.c_void_p(st)), "gnnb_repack")

    def pack_image(self, which):
        """gnnb_pack_image: operand pack ``which`` (0..13) as it stands in device memory (float32 array), after a device synchronise."""
        n = C.c_size_t(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gnnb_pack_image(self.h, int(which), None, 0, C.byref(n)), "gnnb_pack_image")      # (the size query)
            out = np.empty(n.value, dtype=np.float32)
            _lib.check(self.lib.gnnb_pack_image(self.h, int(which), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), "gnnb_pack_image")
        return out

    def online_step(self, args, kw_index, improvement, apply=True, want_scores=False):
        """graph_score_online.py:62-77 for the batch ``args`` (the argument tuple of GraphNet.forward): kw_index (B) flat
        indices into the R ReLU nodes, improvement (B).  Returns (loss (B) numpy, scores (B, R) device tensor or None)."""
        if not getattr(self, "_online", False):
            raise RuntimeError("online_step: call online_create first")
        m = self._marshal(*args)
        B = m.B
        kw = np.ascontiguousarray(kw_index, dtype=np.int32).reshape(-1)
        imp = np.ascontiguousarray(improvement, dtype=np.float32).reshape(-1)
        if kw.size != B or imp.size != B:
            raise ValueError(f"online_step: {kw.size} KW decisions / {imp.size} improvements for a batch of {B}")
        mask_host = m.mask.view(B, self.R).cpu()
        for b in range(B):
            if not (0 <= kw[b] < self.R) or mask_host[b, kw[b]] == 0:
                raise IndexError(f"online_step: KW decision {int(kw[b])} of subproblem {b} is not an undecided ReLU of its mask")
        loss = np.empty(B, dtype=np.float32)
        scores = torch.empty(B, self.R, dtype=torch.float32, device=self.device) if want_scores else None
        batch, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            rc = self.lib.gnnb_online_step(self.h, C.byref(batch), B, kw.ctypes.data_as(C.c_void_p), imp.ctypes.data_as(C.c_void_p),
                                           loss.ctypes.data_as(C.c_void_p), scores.data_ptr() if want_scores else None,
                                           1 if apply else 0, C.c_void_p(st))
        _lib.check(rc, "gnnb_online_step")
        return loss, scores

    def online_step_rows(self, batch, K, rows, kw_index, improvement, loss=None, status=None, apply=True):
        """gnnb_online_step_rows on the current stream: ``online_step`` on the rows ``rows`` ((n,) int32 device tensor, in list order) of the
        K-row device batch ``batch`` (a ``_lib.Batch`` over device tensors, as ``make_batch`` builds it), with nothing crossing the link.
        kw_index (n,) int32 / improvement (n,) fp32: device tensors; loss: None, or a (n,) fp32 device tensor that receives the losses;
        status: None, or a zeroed (1,) int32 device tensor whose bit 3 (value 8) reports a row that named no undecided node or no row of
        the batch (that row's loss is NaN, the others are not affected).  Synchronises the stream, as ``online_step`` does, in repack
        mode "host"; in mode "device" (``set_repack``) a step with apply is only issued: loss and status are valid once the stream gets there."""
        if not getattr(self, "_online", False):
            raise RuntimeError("online_step_rows: call online_create first")
        n, i32, f32 = int(rows.numel()), torch.int32, torch.float32
        self._call("gnnb_online_step_rows", C.byref(batch), int(K), self._rows(rows, n, 1, i32, "rows").data_ptr(), n,
                   self._rows(kw_index, n, 1, i32, "kw_index").data_ptr(), self._rows(improvement, n, 1, f32, "improvement").data_ptr(),
                   None if loss is None else self._rows(loss, n, 1, f32, "loss").data_ptr(),
                   None if status is None else self._rows(status, 1, 1, i32, "status").data_ptr(), 1 if apply else 0)

    # ---- the imitation step ----------------------------------------------
    @staticmethod
    def _margin(margin, what):
        if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)) or not float(margin) >= 0.0:
            raise ValueError(f"{what}: margin = {margin!r} (a real number >= 0)")
        return float(margin)

    def imitation_step_rows(self, batch, K, rows, table, margin=1.0, loss=None, report=None, regret=None, status=None, apply=True):
        """gnnb_imitation_step_rows on the current stream: ``online_step_rows`` under the table loss (include/gnnb.h states the rule).
        rows (n,) int32 and table (K, R) fp64 (row = batch row, NaN: not a candidate -- what ``strong_pick`` leaves in ``table``) are
        device tensors; loss (n,) fp32, report (n, 4) int32 [teacher, pick, n_cand, n_viol], regret (n,) fp64 and status (1,) int32
        (zeroed by the caller; bit 3: a refused row) are None or device tensors that receive them.  Synchronises the stream where
        ``online_step_rows`` does: in repack mode "host", not in mode "device"."""
        if not getattr(self, "_online", False):
            raise RuntimeError("imitation_step_rows: call online_create first")
        margin = self._margin(margin, "imitation_step_rows")
        n, i32, f32, f64 = int(rows.numel()), torch.int32, torch.float32, torch.float64
        self._call("gnnb_imitation_step_rows", C.byref(batch), int(K), self._rows(rows, n, 1, i32, "rows").data_ptr(), n,
                   self._rows(table, int(K), self.R, f64, "table").data_ptr(), margin,
                   None if loss is None else self._rows(loss, n, 1, f32, "loss").data_ptr(),
                   None if report is None else self._rows(report, n, 4, i32, "report").data_ptr(),
                   None if regret is None else self._rows(regret, n, 1, f64, "regret").data_ptr(),
                   None if status is None else self._rows(status, 1, 1, i32, "status").data_ptr(), 1 if apply else 0)

    def imitation_step(self, args, table, margin=1.0, apply=True):
        """One imitation step on the batch ``args`` (the argument tuple of GraphNet.forward) and its (B, R) table (host or device, any
        float type; NaN: not a candidate): marshals and calls ``imitation_step_rows`` with rows = arange(B).  Returns (loss (B,) fp32,
        report (B, 4) int32, regret (B,) fp64) as numpy; raises IndexError when a row was refused (a candidate at a decided node, or an
        infinite table entry)."""
        if not getattr(self, "_online", False):
            raise RuntimeError("imitation_step: call online_create first")
        margin = self._margin(margin, "imitation_step")
        m = self._marshal(*args)
        B, dev = m.B, self.device
        tab = torch.as_tensor(table).to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if tab.numel() != B * self.R:
            raise ValueError(f"imitation_step: a table of {tab.numel()} values for a batch of {B} x {self.R} ReLU nodes")
        rows = torch.arange(B, dtype=torch.int32, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        report = torch.empty(B, 4, dtype=torch.int32, device=dev)
        regret = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        batch, keep = make_batch(m.lbs, m.ubs, m.duals, m.prim, m.x_lp, m.mask, m.pw, m.pb)
        self.imitation_step_rows(batch, B, rows, tab, margin, loss, report, regret, status, apply)
        if int(status.cpu()[0]) & 8:
            raise IndexError("imitation_step: a table row names a candidate that is no undecided ReLU of its mask, or holds an infinite entry")
        return loss.cpu().numpy(), report.cpu().numpy(), regret.cpu().numpy()

    def imitation_loss(self, scores, mask, table, margin=1.0, ds=None, loss=None, report=None, regret=None, status=None):
        """gnnb_imitation_loss on the current stream: the loss rule alone on caller-owned device tensors (an inspection hook).  scores,
        mask (n, R) fp32; table (n, R) fp64; ds None (a zeroed one is made) or (n, R) fp32, which receives d loss / d scores on top of
        what it holds; loss (n,) fp32, report (n, 4) int32, regret (n,) fp64, status (1,) int32: None (made here, status zeroed) or
        given.  Needs a bound network and no trainer.  Returns (loss, ds, report, regret, status) as device tensors; no synchronisation."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        margin = self._margin(margin, "imitation_loss")
        R, dev, i32, f32, f64 = self.R, self.device, torch.int32, torch.float32, torch.float64
        if not torch.is_tensor(scores) or scores.numel() % R or scores.numel() == 0:
            raise ValueError(f"imitation_loss: scores must hold n x {R} values")
        n = scores.numel() // R
        ds = torch.zeros(n, R, dtype=f32, device=dev) if ds is None else ds
        loss = torch.empty(n, dtype=f32, device=dev) if loss is None else loss
        report = torch.empty(n, 4, dtype=i32, device=dev) if report is None else report
        regret = torch.empty(n, dtype=f64, device=dev) if regret is None else regret
        status = torch.zeros(1, dtype=i32, device=dev) if status is None else status
        self._call("gnnb_imitation_loss", self._rows(scores, n, R, f32, "scores").data_ptr(), self._rows(mask, n, R, f32, "mask").data_ptr(),
                   self._rows(table, n, R, f64, "table").data_ptr(), n, margin, self._rows(loss, n, 1, f32, "loss").data_ptr(),
                   self._rows(ds, n, R, f32, "ds").data_ptr(), self._rows(report, n, 4, i32, "report").data_ptr(),
                   self._rows(regret, n, 1, f64, "regret").data_ptr(), self._rows(status, 1, 1, i32, "status").data_ptr())
        return loss, ds, report, regret, status

    # ---- the replay buffer (frontier.ReplayBuffer owns the tensors) ----------
    def replay_bytes(self, capacity):
        """gnnb_replay_bytes: the bytes of a buffer's batch tensors and table for ``capacity`` slots on the bound network (0: no network
        bound, or a capacity outside 1..65536)."""
        return int(self.lib.gnnb_replay_bytes(self.h, int(capacity)))

    def replay_push(self, src, K, rows, n, table, dst, capacity, dst_table, state, status=None):
        """gnnb_replay_push on the current stream: the useful ones of the rows ``rows[:n]`` ((n,) int32 device tensor, list order) of the
        K-row device batch ``src`` (a ``_lib.Batch``) and its (K, R) fp64 ``table`` go into the ring of ``capacity`` rows ``dst`` (a
        ``_lib.Batch`` over the buffer's tensors) and ``dst_table`` ((capacity, R) fp64); ``state``: the buffer's (4,) int32 word; status:
        None, or a (1,) int32 device tensor whose bit 3 reports a refused row.  Device work only; needs no trainer."""
        n, K, cap, i32, f64 = int(n), int(K), int(capacity), torch.int32, torch.float64
        self._call("gnnb_replay_push", C.byref(src), K, self._rows(table, max(K, 0), self.R, f64, "table").data_ptr(),
                   self._rows(rows, max(n, 0), 1, i32, "rows").data_ptr(), n, C.byref(dst), cap,
                   self._rows(dst_table, max(cap, 0), self.R, f64, "dst_table").data_ptr(), self._rows(state, 4, 1, i32, "state").data_ptr(),
                   None if status is None else self._rows(status, 1, 1, i32, "status").data_ptr())

    def replay_sample(self, state, capacity, n, seed, draw, idx):
        """gnnb_replay_sample on the current stream: ``idx[:n]`` ((n,) int32 device tensor) receives min(n, filled) distinct slots of the
        filled part of a buffer of ``capacity`` slots -- ``filled`` is read from ``state`` on the device -- and -1 beyond; a pure function
        of (filled, n, seed, draw) (include/gnnb.h states the keys).  Device work only."""
        n, i32 = int(n), torch.int32
        self._call("gnnb_replay_sample", self._rows(state, 4, 1, i32, "state").data_ptr(), int(capacity), n, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                   C.c_uint64(int(draw) & (2 ** 64 - 1)), self._rows(idx, max(n, 0), 1, i32, "idx").data_ptr())

    def online_grad(self):
        """d loss / d parameters of the last online_step or imitation step, flat float32 array in checkpoint order."""
        out = np.empty(GNN_BLOB_FLOATS, dtype=np.float32)
        with torch.cuda.device(self.device):                      # (in repack mode "device" it synchronises the device first)
            _lib.check(self.lib.gnnb_online_grad(self.h, out.ctypes.data_as(C.c_void_p), out.size), "gnnb_online_grad")
        return out

    # ---- BaBSR fallback scorer -------------------------------------------------
    def babsr(self, lower_bounds_all, upper_bounds_all, layers, masks):
        """kw_score_conv.py choose_node_conv :41-113 for a batch: same bounds / layers / masks arguments as
        ``forward``; returns a BabsrResult (device tensors, no synchronisation)."""
        fixed = layers["fixed_layers"]
        self.bind(fixed, tuple(lower_bounds_all[0].shape[1:]))
        B = batch_size(lower_bounds_all[0], layers["prop_layers"])
        lbs, ubs, mask = [self._dev(t) for t in lower_bounds_all], [self._dev(t) for t in upper_bounds_all], self._dev(masks)
        check_batch(self.sizes, self.R, fixed, B, lbs, ubs, mask=mask)
        pw, _ = self._prop(layers["prop_layers"])
        scores = torch.empty(B, self.R, dtype=torch.float32, device=self.device)
        icp = torch.empty(B, self.R, dtype=torch.float32, device=self.device)
        self._call("gnnb_babsr", table(lbs), table(ubs), len(lbs), pw.data_ptr(), mask.data_ptr(), B, scores.data_ptr(), icp.data_ptr())
        return BabsrResult(scores, icp, mask.view(B, self.R), self.sizes[1:-1])

    # ---- Wong-Kolter intermediate bounds (lp_producer.LayerGraphLP.kw_bounds for a batch) ------------------------------------
    def _domains(self, fixed_layers, prop_layers, x_lo, x_hi, masks):
        """What kw_bounds and dual_ascent share: bind the network (the input shape is read from the box) and bring a batch of domains to
        the device.  Returns (B, x_lo, x_hi as (B, N_0) fp64, the (B, R) int8 mask, property weights, property biases)."""
        B = int(x_lo.shape[0])
        if fixed_layers and type(fixed_layers[0]) is nn.Conv2d and (x_lo.dim() != 4 or x_hi.dim() != 4):
            raise ValueError(f"the first layer is a Conv2d: x_lo / x_hi must be (B, C, H, W) boxes, got {tuple(x_lo.shape)} / {tuple(x_hi.shape)}")
        self.bind(fixed_layers, tuple(x_lo.shape[1:]))
        batch_size(x_lo, prop_layers)
        xl, xu = f64(x_lo, B, self.sizes[0], "x_lo", self.device), f64(x_hi, B, self.sizes[0], "x_hi", self.device)
        mask = torch.as_tensor(masks).to(device=self.device, dtype=torch.int8).contiguous()
        if mask.numel() != B * self.R:
            raise ValueError(f"masks has {tuple(mask.shape)}, expected ({B}, {self.R})")
        return (B, xl, xu, mask) + self._prop(prop_layers)

    def kw_tighten_workspace(self, B):
        return self._workspace("kw_tighten", B, "gnnb_kw_tighten_workspace_bytes")

    def kw_bounds(self, fixed_layers, prop_layers, x_lo, x_hi, masks, parents=None, split_layers=None, want_fp32=False, tighten=0, lr=0.1):
        """gnnb_kw_bounds on the current stream; with ``tighten`` = n > 0 gnnb_kw_tighten: the bounds of the ambiguous nodes of graph layers
        2..L tightened by n steps (``lr``) of dual ascent per node, and ``KwBoundsResult.counts`` (B, 2) int32: the nodes it ran for / decided.  x_lo / x_hi: (B, C, H, W) input boxes (fp64 on the device), or (B, N_0) when the first
        layer is not a Conv2d (the input shape is read from the box); prop_layers: B Linear(N_L, 1); masks: (B, R) in {-1, 0, 1}, flat
        ReLU order; parents: None or (lbs, ubs), each n_graph-1 tensors (B, N_k) of graph layers 1..L+1 (fp64); split_layers: (B,) ReLU
        layer of each domain's split, -1 = no parent.  Returns a KwBoundsResult."""
        B, xl, xu, mask, pw, pb = self._domains(fixed_layers, prop_layers, x_lo, x_hi, masks)
        ng, dev = len(self.sizes), self.device
        plb = pub = split = None
        if parents is not None:
            if split_layers is None or len(parents[0]) != ng - 1 or len(parents[1]) != ng - 1:
                raise ValueError("parents need n_graph-1 lower and upper tensors and split_layers")
            plb = [f64(t, B, self.sizes[k + 1], f"parent lb {k + 1}", dev) for k, t in enumerate(parents[0])]
            pub = [f64(t, B, self.sizes[k + 1], f"parent ub {k + 1}", dev) for k, t in enumerate(parents[1])]
            split = torch.as_tensor(split_layers).to(device=dev, dtype=torch.int32).contiguous()
            if split.numel() != B:
                raise ValueError("split_layers must hold one entry per domain")
        lb = [torch.empty(B, n, dtype=torch.float64, device=dev) for n in self.sizes[1:]]
        ub = [torch.empty(B, n, dtype=torch.float64, device=dev) for n in self.sizes[1:]]
        lb32 = ub32 = None
        if want_fp32:
            shapes = [tuple(x_lo.shape)] + [(B, n) for n in self.sizes[1:]]      # the box keeps its shape: bind() reads the input's from it
            lb32 = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes]
            ub32 = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes]
        infeasible = torch.empty(B, dtype=torch.int32, device=dev)
        ws = self.kw_workspace(B)
        kb = _lib.KwBatch(xl.data_ptr(), xu.data_ptr(), pw.data_ptr(), pb.data_ptr(), mask.data_ptr(), table(plb), table(pub), ptr(split), ng)
        if tighten < 0:
            raise ValueError(f"tighten = {tighten} < 0")
        if tighten > 0:
            counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
            tws = self.kw_tighten_workspace(B)
            self._call("gnnb_kw_tighten", C.byref(kb), B, int(tighten), float(lr), table(lb), table(ub), table(lb32), table(ub32), infeasible.data_ptr(),
                       counts.data_ptr(), ws.data_ptr(), ws.numel(), tws.data_ptr(), tws.numel())
            return KwBoundsResult(lb, ub, lb32, ub32, infeasible, counts)
        self._call("gnnb_kw_bounds", C.byref(kb), B, table(lb), table(ub), table(lb32), table(ub32), infeasible.data_ptr(), ws.data_ptr(), ws.numel())
        return KwBoundsResult(lb, ub, lb32, ub32, infeasible)

    # ---- dual ascent on the subproblem LPs (lp_producer.LayerGraphLP.dual_ascent_host for a batch) --------------------------------
    def dual_ascent(self, fixed_layers, prop_layers, x_lo, x_hi, masks, lb, ub, n_iter, lr=0.1, alpha=None, beta=None, want_grad=False,
                    want_scorer_inputs=False, lb32_prop=None, workspace=None):
        """gnnb_dual_ascent on the current stream: ``n_iter`` steps of projected Adam on the dual of every domain's LP relaxation, the
        intermediate bounds fixed.  x_lo / x_hi / prop_layers / masks: as ``kw_bounds`` takes them; lb / ub: n_graph-1 fp64 tensors
        (B, N_k) of graph layers 1..L+1, mask applied (``KwBoundsResult.lb`` / ``.ub``).  alpha / beta: None (start at u / (u - l) and 0)
        or (B, R) fp64 to start from (copied).  lb32_prop: None, or a (B,) / (B, 1) fp32 device tensor that receives the bound (the
        property entry of ``KwBoundsResult.lb32``).  workspace: None (the engine's own), or a device uint8 tensor.  Returns a DualAscentResult."""
        if (alpha is None) != (beta is None):
            raise ValueError("alpha and beta go together")
        B, xl, xu, mask, pw, pb = self._domains(fixed_layers, prop_layers, x_lo, x_hi, masks)
        ng, dev, R = len(self.sizes), self.device, self.R
        if len(lb) != ng - 1 or len(ub) != ng - 1:
            raise ValueError(f"{len(lb)} / {len(ub)} bound tensors, expected {ng - 1} (graph layers 1..L+1)")
        lbs = [f64(t, B, self.sizes[k + 1], f"lb {k + 1}", dev) for k, t in enumerate(lb)]
        ubs = [f64(t, B, self.sizes[k + 1], f"ub {k + 1}", dev) for k, t in enumerate(ub)]
        warm = alpha is not None
        al = f64(alpha, B, R, "alpha", dev).clone() if warm else torch.empty(B, R, dtype=torch.float64, device=dev)
        be = f64(beta, B, R, "beta", dev).clone() if warm else torch.empty(B, R, dtype=torch.float64, device=dev)
        bound = torch.empty(B, dtype=torch.float64, device=dev)
        ga = gb = None
        if want_grad:
            ga, gb = torch.empty_like(al), torch.empty_like(al)
        duals = prims = x_lp = None
        if want_scorer_inputs:
            duals = [torch.empty(B * n, 3, dtype=torch.float32, device=dev) for n in self.sizes[1:-1]]
            prims, k = [], 0
            for q, l in enumerate(fixed_layers):                  # primals[q]: the output of network layer q
                nxt = fixed_layers[q + 1] if q + 1 < len(fixed_layers) else None
                if type(l) is nn.ReLU or type(nxt) is nn.ReLU:
                    k += type(nxt) is nn.ReLU
                    prims.append(torch.empty(B * self.sizes[k], dtype=torch.float32, device=dev))
                else:                                             # (gnnb_forward never reads it)
                    prims.append(torch.zeros(1, dtype=torch.float32, device=dev))
            prims.append(torch.empty(B, dtype=torch.float32, device=dev))
            x_lp = torch.empty(tuple(x_lo.shape), dtype=torch.float32, device=dev)
        if lb32_prop is not None and (lb32_prop.numel() != B or lb32_prop.dtype != torch.float32 or lb32_prop.device != dev
                                      or not lb32_prop.is_contiguous()):
            raise ValueError("lb32_prop must be a contiguous device fp32 tensor of B values")
        ws = self.dual_workspace(B) if workspace is None else workspace
        db = _lib.DualBatch(table(lbs), table(ubs), xl.data_ptr(), xu.data_ptr(), pw.data_ptr(), pb.data_ptr(), mask.data_ptr(), ng)
        self._call("gnnb_dual_ascent", C.byref(db), B, int(n_iter), float(lr), al.data_ptr(), be.data_ptr(), int(warm), bound.data_ptr(), ptr(ga),
                   ptr(gb), table(duals), table(prims), ptr(x_lp), ptr(lb32_prop), ws.data_ptr(), ws.numel())
        return DualAscentResult(bound, al, be, ga, gb, duals, prims, x_lp)

    # ---- the real network at a batch of points, fp64 (the BaB loop's upper bound at the LP's input point) ---------------------------
    def net_eval(self, fixed_layers, prop_layers, x, out=None, prop=None, workspace=None):
        """gnnb_net_eval on the current stream.  x: (B, C, H, W) (or (B, N_0)) points, fp32 on the device (``DualAscentResult.x_lp``);
        prop_layers: B Linear(N_L, 1), or ``prop`` = (weights (B, N_L), biases (B,)) fp32 device tensors.  Returns the (B,) fp64 values of
        property layer b on the network's output at point b (``out``: a tensor to write them to).  Nothing is synchronised."""
        B = int(x.shape[0])
        self.bind(fixed_layers, tuple(x.shape[1:]))
        x = self._rows(x, B, self.sizes[0], torch.float32, "x")
        pw, pb = self._prop(prop_layers) if prop is None else prop
        pw, pb = self._rows(pw, B, self.sizes[-2], torch.float32, "property weights"), self._rows(pb, B, 1, torch.float32, "property biases")
        out = torch.empty(B, dtype=torch.float64, device=self.device) if out is None else self._rows(out, B, 1, torch.float64, "out")
        ws = self._workspace("net_eval", B, "gnnb_net_eval_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_net_eval", x.data_ptr(), pw.data_ptr(), pb.data_ptr(), B, out.data_ptr(), ws.data_ptr(), ws.numel())
        return out.reshape(-1)[:B]

    def net_descend(self, fixed_layers, prop_layers, x0, x_lo, x_hi, n_steps, step=1.0 / 64, x_best=None, value=None, want_grad=False,
                    want_steps=False, prop=None, workspace=None):
        """gnnb_net_descend on the current stream: up to ``n_steps`` projected signed-gradient steps of ``step``
        times the box's width on the bound network followed by property row b, from each of the B points x0 ((B, C, H, W) or (B, N_0)
        fp32 on the device) inside [x_lo, x_hi] ((B, N_0) fp64 device tensors).  prop_layers / prop: as ``net_eval``.  x_best (B, N_0)
        fp32 and value (B,) fp64: tensors to write to (None: new ones; x_best must not be x0).  Returns (x_best, value, grad0, steps):
        the best point seen, the network's value there (``net_eval``'s, bit for bit), the gradient at x0 ((B, N_0) fp64) with
        ``want_grad`` and the number of steps evaluated ((B,) int32) with ``want_steps``, else None.  Nothing is synchronised."""
        B = int(x0.shape[0])
        self.bind(fixed_layers, tuple(x0.shape[1:]))
        N0, f64, f32 = self.sizes[0], torch.float64, torch.float32
        x0 = self._rows(x0, B, N0, f32, "x0")
        pw, pb = self._prop(prop_layers) if prop is None else prop
        pw, pb = self._rows(pw, B, self.sizes[-2], f32, "property weights"), self._rows(pb, B, 1, f32, "property biases")
        x_best = torch.empty(B, N0, dtype=f32, device=self.device) if x_best is None else self._rows(x_best, B, N0, f32, "x_best")
        value = torch.empty(B, dtype=f64, device=self.device) if value is None else self._rows(value, B, 1, f64, "value")
        grad0 = torch.empty(B, N0, dtype=f64, device=self.device) if want_grad else None
        steps = torch.empty(B, dtype=torch.int32, device=self.device) if want_steps else None
        ws = self._workspace("net_descend", B, "gnnb_net_descend_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_net_descend", x0.data_ptr(), self._rows(x_lo, B, N0, f64, "x_lo").data_ptr(), self._rows(x_hi, B, N0, f64, "x_hi").data_ptr(),
                   pw.data_ptr(), pb.data_ptr(), B, int(n_steps), float(step), x_best.data_ptr(), value.data_ptr(), ptr(grad0), ptr(steps),
                   ws.data_ptr(), ws.numel())
        return x_best, value, grad0, steps

    def net_starts(self, fixed_layers, x0, x_lo, x_hi, n_random, seed=0, starts=None):
        """gnnb_net_starts on the current stream: the start points of B rows, (B, n_random + 1, N_0) fp32.  Slot 0
        of row b is x0[b] ((B, C, H, W) or (B, N_0) fp32 on the device); slot r >= 1 is a counter-based uniform point of the row's box
        [x_lo, x_hi] ((B, N_0) fp64 device tensors) that depends on the row's own x0, box and ``seed`` (0..2^64 - 1) only.  starts: a tensor
        to write to (None: a new one).  Nothing is synchronised."""
        B, R = int(x0.shape[0]), int(n_random)
        self.bind(fixed_layers, tuple(x0.shape[1:]))
        N0, f64, f32 = self.sizes[0], torch.float64, torch.float32
        x0 = self._rows(x0, B, N0, f32, "x0")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed = {seed!r}: an integer in 0..2^64 - 1")
        n = max(R, 0) + 1
        starts = torch.empty(B, n, N0, dtype=f32, device=self.device) if starts is None else self._rows(starts, B, n * N0, f32, "starts")
        self._call("gnnb_net_starts", x0.data_ptr(), self._rows(x_lo, B, N0, f64, "x_lo").data_ptr(), self._rows(x_hi, B, N0, f64, "x_hi").data_ptr(),
                   B, R, seed, starts.data_ptr())
        return starts

    def net_descend_starts(self, fixed_layers, prop_layers, starts, x_lo, x_hi, n_steps, step=1.0 / 64, x_best=None, value=None,
                           want_index=False, want_values=False, want_steps=False, prop=None, workspace=None, in_shape=None):
        """gnnb_net_descend_starts on the current stream: ``net_descend``'s rule from every one of the n_starts
        start points of every row -- starts: (B, n_starts, N_0) fp32 on the device, row b's inside [x_lo[b], x_hi[b]] ((B, N_0) fp64)
        under property row b (prop_layers / prop: as ``net_eval``) -- and per row the minimum of the starts' best values in the order
        (value, start index), a NaN never winning.  x_best (B, N_0) fp32 and value (B,) fp64: tensors to write to (None: new ones; x_best
        must not be starts).  Returns (x_best, value, index, values, steps): the winner's point and value (``net_eval``'s, bit for bit),
        its slot ((B,) int32) with ``want_index``, every start's best value ((B, n_starts) fp64) with ``want_values`` and steps evaluated
        ((B, n_starts) int32) with ``want_steps``, else None.  in_shape: the network's input shape (None: the one the engine is bound
        with, ``net_starts``' for instance).  Nothing is synchronised."""
        if not torch.is_tensor(starts) or starts.dim() != 3:
            raise ValueError("starts: expected a (B, n_starts, N_0) tensor")
        B, n = int(starts.shape[0]), int(starts.shape[1])
        if in_shape is None:                                      # (the start points are flat: the shape comes from the bind before, net_starts' say)
            if self._net_key is None:
                raise ValueError("in_shape: the network's input shape is needed to bind it")
            in_shape = self._net_key[2]
        self.bind(fixed_layers, tuple(in_shape))
        N0, f64, f32, i32 = self.sizes[0], torch.float64, torch.float32, torch.int32
        starts = self._rows(starts, B, n * N0, f32, "starts")
        pw, pb = self._prop(prop_layers) if prop is None else prop
        pw, pb = self._rows(pw, B, self.sizes[-2], f32, "property weights"), self._rows(pb, B, 1, f32, "property biases")
        x_best = torch.empty(B, N0, dtype=f32, device=self.device) if x_best is None else self._rows(x_best, B, N0, f32, "x_best")
        value = torch.empty(B, dtype=f64, device=self.device) if value is None else self._rows(value, B, 1, f64, "value")
        index = torch.empty(B, dtype=i32, device=self.device) if want_index else None
        values = torch.empty(B, n, dtype=f64, device=self.device) if want_values else None
        steps = torch.empty(B, n, dtype=i32, device=self.device) if want_steps else None
        if workspace is None:
            workspace = self._starts_workspace(B, n)
        self._call("gnnb_net_descend_starts", starts.data_ptr(), n, self._rows(x_lo, B, N0, f64, "x_lo").data_ptr(),
                   self._rows(x_hi, B, N0, f64, "x_hi").data_ptr(), pw.data_ptr(), pb.data_ptr(), B, int(n_steps), float(step), x_best.data_ptr(),
                   value.data_ptr(), ptr(index), ptr(values), ptr(steps), workspace.data_ptr(), workspace.numel())
        return x_best, value, index, values, steps

    def _starts_workspace(self, B, n_starts):
        """The engine's own workspace of ``net_descend_starts``, grown on demand."""
        need = max(1, self.lib.gnnb_net_descend_starts_workspace_bytes(self.h, B, n_starts))
        ws = getattr(self, "_ws_starts", None)
        if ws is None or ws.numel() < need:
            ws = self._ws_starts = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    # ---- a BaB frontier in device memory (frontier.py runs the loop; include/gnnb.h gnnb_frontier_*) ---------------------------------
    def _rows(self, t, n, cols, dtype, what):
        """t as it is, checked: a contiguous device tensor of ``dtype`` holding at least n rows of ``cols`` (the steps below copy nothing)."""
        if not torch.is_tensor(t) or t.dtype != dtype or t.device != self.device or not t.is_contiguous() or t.numel() < n * cols:
            raise ValueError(f"{what}: expected a contiguous {dtype} tensor on {self.device} with at least {n}x{cols} values")
        return t

    def _layer_rows(self, ts, n, first, dtype, what):
        sizes = self.sizes[first:]
        if len(ts) != len(sizes):
            raise ValueError(f"{what}: {len(ts)} tensors, expected {len(sizes)} (graph layers {first}..L+1)")
        return table([self._rows(t, n, s, dtype, f"{what}[{k}]") for k, (t, s) in enumerate(zip(ts, sizes))])

    def _pool(self, pool):
        """The gnnb_pool of a ``frontier.DomainPool`` (any object with its attributes) and what must outlive the call."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        cap, R = int(pool.capacity), self.R
        tl, tu = self._layer_rows(pool.lb, cap, 1, torch.float64, "pool.lb"), self._layer_rows(pool.ub, cap, 1, torch.float64, "pool.ub")
        st = _lib.Pool(self._rows(pool.mask, cap, R, torch.int8, "pool.mask").data_ptr(), tl, tu,
                       self._rows(pool.alpha, cap, R, torch.float64, "pool.alpha").data_ptr(),
                       self._rows(pool.beta, cap, R, torch.float64, "pool.beta").data_ptr(),
                       self._rows(pool.bound, cap, 1, torch.float64, "pool.bound").data_ptr(),
                       self._rows(pool.open, cap, 1, torch.int32, "pool.open").data_ptr(), cap, len(self.sizes))
        return st, (tl, tu)

    def frontier_gather(self, pool, slots, x_lo, x_hi, mask, lb, ub, lb32, ub32, alpha, beta, scorer_mask):
        """gnnb_frontier_gather on the current stream: the pool rows of ``slots`` ((K,) int32, distinct) into row i of the given tensors:
        mask (K, R) int8, lb / ub (graph layers 1..L+1, fp64), lb32 / ub32 (graph layers 0..L+1, fp32, layer 0 from x_lo / x_hi (K, N_0)
        fp64), alpha / beta (K, R) fp64, scorer_mask (K, R) fp32.  Every tensor is a device tensor of the caller's; nothing is copied."""
        K = int(slots.numel())
        st, keep = self._pool(pool)
        R, N0 = self.R, self.sizes[0]
        args = (self._rows(slots, K, 1, torch.int32, "slots").data_ptr(), K, self._rows(x_lo, K, N0, torch.float64, "x_lo").data_ptr(),
                self._rows(x_hi, K, N0, torch.float64, "x_hi").data_ptr(), self._rows(mask, K, R, torch.int8, "mask").data_ptr(),
                self._layer_rows(lb, K, 1, torch.float64, "lb"), self._layer_rows(ub, K, 1, torch.float64, "ub"),
                self._layer_rows(lb32, K, 0, torch.float32, "lb32"), self._layer_rows(ub32, K, 0, torch.float32, "ub32"),
                self._rows(alpha, K, R, torch.float64, "alpha").data_ptr(), self._rows(beta, K, R, torch.float64, "beta").data_ptr(),
                self._rows(scorer_mask, K, R, torch.float32, "scorer_mask").data_ptr())
        self._call("gnnb_frontier_gather", C.byref(st), *args)

    def frontier_expand(self, pool, slots, decisions, mask, parent_lb, parent_ub, split_layer, alpha, beta, live):
        """gnnb_frontier_expand on the current stream: the 2K children of the parents in ``slots`` split at ``decisions`` ((K, 2) int32,
        ``ForwardResult.decisions``), rows 2i (blocked) and 2i + 1 (passing) of mask (2K, R) int8, parent_lb / parent_ub (graph layers
        1..L+1, fp64), split_layer (2K,) int32, alpha / beta (2K, R) fp64, live (2K,) int32 -- the inputs of ``kw_bounds`` / ``dual_ascent``."""
        K = int(slots.numel())
        st, keep = self._pool(pool)
        R = self.R
        args = (self._rows(slots, K, 1, torch.int32, "slots").data_ptr(), self._rows(decisions, K, 2, torch.int32, "decisions").data_ptr(), K,
                self._rows(mask, 2 * K, R, torch.int8, "mask").data_ptr(), self._layer_rows(parent_lb, 2 * K, 1, torch.float64, "parent_lb"),
                self._layer_rows(parent_ub, 2 * K, 1, torch.float64, "parent_ub"),
                self._rows(split_layer, 2 * K, 1, torch.int32, "split_layer").data_ptr(),
                self._rows(alpha, 2 * K, R, torch.float64, "alpha").data_ptr(), self._rows(beta, 2 * K, R, torch.float64, "beta").data_ptr(),
                self._rows(live, 2 * K, 1, torch.int32, "live").data_ptr())
        self._call("gnnb_frontier_expand", C.byref(st), *args)

    def frontier_commit(self, pool, slots, mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live, state, eps=1e-4, decision_bound=None,
                        workspace=None):
        """gnnb_frontier_commit on the current stream: resolve, keep or close the 2K children of the parents in ``slots``, store the kept
        ones in the pool and update ``state`` (``_lib.FRONTIER_STATE_DOUBLES`` device doubles, indices ``_lib.FS_*``).  mask / live: what
        ``frontier_expand`` wrote; lb / ub / infeasible: ``kw_bounds``'; bound / alpha / beta: ``dual_ascent``'s; ub_value: ``net_eval``'s."""
        K = int(slots.numel())
        st, keep = self._pool(pool)
        ch, keep_ch = self._children(_ChildRows(mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live), 2 * K)
        self._rows(state, _lib.FRONTIER_STATE_DOUBLES, 1, torch.float64, "state")
        ws = self._workspace("commit", K, "gnnb_frontier_commit_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_commit", C.byref(st), self._rows(slots, K, 1, torch.int32, "slots").data_ptr(), K, C.byref(ch), float(eps),
                   float("nan") if decision_bound is None else float(decision_bound), state.data_ptr(), ws.data_ptr(), ws.numel())

    def frontier_expand_depth(self, pool, slots, depth, cand0, cand_dec, mask, parent_lb, parent_ub, split_layer, alpha, beta, live):
        """gnnb_frontier_expand_depth on the current stream: C = 2^depth child rows per parent in ``slots`` from
        the candidate lists ``strong_list`` wrote (cand0 (K + 1,) int32, cand_dec (n, 2) int32 with n = cand0[K], read on the device).
        Parent i with m listed nodes gets live rows C i + j, j < 2^m, its mask with the b-th listed node set to bit b of j; its other
        rows, and every row of a parent with 0 or more than ``depth`` nodes, are dead rows with the parent's mask.  The outputs are
        ``frontier_expand``'s with K * C rows.  Nothing is copied."""
        K, depth = int(slots.numel()), int(depth)
        st, keep = self._pool(pool)
        R, n, i32, f64 = self.R, max(K, 0) << min(max(depth, 0), 8), torch.int32, torch.float64
        args = (self._rows(slots, K, 1, i32, "slots").data_ptr(), K, depth, self._rows(cand0, K + 1, 1, i32, "cand0").data_ptr(),
                self._rows(cand_dec, 1, 2, i32, "cand_dec").data_ptr(), self._rows(mask, n, R, torch.int8, "mask").data_ptr(),
                self._layer_rows(parent_lb, n, 1, f64, "parent_lb"), self._layer_rows(parent_ub, n, 1, f64, "parent_ub"),
                self._rows(split_layer, n, 1, i32, "split_layer").data_ptr(), self._rows(alpha, n, R, f64, "alpha").data_ptr(),
                self._rows(beta, n, R, f64, "beta").data_ptr(), self._rows(live, n, 1, i32, "live").data_ptr())
        self._call("gnnb_frontier_expand_depth", C.byref(st), *args)

    def frontier_commit_depth(self, pool, slots, depth, mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live, state, eps=1e-4,
                              decision_bound=None, workspace=None):
        """gnnb_frontier_commit_depth on the current stream: ``frontier_commit``'s rule on the K * 2^depth child
        rows ``frontier_expand_depth`` laid out; a kept child of rank r goes to slots[r] for r < K, else to slot in_use + (r - K)."""
        K, depth = int(slots.numel()), int(depth)
        st, keep = self._pool(pool)
        n = max(K, 0) << min(max(depth, 0), 8)
        ch, keep_ch = self._children(_ChildRows(mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live), n)
        self._rows(state, _lib.FRONTIER_STATE_DOUBLES, 1, torch.float64, "state")
        if workspace is None:
            need = self.lib.gnnb_frontier_commit_depth_workspace_bytes(self.h, K, depth)
            workspace = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        self._call("gnnb_frontier_commit_depth", C.byref(st), self._rows(slots, K, 1, torch.int32, "slots").data_ptr(), K, depth, C.byref(ch),
                   float(eps), float("nan") if decision_bound is None else float(decision_bound), state.data_ptr(), workspace.data_ptr(),
                   workspace.numel())

    def babsr_rows(self, lb32, ub32, prop_w, scorer_mask, B, scores, intercepts):
        """gnnb_babsr on the current stream over the first B of the parent rows ``frontier_gather`` wrote (lb32 / ub32: graph layers
        0..L+1 fp32; prop_w (B, N_L) fp32; scorer_mask (B, R) fp32) into scores / intercepts (B, R) fp32.  Nothing is copied."""
        R = self.R
        tl, tu = self._layer_rows(lb32, B, 0, torch.float32, "lb32"), self._layer_rows(ub32, B, 0, torch.float32, "ub32")
        self._call("gnnb_babsr", tl, tu, len(self.sizes), self._rows(prop_w, B, self.sizes[-2], torch.float32, "prop_w").data_ptr(),
                   self._rows(scorer_mask, B, R, torch.float32, "scorer_mask").data_ptr(), B,
                   self._rows(scores, B, R, torch.float32, "scores").data_ptr(), self._rows(intercepts, B, R, torch.float32, "intercepts").data_ptr())

    def _fallback(self, K, S, live, infeasible, bound, scores, intercepts, scorer_mask, icp, ineff, branching_threshold, kwbd_threshold, sparsest_layer,
                  decision_threshold, random_order):
        """The gnnb_fallback of K parent rows whose counters and tables are S rows long (1: one job; the segments of a plan), and what must
        outlive the call."""
        from .lp_producer import _random_order
        R, i32 = self.R, torch.int32
        order = list(_random_order(len(self.sizes) - 2, sparsest_layer) if random_order is None else random_order)
        order_c = (C.c_int32 * max(1, len(order)))(*order)
        fb = _lib.Fallback(self._rows(live, 2 * K, 1, i32, "live").data_ptr(), self._rows(infeasible, 2 * K, 1, i32, "infeasible").data_ptr(),
                           self._rows(bound, 2 * K, 1, torch.float64, "bound").data_ptr(), self._rows(scores, K, R, torch.float32, "scores").data_ptr(),
                           self._rows(intercepts, K, R, torch.float32, "intercepts").data_ptr(),
                           self._rows(scorer_mask, K, R, torch.float32, "scorer_mask").data_ptr(), float(branching_threshold), float(decision_threshold),
                           int(kwbd_threshold), int(sparsest_layer), order_c, len(order), self._rows(icp, S, 1, i32, "icp").data_ptr(),
                           self._rows(ineff, S, R, i32, "ineff").data_ptr())
        return fb, order_c

    def frontier_fallback(self, pool, slots, live, infeasible, bound, scores, intercepts, scorer_mask, icp, ineff, gnn_improvement, kw_decisions,
                          sel_rows, sel_slots, sel_decisions, m, branching_threshold, kwbd_threshold=10, sparsest_layer=0, decision_threshold=0.001,
                          random_order=None, workspace=None):
        """gnnb_frontier_fallback on the current stream: for the K parents in ``slots`` whose GNN children (pair A:
        live / infeasible / bound, 2K rows) are bounded, the GNN's improvement of the bound into gnn_improvement (K,) fp64, the BaBSR
        decision of every parent below ``branching_threshold`` into kw_decisions (K, 2) int32 ([-1, -1]: none), and the parents whose KW
        point was inefficient fewer than ``kwbd_threshold`` times as a dense list in row order: sel_rows / sel_slots (K,), sel_decisions
        (K, 2), their number m (1,), all int32.  scores / intercepts: ``babsr_rows`` on the parents' rows; icp (1,) int32 the run's
        intercept counter (read and updated), ineff (R,) int32 the counts of inefficient KW points (read).  random_order: the ReLU layers
        popped from the end (None: ``lp_producer._random_order``)."""
        K = int(slots.numel())
        st, keep = self._pool(pool)
        i32 = torch.int32
        fb, keep_fb = self._fallback(K, 1, live, infeasible, bound, scores, intercepts, scorer_mask, icp, ineff, branching_threshold, kwbd_threshold,
                                     sparsest_layer, decision_threshold, random_order)
        ws = self._workspace("fallback", K, "gnnb_frontier_fallback_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_fallback", C.byref(st), self._rows(slots, K, 1, i32, "slots").data_ptr(), K, C.byref(fb),
                   self._rows(gnn_improvement, K, 1, torch.float64, "gnn_improvement").data_ptr(),
                   self._rows(kw_decisions, K, 2, i32, "kw_decisions").data_ptr(), self._rows(sel_rows, K, 1, i32, "sel_rows").data_ptr(),
                   self._rows(sel_slots, K, 1, i32, "sel_slots").data_ptr(), self._rows(sel_decisions, K, 2, i32, "sel_decisions").data_ptr(),
                   self._rows(m, 1, 1, i32, "m").data_ptr(), ws.data_ptr(), ws.numel())

    def _babsr_rule(self, n, S, scores, intercepts, scorer_mask, icp, decisions, sparsest_layer, decision_threshold, random_order):
        """The arguments ``gnnb_frontier_babsr_decide`` and its jobs form share, for n parent rows and S counters, and what must outlive
        the call."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        from .lp_producer import _random_order
        R, i32, f32 = self.R, torch.int32, torch.float32
        order = list(_random_order(len(self.sizes) - 2, sparsest_layer) if random_order is None else random_order)
        order_c = (C.c_int32 * max(1, len(order)))(*order)
        args = (self._rows(scores, n, R, f32, "scores").data_ptr(), self._rows(intercepts, n, R, f32, "intercepts").data_ptr(),
                self._rows(scorer_mask, n, R, f32, "scorer_mask").data_ptr(), float(decision_threshold), int(sparsest_layer), order_c, len(order),
                self._rows(icp, S, 1, i32, "icp").data_ptr(), self._rows(decisions, n, 2, i32, "decisions").data_ptr())
        return args, order_c

    def frontier_babsr_decide(self, scores, intercepts, scorer_mask, icp, decisions, K=None, sparsest_layer=0, decision_threshold=0.001,
                              random_order=None, workspace=None):
        """gnnb_frontier_babsr_decide on the current stream: the BaBSR decision (``kw_score_conv.decide``) of
        each of the first K rows (None: every row of ``decisions``) of scores / intercepts (``babsr_rows``) and scorer_mask
        (``frontier_gather``), all (K, R) fp32, into decisions (K, 2) int32 ([-1, -1]: a NaN row, a row without an undecided node);
        icp (1,) int32, the run's intercept counter, is read and updated in row order.  random_order: the ReLU layers popped from the
        end (None: ``lp_producer._random_order``).  Nothing is copied."""
        K = int(decisions.numel()) // 2 if K is None else int(K)
        args, keep = self._babsr_rule(max(K, 0), 1, scores, intercepts, scorer_mask, icp, decisions, sparsest_layer, decision_threshold, random_order)
        ws = self._workspace("babsr_decide", K, "gnnb_frontier_babsr_decide_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_babsr_decide", K, *args, ws.data_ptr(), ws.numel())

    def frontier_babsr_decide_jobs(self, plan, scores, intercepts, scorer_mask, icp, decisions, sparsest_layer=0, decision_threshold=0.001,
                                   random_order=None, workspace=None):
        """gnnb_frontier_babsr_decide_jobs on the current stream: ``frontier_babsr_decide`` per plan entry on its rows of the (n, R) /
        (n, 2) tensors with its segment's counter icp[segment] ((segments,) int32).  A segment without an entry and rows from n on are
        not touched."""
        pl, n, S = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0)
        args, keep = self._babsr_rule(n, S, scores, intercepts, scorer_mask, icp, decisions, sparsest_layer, decision_threshold, random_order)
        ws = self._workspace("babsr_decide", max(n, 1), "gnnb_frontier_babsr_decide_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_babsr_decide_jobs", C.byref(pl), *args, ws.data_ptr(), ws.numel())

    def strong_list(self, pool, slots, scorer_mask, scores, top_m, cand0, cand_row, cand_slot, cand_dec, workspace=None):
        """gnnb_strong_list on the current stream: the candidate splits of the K parents in ``slots`` ((K,) int32)
        as dense lists in row order.  scorer_mask (K, R) fp32 (``frontier_gather``); top_m 0: every undecided node, scores None; top_m
        M > 0: the M first on (score descending, flat index ascending), scores (K, R) fp32 (``babsr_rows``).  cand0 (K + 1,) int32 receives
        the exclusive prefix of the rows' counts (cand0[K] = n), cand_row / cand_slot (n,) and cand_dec (n, 2) int32 the lists; they hold
        K * min(R, top_m or R) entries, and entries from n on are not written.  Nothing is copied."""
        K, top_m = int(slots.numel()), int(top_m)
        st, keep = self._pool(pool)
        R, i32, f32 = self.R, torch.int32, torch.float32
        cap = max(K, 0) * (min(R, top_m) if top_m > 0 else R)
        ws = self._workspace("strong_list", K, "gnnb_strong_list_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_strong_list", C.byref(st), self._rows(slots, K, 1, i32, "slots").data_ptr(), K,
                   self._rows(scorer_mask, K, R, f32, "scorer_mask").data_ptr(),
                   None if scores is None else self._rows(scores, K, R, f32, "scores").data_ptr(), top_m,
                   self._rows(cand0, K + 1, 1, i32, "cand0").data_ptr(), self._rows(cand_row, cap, 1, i32, "cand_row").data_ptr(),
                   self._rows(cand_slot, cap, 1, i32, "cand_slot").data_ptr(), self._rows(cand_dec, cap, 2, i32, "cand_dec").data_ptr(),
                   ws.data_ptr(), ws.numel())

    def strong_list_union(self, pool, slots, scorer_mask, scores_a, top_a, scores_b, top_b, cand0, cand_row, cand_slot, cand_dec, cand_src,
                          workspace=None):
        """gnnb_strong_list_union on the current stream: per parent the union of ``strong_list``'s candidates for
        (scores_a, top_a) and for (scores_b, top_b), each node once, in ascending flat index; both score arrays (K, R) fp32, both counts at
        least 1.  cand_src (n,) int32 receives 1 (in A's set only), 2 (in B's only) or 3 (in both); the other lists are ``strong_list``'s and
        hold K * min(R, top_a + top_b) entries; entries from n on are not written.  A NaN at an undecided node of either array empties the
        row.  Nothing is copied."""
        K, top_a, top_b = int(slots.numel()), int(top_a), int(top_b)
        st, keep = self._pool(pool)
        R, i32, f32 = self.R, torch.int32, torch.float32
        cap = max(K, 0) * min(R, max(top_a, 0) + max(top_b, 0))
        ws = self._workspace("strong_list_union", K, "gnnb_strong_list_union_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_strong_list_union", C.byref(st), self._rows(slots, K, 1, i32, "slots").data_ptr(), K,
                   self._rows(scorer_mask, K, R, f32, "scorer_mask").data_ptr(), self._rows(scores_a, K, R, f32, "scores_a").data_ptr(), top_a,
                   self._rows(scores_b, K, R, f32, "scores_b").data_ptr(), top_b, self._rows(cand0, K + 1, 1, i32, "cand0").data_ptr(),
                   self._rows(cand_row, cap, 1, i32, "cand_row").data_ptr(), self._rows(cand_slot, cap, 1, i32, "cand_slot").data_ptr(),
                   self._rows(cand_dec, cap, 2, i32, "cand_dec").data_ptr(), self._rows(cand_src, cap, 1, i32, "cand_src").data_ptr(),
                   ws.data_ptr(), ws.numel())

    def strong_pick(self, pool, slots, cand0, cand_dec, n, live, infeasible, bound, decisions, best_improvement, improvement, table=None):
        """gnnb_strong_pick on the current stream: the improvement of each of the n listed candidates from its two
        bounded child rows (live / infeasible (2n,) int32, bound (2n,) fp64, list order) into improvement (n,) fp64, and per parent row
        the arg-max into decisions (K, 2) int32 ([-1, -1]: none) and best_improvement (K,) fp64 (NaN: none); table: None, or (K, R) fp64
        that receives imp at every candidate's flat index and NaN elsewhere.  n: the host's copy of cand0[K], for the shape checks only --
        the kernel reads its own.  Nothing is copied."""
        K, n = int(slots.numel()), max(int(n), 0)
        st, keep = self._pool(pool)
        i32, f64 = torch.int32, torch.float64
        self._call("gnnb_strong_pick", C.byref(st), self._rows(slots, K, 1, i32, "slots").data_ptr(), K,
                   self._rows(cand0, K + 1, 1, i32, "cand0").data_ptr(), self._rows(cand_dec, n, 2, i32, "cand_dec").data_ptr(),
                   self._rows(live, 2 * n, 1, i32, "live").data_ptr(), self._rows(infeasible, 2 * n, 1, i32, "infeasible").data_ptr(),
                   self._rows(bound, 2 * n, 1, f64, "bound").data_ptr(), self._rows(decisions, K, 2, i32, "decisions").data_ptr(),
                   self._rows(best_improvement, K, 1, f64, "best_improvement").data_ptr(),
                   self._rows(improvement, n, 1, f64, "improvement").data_ptr(),
                   None if table is None else self._rows(table, K, self.R, f64, "table").data_ptr())

    def strong_rows_jobs(self, cand_slot, c, segments, seg_cap, seg_x_lo, seg_x_hi, seg_prop_w, seg_prop_b, x_lo, x_hi, prop_w, prop_b):
        """gnnb_strong_rows_jobs on the current stream: child rows 2q and 2q + 1 of x_lo / x_hi (2c, N_0) fp64,
        prop_w (2c, N_L) and prop_b (2c,) fp32 receive the box and property row of segment cand_slot[q] // seg_cap from the per-segment
        tables seg_x_lo / seg_x_hi (segments, N_0), seg_prop_w (segments, N_L), seg_prop_b (segments,); cand_slot (c,) int32 is a chunk of
        ``strong_list``'s.  A slot outside the pool leaves its two rows unwritten.  Nothing is copied by the host."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        c, S = int(c), int(segments)
        n, N0, NL, i32, f32, f64 = max(c, 0), self.sizes[0], self.sizes[-2], torch.int32, torch.float32, torch.float64
        self._call("gnnb_strong_rows_jobs", self._rows(cand_slot, n, 1, i32, "cand_slot").data_ptr(), c, S, int(seg_cap),
                   self._rows(seg_x_lo, max(S, 0), N0, f64, "seg_x_lo").data_ptr(), self._rows(seg_x_hi, max(S, 0), N0, f64, "seg_x_hi").data_ptr(),
                   self._rows(seg_prop_w, max(S, 0), NL, f32, "seg_prop_w").data_ptr(), self._rows(seg_prop_b, max(S, 0), 1, f32, "seg_prop_b").data_ptr(),
                   self._rows(x_lo, 2 * n, N0, f64, "x_lo").data_ptr(), self._rows(x_hi, 2 * n, N0, f64, "x_hi").data_ptr(),
                   self._rows(prop_w, 2 * n, NL, f32, "prop_w").data_ptr(), self._rows(prop_b, 2 * n, 1, f32, "prop_b").data_ptr())

    def _children(self, ch, n, what=None):
        """The gnnb_children of a set of child rows (any object with mask, lb, ub, infeasible, bound, alpha, beta, ubv, live) and what must
        outlive the call.  what: the rows' name in a message (None: loose tensors, named as ``frontier_commit`` takes them)."""
        R, f64, i32 = self.R, torch.float64, torch.int32

        def name(a):
            return f"{what}.{a}" if what else {"ubv": "ub_value"}.get(a, a)
        tl, tu = self._layer_rows(ch.lb, n, 1, f64, name("lb")), self._layer_rows(ch.ub, n, 1, f64, name("ub"))
        ptrs = [self._rows(getattr(ch, a), n, cols, dtype, name(a)).data_ptr()
                for a, cols, dtype in (("mask", R, torch.int8), ("infeasible", 1, i32), ("bound", 1, f64), ("alpha", R, f64), ("beta", R, f64),
                                       ("ubv", 1, f64), ("live", 1, i32))]
        return _lib.Children(ptrs[0], tl, tu, *ptrs[1:], len(self.sizes)), (tl, tu)

    def frontier_choose(self, pool, K, m, sel_rows, sel_slots, sel_decisions, gnn_decisions, gnn_improvement, pair_a, pair_b, ineff, kw_improvement,
                        used_kw, decisions):
        """gnnb_frontier_choose on the current stream: ``bab_caller.resolve_branching`` for the m selected parents of ``frontier_fallback``
        once their KW children (pair_b: 2m rows, rows 2j / 2j + 1 those of sel_rows[j]) are bounded.  A parent whose KW pair improves the
        bound more than its GNN pair gets pair_b's rows copied over rows 2 sel_rows[j], + 1 of pair_a (2K rows) and the KW decision; one
        whose KW pair improves less, and less than 0.05, adds 1 to ineff[node].  Writes kw_improvement (K,) fp64 (-1: not selected),
        used_kw (K,) and decisions (K, 2) int32.  pair_a / pair_b: objects with mask, lb, ub, infeasible, bound, alpha, beta, ubv, live."""
        st, keep = self._pool(pool)
        i32 = torch.int32
        pa, keep_a = self._children(pair_a, 2 * K, "pair_a")
        pb, keep_b = self._children(pair_b, 2 * max(m, 1), "pair_b")
        self._call("gnnb_frontier_choose", C.byref(st), K, m, self._rows(sel_rows, max(m, 1), 1, i32, "sel_rows").data_ptr(),
                   self._rows(sel_slots, max(m, 1), 1, i32, "sel_slots").data_ptr(),
                   self._rows(sel_decisions, max(m, 1), 2, i32, "sel_decisions").data_ptr(),
                   self._rows(gnn_decisions, K, 2, i32, "gnn_decisions").data_ptr(),
                   self._rows(gnn_improvement, K, 1, torch.float64, "gnn_improvement").data_ptr(), C.byref(pa), C.byref(pb),
                   self._rows(ineff, self.R, 1, i32, "ineff").data_ptr(),
                   self._rows(kw_improvement, K, 1, torch.float64, "kw_improvement").data_ptr(),
                   self._rows(used_kw, K, 1, i32, "used_kw").data_ptr(), self._rows(decisions, K, 2, i32, "decisions").data_ptr())

    def frontier_learn(self, K, gnn_decisions, kw_decisions, used_kw, gnn_improvement, kw_improvement, online_threshold, wrong, learn_rows, learn_kw,
                       learn_imp, n_learn):
        """gnnb_frontier_learn on the current stream: ``bab_caller.resolve_online``'s count of wrong points for the
        K parents of a round once ``frontier_choose`` has run.  A row with used_kw = 1 adds 1 to wrong[flat index of its GNN decision]
        (wrong: (R,) int32, read and updated in row order); once that count reaches ``online_threshold`` the row is a learn row: learn_rows /
        learn_kw (the flat index of its KW decision) (K,) int32 and learn_imp (K,) fp32 (1.0 if the KW pair improved the bound by more than
        0.1 over the GNN's, else 0.0) receive it densely and in row order, n_learn (1,) int32 their number."""
        i32, f64 = torch.int32, torch.float64
        self._call("gnnb_frontier_learn", K, self._rows(gnn_decisions, K, 2, i32, "gnn_decisions").data_ptr(),
                   self._rows(kw_decisions, K, 2, i32, "kw_decisions").data_ptr(), self._rows(used_kw, K, 1, i32, "used_kw").data_ptr(),
                   self._rows(gnn_improvement, K, 1, f64, "gnn_improvement").data_ptr(),
                   self._rows(kw_improvement, K, 1, f64, "kw_improvement").data_ptr(), int(online_threshold),
                   self._rows(wrong, self.R, 1, i32, "wrong").data_ptr(), self._rows(learn_rows, K, 1, i32, "learn_rows").data_ptr(),
                   self._rows(learn_kw, K, 1, i32, "learn_kw").data_ptr(), self._rows(learn_imp, K, 1, torch.float32, "learn_imp").data_ptr(),
                   self._rows(n_learn, 1, 1, i32, "n_learn").data_ptr())

    def _witness_src(self, n, m, x_a, x_b, used_kw, sel_rows):
        """The gnnb_witness_src of a round of n parents, m of them selected (x_b / used_kw / sel_rows: None, or pair B's)."""
        N0, i32, lists = self.sizes[0], torch.int32, max(int(m), 1)
        return _lib.WitnessSrc(self._rows(x_a, 2 * n, N0, torch.float32, "x_a").data_ptr(),
                               None if x_b is None else self._rows(x_b, 2 * lists, N0, torch.float32, "x_b").data_ptr(),
                               None if used_kw is None else self._rows(used_kw, n, 1, i32, "used_kw").data_ptr(),
                               None if sel_rows is None else self._rows(sel_rows, lists, 1, i32, "sel_rows").data_ptr(), int(m))

    def frontier_witness(self, K, children, x_a, best_value, best_point, x_b=None, used_kw=None, sel_rows=None, m=0):
        """gnnb_frontier_witness on the current stream, between the choice and ``frontier_commit``: the lowest
        ub_value among the live feasible rows of ``children`` (2K rows; an object with mask, lb, ub, infeasible, bound, alpha, beta, ubv,
        live), equal values by row; when it is strictly below best_value ((1,) fp64, +inf at the start of a run) the point it was
        evaluated at goes to best_point ((N_0,) fp32) and the value to best_value.  x_a (2K, N_0) fp32: the rows' points; a row whose
        parent has used_kw set takes row 2j + (c & 1) of x_b ((2m, N_0) fp32) with sel_rows[j] its parent, as ``frontier_choose`` left them."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        ch, keep = self._children(children, 2 * K, "children")
        src = self._witness_src(K, m, x_a, x_b, used_kw, sel_rows)
        self._call("gnnb_frontier_witness", K, C.byref(ch), C.byref(src), self._rows(best_value, 1, 1, torch.float64, "best_value").data_ptr(),
                   self._rows(best_point, 1, self.sizes[0], torch.float32, "best_point").data_ptr())

    # ---- many jobs in one pool (frontier.py verify_properties; include/gnnb.h gnnb_frontier_*_jobs) ------------------------------------
    def _plan(self, plan):
        """The gnnb_plan of a ``frontier.RoundPlan`` (any object with its attributes): host (E, 3) int32 CPU tensor, device the same values
        on the device, n_entries, n, segments, seg_cap."""
        if not torch.is_tensor(plan.host) or plan.host.dtype != torch.int32 or plan.host.device.type != "cpu" or not plan.host.is_contiguous() \
                or plan.host.numel() < 3 * plan.n_entries:
            raise ValueError(f"plan.host: expected a contiguous int32 CPU tensor with at least {plan.n_entries}x3 values")
        self._rows(plan.device, max(int(plan.n_entries), 0), 3, torch.int32, "plan.device")
        return _lib.Plan(plan.host.data_ptr(), plan.device.data_ptr(), int(plan.n_entries), int(plan.n), int(plan.segments), int(plan.seg_cap))

    def frontier_pick_jobs(self, pool, plan, state, slots, row_seg):
        """gnnb_frontier_pick_jobs on the current stream: per plan entry the k slots of lowest bound of its segment (``FrontierRun.pick``'s
        rule on the segment) as global slot numbers into slots[row0:row0 + k], the segment into row_seg[row0:row0 + k] ((n,) int32 each).
        state: the (segments, ``_lib.FRONTIER_STATE_DOUBLES``) records."""
        st, keep = self._pool(pool)
        pl, n = self._plan(plan), max(int(plan.n), 0)
        args = (self._rows(state, max(int(plan.segments), 0), _lib.FRONTIER_STATE_DOUBLES, torch.float64, "state").data_ptr(),
                self._rows(slots, n, 1, torch.int32, "slots").data_ptr(), self._rows(row_seg, n, 1, torch.int32, "row_seg").data_ptr())
        self._call("gnnb_frontier_pick_jobs", C.byref(st), C.byref(pl), *args)

    def frontier_rows_jobs(self, plan, row_seg, seg_x_lo, seg_x_hi, seg_prop_w, seg_prop_b, x_lo, x_hi, prop_w, prop_b, child_x_lo, child_x_hi,
                           child_prop_w, child_prop_b):
        """gnnb_frontier_rows_jobs on the current stream: the boxes and property rows of the n parent rows (x_lo / x_hi (n, N_0) fp64, prop_w
        (n, N_L), prop_b (n,) fp32) and of the 2n child rows (child_*) from the per-segment tables seg_* by row_seg ((n,) int32)."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        pl, n, S, N0, NL = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0), self.sizes[0], self.sizes[-2]
        f64, f32 = torch.float64, torch.float32
        args = (self._rows(row_seg, n, 1, torch.int32, "row_seg").data_ptr(),
                self._rows(seg_x_lo, S, N0, f64, "seg_x_lo").data_ptr(), self._rows(seg_x_hi, S, N0, f64, "seg_x_hi").data_ptr(),
                self._rows(seg_prop_w, S, NL, f32, "seg_prop_w").data_ptr(), self._rows(seg_prop_b, S, 1, f32, "seg_prop_b").data_ptr(),
                self._rows(x_lo, n, N0, f64, "x_lo").data_ptr(), self._rows(x_hi, n, N0, f64, "x_hi").data_ptr(),
                self._rows(prop_w, n, NL, f32, "prop_w").data_ptr(), self._rows(prop_b, n, 1, f32, "prop_b").data_ptr(),
                self._rows(child_x_lo, 2 * n, N0, f64, "child_x_lo").data_ptr(), self._rows(child_x_hi, 2 * n, N0, f64, "child_x_hi").data_ptr(),
                self._rows(child_prop_w, 2 * n, NL, f32, "child_prop_w").data_ptr(), self._rows(child_prop_b, 2 * n, 1, f32, "child_prop_b").data_ptr())
        self._call("gnnb_frontier_rows_jobs", C.byref(pl), *args)

    def frontier_commit_jobs(self, pool, plan, slots, mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live, state, decision_bound, eps=1e-4,
                             workspace=None):
        """gnnb_frontier_commit_jobs on the current stream: ``frontier_commit`` per plan entry on its children (rows [2 row0, 2 row0 + 2k) of
        the 2n-row tensors), its parents' slots (slots (n,) int32, global numbers), its segment, its record of ``state`` ((segments, 9)
        fp64) and its entry of ``decision_bound`` ((segments,) fp64 on the device, NaN: none)."""
        st, keep = self._pool(pool)
        pl, n, S = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0)
        ch, keep_ch = self._children(_ChildRows(mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live), 2 * n)
        self._rows(state, S, _lib.FRONTIER_STATE_DOUBLES, torch.float64, "state")
        self._rows(decision_bound, S, 1, torch.float64, "decision_bound")
        ws = self._workspace("commit_jobs", max(n, 1), "gnnb_frontier_commit_jobs_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_commit_jobs", C.byref(st), C.byref(pl), self._rows(slots, n, 1, torch.int32, "slots").data_ptr(), C.byref(ch),
                   float(eps), decision_bound.data_ptr(), state.data_ptr(), ws.data_ptr(), ws.numel())

    def frontier_fallback_jobs(self, pool, plan, slots, live, infeasible, bound, scores, intercepts, scorer_mask, icp, ineff, seg_x_lo, seg_x_hi,
                               seg_prop_w, seg_prop_b, gnn_improvement, kw_decisions, sel_rows, sel_slots, sel_decisions, m_entry, b_x_lo, b_x_hi,
                               b_prop_w, b_prop_b, branching_threshold, kwbd_threshold=10, sparsest_layer=0, decision_threshold=0.001, random_order=None,
                               workspace=None):
        """gnnb_frontier_fallback_jobs on the current stream: ``frontier_fallback`` per plan entry on its rows with
        its segment's counter icp[segment] ((segments,) int32) and table ineff[segment] ((segments, R) int32).  gnn_improvement (n,) and
        kw_decisions (n, 2) by global row; the selected parents of all entries as one dense list in plan order -- sel_rows (global rows),
        sel_slots (global slots) (n,), sel_decisions (n, 2) -- and m_entry (n_entries + 1,) int32: m per entry, then their sum M.  The
        boxes and property rows of pair B's rows 2q, 2q + 1 (q < M) go from the seg_* tables to b_x_lo / b_x_hi (2n, N_0), b_prop_w
        (2n, N_L), b_prop_b (2n,)."""
        st, keep = self._pool(pool)
        pl, n, S, E = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0), max(int(plan.n_entries), 0)
        N0, NL, f64, f32, i32 = self.sizes[0], self.sizes[-2], torch.float64, torch.float32, torch.int32
        fb, keep_fb = self._fallback(n, S, live, infeasible, bound, scores, intercepts, scorer_mask, icp, ineff, branching_threshold, kwbd_threshold,
                                     sparsest_layer, decision_threshold, random_order)
        ws = self._workspace("fallback_jobs", max(n, 1), "gnnb_frontier_fallback_jobs_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_fallback_jobs", C.byref(st), C.byref(pl), self._rows(slots, n, 1, i32, "slots").data_ptr(), C.byref(fb),
                   self._rows(seg_x_lo, S, N0, f64, "seg_x_lo").data_ptr(), self._rows(seg_x_hi, S, N0, f64, "seg_x_hi").data_ptr(),
                   self._rows(seg_prop_w, S, NL, f32, "seg_prop_w").data_ptr(), self._rows(seg_prop_b, S, 1, f32, "seg_prop_b").data_ptr(),
                   self._rows(gnn_improvement, n, 1, f64, "gnn_improvement").data_ptr(), self._rows(kw_decisions, n, 2, i32, "kw_decisions").data_ptr(),
                   self._rows(sel_rows, n, 1, i32, "sel_rows").data_ptr(), self._rows(sel_slots, n, 1, i32, "sel_slots").data_ptr(),
                   self._rows(sel_decisions, n, 2, i32, "sel_decisions").data_ptr(), self._rows(m_entry, E + 1, 1, i32, "m_entry").data_ptr(),
                   self._rows(b_x_lo, 2 * n, N0, f64, "b_x_lo").data_ptr(), self._rows(b_x_hi, 2 * n, N0, f64, "b_x_hi").data_ptr(),
                   self._rows(b_prop_w, 2 * n, NL, f32, "b_prop_w").data_ptr(), self._rows(b_prop_b, 2 * n, 1, f32, "b_prop_b").data_ptr(),
                   ws.data_ptr(), ws.numel())

    def frontier_choose_jobs(self, pool, plan, M, m_entry, sel_rows, sel_slots, sel_decisions, gnn_decisions, gnn_improvement, pair_a, pair_b, ineff,
                             kw_improvement, used_kw, decisions):
        """gnnb_frontier_choose_jobs on the current stream: ``frontier_choose`` per plan entry on its range of the dense lists
        (``frontier_fallback_jobs``' outputs; M: the host's copy of m_entry[n_entries]) with ineff[segment] ((segments, R) int32).  pair_a:
        the 2n child rows, pair_b: the 2M rows bounded for the selected parents.  Writes kw_improvement (n,), used_kw (n,), decisions (n, 2)."""
        st, keep = self._pool(pool)
        pl, n, S, E = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0), max(int(plan.n_entries), 0)
        i32, lists = torch.int32, max(int(M), 1)
        pa, keep_a = self._children(pair_a, 2 * n, "pair_a")
        pb, keep_b = self._children(pair_b, 2 * lists, "pair_b")
        self._call("gnnb_frontier_choose_jobs", C.byref(st), C.byref(pl), int(M), self._rows(m_entry, E + 1, 1, i32, "m_entry").data_ptr(),
                   self._rows(sel_rows, lists, 1, i32, "sel_rows").data_ptr(), self._rows(sel_slots, lists, 1, i32, "sel_slots").data_ptr(),
                   self._rows(sel_decisions, lists, 2, i32, "sel_decisions").data_ptr(), self._rows(gnn_decisions, n, 2, i32, "gnn_decisions").data_ptr(),
                   self._rows(gnn_improvement, n, 1, torch.float64, "gnn_improvement").data_ptr(), C.byref(pa), C.byref(pb),
                   self._rows(ineff, S, self.R, i32, "ineff").data_ptr(), self._rows(kw_improvement, n, 1, torch.float64, "kw_improvement").data_ptr(),
                   self._rows(used_kw, n, 1, i32, "used_kw").data_ptr(), self._rows(decisions, n, 2, i32, "decisions").data_ptr())

    def frontier_learn_jobs(self, plan, gnn_decisions, kw_decisions, used_kw, gnn_improvement, kw_improvement, online_threshold, wrong, learn_rows,
                            learn_kw, learn_imp, learn_entry, workspace=None):
        """gnnb_frontier_learn_jobs on the current stream, behind ``frontier_choose_jobs``: ``frontier_learn`` per
        plan entry on its rows with its segment's table wrong[segment] ((segments, R) int32).  The learn rows of all entries form one dense
        list in plan order -- learn_rows (GLOBAL rows of the n-row parent batch), learn_kw (n,) int32, learn_imp (n,) fp32 -- and
        learn_entry (n_entries + 1,) int32 receives the count per entry, then their sum N."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        pl, n, S, E = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0), max(int(plan.n_entries), 0)
        i32, f64 = torch.int32, torch.float64
        ws = self._workspace("learn_jobs", max(n, 1), "gnnb_frontier_learn_jobs_workspace_bytes") if workspace is None else workspace
        self._call("gnnb_frontier_learn_jobs", C.byref(pl), self._rows(gnn_decisions, n, 2, i32, "gnn_decisions").data_ptr(),
                   self._rows(kw_decisions, n, 2, i32, "kw_decisions").data_ptr(), self._rows(used_kw, n, 1, i32, "used_kw").data_ptr(),
                   self._rows(gnn_improvement, n, 1, f64, "gnn_improvement").data_ptr(),
                   self._rows(kw_improvement, n, 1, f64, "kw_improvement").data_ptr(), int(online_threshold),
                   self._rows(wrong, S, self.R, i32, "wrong").data_ptr(), self._rows(learn_rows, n, 1, i32, "learn_rows").data_ptr(),
                   self._rows(learn_kw, n, 1, i32, "learn_kw").data_ptr(), self._rows(learn_imp, n, 1, torch.float32, "learn_imp").data_ptr(),
                   self._rows(learn_entry, E + 1, 1, i32, "learn_entry").data_ptr(), ws.data_ptr(), ws.numel())

    def frontier_witness_jobs(self, plan, children, x_a, best_value, best_point, M=0, m_entry=None, x_b=None, used_kw=None, sel_rows=None):
        """gnnb_frontier_witness_jobs on the current stream: ``frontier_witness`` per plan entry on its rows of ``children`` (2n rows) and
        its range of the dense lists (M, m_entry: ``frontier_fallback_jobs``'), with best_value[segment] ((segments,) fp64) and
        best_point[segment] ((segments, N_0) fp32)."""
        if self.sizes is None:
            raise RuntimeError("bind a network first")
        pl, n, S, E = self._plan(plan), max(int(plan.n), 0), max(int(plan.segments), 0), max(int(plan.n_entries), 0)
        ch, keep = self._children(children, 2 * n, "children")
        src = self._witness_src(n, M, x_a, x_b, used_kw, sel_rows)
        self._call("gnnb_frontier_witness_jobs", C.byref(pl), int(M), None if m_entry is None else self._rows(m_entry, E + 1, 1, torch.int32, "m_entry").data_ptr(),
                   C.byref(ch), C.byref(src), self._rows(best_value, S, 1, torch.float64, "best_value").data_ptr(),
                   self._rows(best_point, S, self.sizes[0], torch.float32, "best_point").data_ptr())

    # ---- inspection (tests / bench) ---------------------------------------------------------
    def mu_rows(self, B, k):
        """(rows, linear_id): the raw rows of graph layer k as the last forward at batch B left them in the workspace -- a
        (B, N_k, p) view -- and the index (state-dict order) of the Linear they still have to go through: producers leave
        their last Linear to the consumer, mu = (W.rows + b).[r0 != 0]; -1: the rows are final.
        Rows of dead nodes, and after a default (restricted) forward the rows of layer 1 that are not scored, hold
        whatever was there before."""
        off, n = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.gnnb_mu_location(self.h, B, k, C.byref(off), C.byref(n)), "gnnb_mu_location")
        ws = self.workspace(B)
        rows = ws[off.value:off.value + 4 * n.value].view(torch.float32).view(B, self.sizes[k], self.p)
        lid = C.c_int(-1)
        _lib.check(self.lib.gnnb_mu_projection(self.h, k, C.byref(lid)), "gnnb_mu_projection")
        return rows, lid.value

    def linear_host(self, idx):
        """(weight (out, in), bias (out)) of the idx-th Linear of the checkpoint as float64 numpy arrays."""
        off = sum(o * i + o for o, i in GNN_LINEARS[:idx])
        o, i = GNN_LINEARS[idx]
        return (self._blob[off:off + o * i].reshape(o, i).astype(np.float64), self._blob[off + o * i:off + o * i + o].astype(np.float64))

    def mu(self, B, k):
        """Embedding mu[k] (B, N_k, p) of the last forward at batch B, for inspection: the deferred projection is applied
        on the HOST in float64 (numpy), nothing of it runs through torch on the GPU.  Returns a float32 CPU tensor."""
        rows, lid = self.mu_rows(B, k)
        rows = rows.cpu().numpy()
        if lid < 0:
            return torch.from_numpy(rows.copy())
        W, b = self.linear_host(lid)
        live = np.ones(rows.shape[:2], dtype=bool)
        if 1 <= k < len(self.sizes) - 1:
            lb, ub = (t.reshape(B, -1).cpu().numpy() for t in self._last_bounds[k])
            lower_temp, upper_temp = lb - np.maximum(lb, 0), np.maximum(ub, 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                live = (upper_temp / (upper_temp - lower_temp)) != 0      # graph_conv.py:178 / :347
        safe = np.where(live[..., None], rows, 0.0).astype(np.float64)     # dead rows may never have been written
        out = (safe @ W.T + b) * live[..., None]
        return torch.from_numpy(out.astype(np.float32))

    def describe(self):
        """The launch plan of one forward on the bound network (dict parsed from gnnb_describe's JSON)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        _lib.check(self.lib.gnnb_describe(self.h, buf, len(buf)), "gnnb_describe")
        return json.loads(buf.value.decode())

    def set_halfpass_limit(self, n):
        _lib.check(self.lib.gnnb_set_halfpass_limit(self.h, n), "gnnb_set_halfpass_limit")

    def profile_enable(self, on):
        _lib.check(self.lib.gnnb_profile_enable(self.h, int(on)), "gnnb_profile_enable")

    def profile_trace(self, cap=4096):
        """[(kernel class name, ms)] of the launches ``profile_read`` has resolved since the last call, in launch order."""
        cls, ms = (C.c_int * cap)(), (C.c_double * cap)()
        n = self.lib.gnnb_profile_trace(self.h, cls, ms, cap)
        if n < 0:
            raise RuntimeError("gnnb_profile_trace failed")
        return [(self.lib.gnnb_profile_class_name(cls[i]).decode(), ms[i]) for i in range(min(n, cap))]

    def profile_read(self, reset=True):
        n = self.lib.gnnb_profile_classes()
        ms, cnt = (C.c_double * n)(), (C.c_int64 * n)()
        _lib.check(self.lib.gnnb_profile_read(self.h, ms, cnt, n, int(reset)), "gnnb_profile_read")
        return {self.lib.gnnb_profile_class_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}
