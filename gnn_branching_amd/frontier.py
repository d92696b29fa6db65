"""Branch and bound on a frontier of open domains that stays in device memory.

``lp_producer.branch_and_bound`` handles one domain per iteration and moves every bound, dual and primal through Python lists.  Here
the open domains live in a ``DomainPool`` of device tensors, a round expands the K of lowest bound with ONE call of each batch kernel
(``gnnb_dual_ascent`` at n_iter 0 for the scorer's inputs, ``gnnb_forward``, ``gnnb_kw_bounds``, ``gnnb_dual_ascent``) and the steps in
between are the kernels of csrc/gnnb_k_frontier.h (gather, expand, net_eval, commit).  Per round the host reads back one record of
``_lib.FRONTIER_STATE_DOUBLES`` doubles and nothing else.

The rule of a round is ``branch_and_bound``'s, for K domains at once: the children of all K parents are bounded, then
global_ub = min(global_ub, ub of every feasible child), then every child is kept (lb < global_ub - eps, below the decision bound, an
undecided ReLU left) or closed against that one global_ub.  With K = 1 this is ``branch_and_bound`` with ``child_lp="dual_device"``.
"""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib
from .engine import table


class DomainPool:
    """``capacity`` slots of open domains as device tensors (the gnnb_pool of include/gnnb.h) and the loop's state record.

    Per slot: mask (R,) int8 resolved by the bounds; lb / ub per graph layer 1..L+1 (N_k,) fp64, mask applied, exactly as
    ``gnnb_kw_bounds`` wrote them; alpha / beta (R,) fp64, the dual point ``bound`` is the value of; bound; open."""

    def __init__(self, engine, capacity):
        if engine.sizes is None:
            raise RuntimeError("bind the network first (ScorerEngine.bind)")
        dev, R = engine.device, engine.R
        self.capacity = int(capacity)
        cap = self.capacity
        self.mask = torch.zeros(cap, R, dtype=torch.int8, device=dev)
        self.lb = [torch.zeros(cap, n, dtype=torch.float64, device=dev) for n in engine.sizes[1:]]
        self.ub = [torch.zeros(cap, n, dtype=torch.float64, device=dev) for n in engine.sizes[1:]]
        self.alpha = torch.zeros(cap, R, dtype=torch.float64, device=dev)
        self.beta = torch.zeros(cap, R, dtype=torch.float64, device=dev)
        self.bound = torch.zeros(cap, dtype=torch.float64, device=dev)
        self.open = torch.zeros(cap, dtype=torch.int32, device=dev)
        inf = float("inf")
        self.state = torch.tensor([inf, inf, inf] + [0.0] * (_lib.FRONTIER_STATE_DOUBLES - 3), dtype=torch.float64, device=dev)

    @staticmethod
    def bytes_per_domain(sizes, R):
        """mask + alpha + beta over the R ReLU nodes, two fp64 bounds per node of graph layers 1..L+1, bound, open."""
        return R * (1 + 8 + 8) + 16 * sum(sizes[1:]) + 8 + 4

    def arrays(self):
        return [self.mask] + self.lb + self.ub + [self.alpha, self.beta, self.bound, self.open]

    def compact(self, n_open):
        """Move the open slots to the front, in slot order (torch indexing on the device, no synchronisation).  ``n_open``: their number,
        which the host knows from the state record; the record's slots-in-use becomes it."""
        order = torch.sort(self.open, descending=True, stable=True).indices
        self.mask, self.alpha, self.beta, self.bound, self.open = (t[order].contiguous() for t in (self.mask, self.alpha, self.beta, self.bound, self.open))
        self.lb = [t[order].contiguous() for t in self.lb]
        self.ub = [t[order].contiguous() for t in self.ub]
        self.state[_lib.FS_IN_USE] = float(n_open)


class _Rows:
    """Dense batch rows for n domains: what the batch kernels read and write, allocated once."""

    def __init__(self, eng, fixed, n, in_shape, with_fp32):
        dev, R, sizes = eng.device, eng.R, eng.sizes
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        self.mask = torch.zeros(n, R, dtype=torch.int8, device=dev)
        self.lb = [torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]]
        self.ub = [torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]]
        self.alpha = torch.zeros(n, R, dtype=f64, device=dev)
        self.beta = torch.zeros(n, R, dtype=f64, device=dev)
        self.bound = torch.zeros(n, dtype=f64, device=dev)
        self.dual = [torch.zeros(n * s, 3, dtype=f32, device=dev) for s in sizes[1:-1]]
        self.prims, k = [], 0
        for q, l in enumerate(fixed):                             # primals[q]: the output of network layer q (as ScorerEngine.dual_ascent)
            nxt = fixed[q + 1] if q + 1 < len(fixed) else None
            if type(l) is nn.ReLU or type(nxt) is nn.ReLU:
                k += type(nxt) is nn.ReLU
                self.prims.append(torch.zeros(n * sizes[k], dtype=f32, device=dev))
            else:
                self.prims.append(torch.zeros(1, dtype=f32, device=dev))
        self.prims.append(torch.zeros(n, dtype=f32, device=dev))
        self.x_lp = torch.zeros((n,) + tuple(in_shape), dtype=f32, device=dev)
        if with_fp32:                                             # the picked parents: the scorer's side
            self.lb32 = [torch.zeros(n, s, dtype=f32, device=dev) for s in sizes]
            self.ub32 = [torch.zeros(n, s, dtype=f32, device=dev) for s in sizes]
            self.amb = torch.zeros(n, R, dtype=f32, device=dev)
            self.scores = torch.zeros(n, R, dtype=f32, device=dev)
            self.dec = torch.zeros(n, 2, dtype=i32, device=dev)
        else:                                                     # the children: the bounding side
            self.plb = [torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]]
            self.pub = [torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]]
            self.split = torch.full((n,), -1, dtype=i32, device=dev)
            self.live = torch.zeros(n, dtype=i32, device=dev)
            self.infeasible = torch.zeros(n, dtype=i32, device=dev)
            self.ubv = torch.zeros(n, dtype=f64, device=dev)


def _check_args(K, n_iter, lr, eps, max_rounds, capacity):
    if not isinstance(K, int) or isinstance(K, bool) or K < 1 or K > 32767:
        raise ValueError(f"K = {K!r}: an integer in 1..32767")
    if capacity is None:
        capacity = max(1024, 4 * K + 1)
    if not isinstance(capacity, int) or capacity < 2 * K + 1:
        raise ValueError(f"capacity = {capacity!r}: at least 2K + 1 = {2 * K + 1} slots")
    if not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError(f"n_iter = {n_iter!r}")
    if not isinstance(max_rounds, int) or max_rounds < 0:
        raise ValueError(f"max_rounds = {max_rounds!r}")
    if not (eps >= 0) or not (lr > 0):
        raise ValueError(f"eps = {eps!r}, lr = {lr!r}")
    return capacity


class FrontierRun:
    """The device side of ``branch_and_bound_frontier``: ``root()`` once, then per round ``launch_round(k)`` (device work only, nothing
    synchronises) and ``read_state()`` (the round's one device-to-host copy)."""

    def __init__(self, lp, choice, layers, K=16, n_iter=20, lr=0.1, eps=1e-4, decision_bound=None, capacity=None):
        self.capacity = _check_args(K, n_iter, lr, eps, 0, capacity)
        layers = list(layers)
        if type(layers[-1]) is not nn.Linear or layers[-1].out_features != 1:
            raise ValueError("the last layer must be the folded property layer Linear(., 1)")
        self.K, self.n_iter, self.lr, self.eps, self.decision_bound = K, n_iter, float(lr), float(eps), decision_bound
        self.fixed, self.prop_layer = layers[:-1], layers[-1]
        eng = self.eng = choice.model.engine()
        in_shape = tuple(lp.input_lb.shape)
        eng.bind(self.fixed, in_shape)
        dev, self.lib, self.ng = eng.device, eng.lib, len(eng.sizes)
        self.pool = DomainPool(eng, self.capacity)
        n = 2 * K
        # one run verifies one property on one box: broadcast rows, filled once
        self.x_lo = lp.input_lb.reshape(1, -1).to(dev, torch.float64).expand(n, -1).contiguous()
        self.x_hi = lp.input_ub.reshape(1, -1).to(dev, torch.float64).expand(n, -1).contiguous()
        self.pw = self.prop_layer.weight.detach().reshape(1, -1).to(dev, torch.float32).expand(n, -1).contiguous()
        self.pb = self.prop_layer.bias.detach().reshape(1).to(dev, torch.float32).expand(n).contiguous()
        self.P = _Rows(eng, self.fixed, K, in_shape, True)
        self.Ch = _Rows(eng, self.fixed, n, in_shape, False)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.status_all = torch.zeros(1, dtype=torch.int32, device=dev)
        self.root_slot = torch.zeros(1, dtype=torch.int32, device=dev)

        def ws(sizer, B):
            return torch.empty(max(1, getattr(self.lib, sizer)(eng.h, B)), dtype=torch.uint8, device=dev)
        self.ws_fwd, self.ws_kw, self.ws_dual = ws("gnnb_workspace_bytes", K), ws("gnnb_kw_workspace_bytes", n), ws("gnnb_dual_workspace_bytes", n)
        self.ws_eval, self.ws_commit = ws("gnnb_net_eval_workspace_bytes", n), ws("gnnb_frontier_commit_workspace_bytes", K)
        # the argument structs of the existing batch entry points over these rows (pointers never change; B does)
        P, Ch = self.P, self.Ch
        self._keep = [table(g) for g in (P.lb, P.ub, P.lb32, P.ub32, P.dual, P.prims, Ch.lb, Ch.ub, Ch.plb, Ch.pub, Ch.dual, Ch.prims)]
        t = self._keep
        self.dual_P = _lib.DualBatch(t[0], t[1], self.x_lo.data_ptr(), self.x_hi.data_ptr(), self.pw.data_ptr(), self.pb.data_ptr(), P.mask.data_ptr(), self.ng)
        self.fwd_P = _lib.Batch(t[2], t[3], t[4], t[5], P.x_lp.data_ptr(), self.pw.data_ptr(), self.pb.data_ptr(), P.amb.data_ptr(), self.ng,
                                len(P.dual), len(P.prims))
        self.kw_Ch = _lib.KwBatch(self.x_lo.data_ptr(), self.x_hi.data_ptr(), self.pw.data_ptr(), self.pb.data_ptr(), Ch.mask.data_ptr(), t[8], t[9],
                                  Ch.split.data_ptr(), self.ng)
        self.dual_Ch = _lib.DualBatch(t[6], t[7], self.x_lo.data_ptr(), self.x_hi.data_ptr(), self.pw.data_ptr(), self.pb.data_ptr(), Ch.mask.data_ptr(), self.ng)
        self.slots = None

    # ---- the existing batch entry points on the preallocated rows ------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _bound_children(self, B, warm):
        """gnnb_kw_bounds, gnnb_dual_ascent and gnnb_net_eval over the first B child rows."""
        Ch, lib, h, t = self.Ch, self.lib, self.eng.h, self._keep
        with torch.cuda.device(self.eng.device):
            _lib.check(lib.gnnb_kw_bounds(h, C.byref(self.kw_Ch), B, t[6], t[7], None, None, Ch.infeasible.data_ptr(), self.ws_kw.data_ptr(),
                                          self.ws_kw.numel(), self._stream()), "gnnb_kw_bounds")
            _lib.check(lib.gnnb_dual_ascent(h, C.byref(self.dual_Ch), B, self.n_iter, self.lr, Ch.alpha.data_ptr(), Ch.beta.data_ptr(), int(warm),
                                            Ch.bound.data_ptr(), None, None, t[10], t[11], Ch.x_lp.data_ptr(), None, self.ws_dual.data_ptr(),
                                            self.ws_dual.numel(), self._stream()), "gnnb_dual_ascent")
        self.eng.net_eval(self.fixed, None, Ch.x_lp[:B], out=Ch.ubv, prop=(self.pw, self.pb), workspace=self.ws_eval)

    def _commit(self, slots):
        Ch = self.Ch
        self.eng.frontier_commit(self.pool, slots, Ch.mask, Ch.lb, Ch.ub, Ch.infeasible, Ch.bound, Ch.alpha, Ch.beta, Ch.ubv, Ch.live, self.pool.state,
                                 eps=self.eps, decision_bound=self.decision_bound, workspace=self.ws_commit)

    def root(self):
        """Bound the domain with every ReLU undecided (no parent, the default start of the ascent) and commit it as the first open domain:
        child row 0 of a commit with K = 1, slot 0, live = [1, 0]."""
        Ch = self.Ch
        Ch.mask[:1].fill_(-1)
        Ch.split[:2].fill_(-1)
        Ch.live[:2] = torch.tensor([1, 0], dtype=torch.int32).to(Ch.live.device)
        self._bound_children(1, warm=False)
        self._commit(self.root_slot)
        st = self.read_state()
        if st[_lib.FS_INFEASIBLE] > 0:
            raise RuntimeError("infeasible root domain")
        return st

    def pick(self, k, in_use):
        """The k open slots of lowest bound, equal bounds by slot index: a stable sort on the device."""
        pool = self.pool
        key = torch.where(pool.open[:in_use] > 0, pool.bound[:in_use], float("inf"))
        return torch.sort(key, stable=True).indices[:k].to(torch.int32).contiguous()

    def launch_round(self, k, in_use):
        """One round over the k <= K open domains of lowest bound.  Device work only."""
        P, Ch, eng, lib, h, t, pool = self.P, self.Ch, self.eng, self.lib, self.eng.h, self._keep, self.pool
        slots = self.slots = self.pick(k, in_use)
        eng.frontier_gather(pool, slots, self.x_lo, self.x_hi, P.mask, P.lb, P.ub, P.lb32, P.ub32, P.alpha, P.beta, P.amb)
        with torch.cuda.device(eng.device):
            # the scorer's inputs at the stored best point: one evaluation of g (n_iter = 0) instead of ~120 KB of fp32 inputs per open domain
            _lib.check(lib.gnnb_dual_ascent(h, C.byref(self.dual_P), k, 0, self.lr, P.alpha.data_ptr(), P.beta.data_ptr(), 1, P.bound.data_ptr(), None, None,
                                            t[4], t[5], P.x_lp.data_ptr(), P.lb32[-1].data_ptr(), self.ws_dual.data_ptr(), self.ws_dual.numel(),
                                            self._stream()), "gnnb_dual_ascent")
            _lib.check(lib.gnnb_forward(h, C.byref(self.fwd_P), k, P.scores.data_ptr(), P.dec.data_ptr(), self.status.data_ptr(), self.ws_fwd.data_ptr(),
                                        self.ws_fwd.numel(), self._stream()), "gnnb_forward")
        self.status_all |= self.status
        eng.frontier_expand(pool, slots, P.dec, Ch.mask, Ch.plb, Ch.pub, Ch.split, Ch.alpha, Ch.beta, Ch.live)
        self._bound_children(2 * k, warm=True)
        self._commit(slots)

    def read_state(self):
        """The state record as a list of Python floats: the one device-to-host copy of a round."""
        return self.pool.state.cpu().tolist()

    def check_status(self):
        from .engine import _raise_for_status
        _raise_for_status(int(self.status_all.cpu()[0]))


def branch_and_bound_frontier(lp, choice, layers, K=16, n_iter=20, lr=0.1, eps=1e-4, max_rounds=50, decision_bound=None, capacity=None, log=print,
                              trace=None):
    """Branch and bound with the open domains in device memory, K of them expanded per round.

    lp: a ``LayerGraphLP`` (its input box is the root); choice: a ``GraphChoice`` (the GNN; its engine runs every step);
    layers: the network's layers with the folded property layer last.  Per round the up-to-K open domains of lowest bound (equal bounds:
    lowest slot) are split at the GNN's decision, their 2K children bounded by ``gnnb_kw_bounds`` and ``n_iter`` warm-started steps of
    ``gnnb_dual_ascent``, and kept or closed by ``branch_and_bound``'s rule against the global upper bound after the round's minimum.
    The loop stops under ``branch_and_bound``'s conditions: no open domain ("exhausted"), global_ub - global_lb <= eps ("gap"), the
    sign of (minimum - decision_bound) known ("decision"), or after ``max_rounds`` ("max_rounds").  capacity: slots of the pool (None:
    max(1024, 4K + 1)).  A round of k parents needs k slots above the slots in use (its 2k children reuse the parents' slots first): when
    they are not there the pool is compacted, and when the open domains themselves leave no room for k more the loop stops ("capacity") -- global_lb stays sound either way: it is the minimum over the open bounds, closed_lb
    and global_ub.  trace: None, or a list that receives per round a dict of the picked slots, their bounds, the decisions, the
    children's bounds / upper values / live and infeasible flags (extra device-to-host copies: off in a timed run).

    Returns (global_lb, global_ub, rounds, domains_bounded, reason)."""
    _check_args(K, n_iter, lr, eps, max_rounds, capacity)
    run = FrontierRun(lp, choice, layers, K, n_iter, lr, eps, decision_bound, capacity)
    S = _lib
    st = run.root()
    rounds, bounded = 0, 1

    def glb(st):
        return min(st[S.FS_LOWEST_OPEN], st[S.FS_CLOSED_LB], st[S.FS_GLOBAL_UB])
    log(f"root lb {glb(st):.5f} ub {st[S.FS_GLOBAL_UB]:.5f}")
    while True:
        global_lb, global_ub, n_open, in_use = glb(st), st[S.FS_GLOBAL_UB], int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
        if n_open == 0:
            reason = "exhausted"
        elif not global_ub - global_lb > eps:
            reason = "gap"
        elif decision_bound is not None and (global_lb >= decision_bound or global_ub < decision_bound):
            reason = "decision"
        elif rounds >= max_rounds:
            reason = "max_rounds"
        elif n_open + min(K, n_open) > run.capacity:
            reason = "capacity"
        else:
            reason = None
        if reason is not None:
            break
        k = min(K, n_open)
        if in_use + k > run.capacity:                             # the kept children beyond the k parents' slots go above in_use
            run.pool.compact(n_open)
            in_use = n_open
        run.launch_round(k, in_use)
        if trace is not None:
            P, Ch = run.P, run.Ch
            trace.append({"slots": run.slots.cpu().tolist(), "parent_bounds": P.bound[:k].cpu().tolist(), "decisions": P.dec[:k].cpu().tolist(),
                          "child_bounds": Ch.bound[:2 * k].cpu().tolist(), "child_ub": Ch.ubv[:2 * k].cpu().tolist(),
                          "live": Ch.live[:2 * k].cpu().tolist(), "infeasible": Ch.infeasible[:2 * k].cpu().tolist()})
        st = run.read_state()
        if st[S.FS_OVERFLOW] != 0 or math.isnan(st[S.FS_GLOBAL_UB]):
            raise RuntimeError(f"frontier state record is inconsistent: {st}")
        rounds += 1
        bounded += int(st[S.FS_KEPT] + st[S.FS_CLOSED] + st[S.FS_INFEASIBLE])
        log(f"round {rounds} picked {k} kept {int(st[S.FS_KEPT])} closed {int(st[S.FS_CLOSED])} infeasible {int(st[S.FS_INFEASIBLE])} open {int(st[S.FS_N_OPEN])} "
            f"lb {glb(st):.5f} ub {st[S.FS_GLOBAL_UB]:.5f}")
    run.check_status()
    return global_lb, global_ub, rounds, bounded, reason
