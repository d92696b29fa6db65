"""Branch and bound on a frontier of open domains that stays in device memory.

``lp_producer.branch_and_bound`` handles one domain per iteration and moves every bound, dual and primal through Python lists.  Here
the open domains live in a ``DomainPool`` of device tensors, a round expands the K of lowest bound with ONE call of each batch kernel
(``gnnb_dual_ascent`` at n_iter 0 for the scorer's inputs, ``gnnb_forward``, ``gnnb_kw_bounds``, ``gnnb_dual_ascent``) and the steps in
between are the kernels of csrc/gnnb_k_frontier.h (gather, expand, net_eval, commit).  Per round the host reads back one record of
``_lib.FRONTIER_STATE_DOUBLES`` doubles and nothing else.

The rule of a round is ``branch_and_bound``'s, for K domains at once: the children of all K parents are bounded, then
global_ub = min(global_ub, ub of every feasible child), then every child is kept (lb < global_ub - eps, below the decision bound, an
undecided ReLU left) or closed against that one global_ub.  With K = 1 this is ``branch_and_bound`` with ``child_lp="dual_device"``.

``verify_properties`` (``verify_properties_threshold``, section 7.6, with the BaBSR fall-back) runs many JOBS -- a box, a property row, a decision bound, all on one bound network -- through
the same round of launches: the pool is cut into segments of ``capacity`` slots, a segment holds one job and has its own record, and inside
its segment a job runs the rule above unchanged, so it gets the result ``branch_and_bound_frontier`` gives it alone, bit for bit.

``branch_and_bound_frontier(..., branching_threshold=T, online_threshold=N)`` is the reference's online loop
(``lp_producer.branch_and_bound_online``) on the same round: a parent whose KW pair won counts its GNN decision as a wrong point, from the
N-th time on it is a learn row, and behind the commit the round takes one Adam step over its learn rows on the device.
``verify_properties_online`` runs that loop for many jobs in one pool: a wrong-point table per job
(``gnnb_frontier_learn_jobs``) and ONE step per round over the learn rows of all jobs in flight, which share the scorer.

``branch_and_bound_frontier(..., branching="babsr")`` and ``verify_properties_babsr`` are the reference's
``relu_bab`` on the same round: every parent is split at the BaBSR heuristic's decision (``gnnb_babsr``, ``gnnb_frontier_babsr_decide``), one
intercept counter carried through the run (per job), and the GNN is never run.

``branch_and_bound_frontier(..., branching="strong")`` is strong branching, the GNN's teacher, on the same round:
both children of every candidate split of every parent are bounded in chunks (``gnnb_strong_list``, then ``gnnb_frontier_expand``,
``gnnb_kw_bounds`` and ``gnnb_dual_ascent`` per chunk) and every parent is split where its bound improves most (``gnnb_strong_pick``);
``strong_audit=[]`` computes the same table next to a "gnn" or "babsr" run and records how far the committed decision is from the best.

``branch_and_bound_frontier(..., imitate=N)`` connects the two: every N-th round leaves its table in device memory
and, behind the commit, takes one Adam step of the GNN on it (``gnnb_imitation_step_rows``), so a "gnn" or "strong" run labels its own
states with the teacher and learns from them without the table, the scorer inputs or the gradient crossing the link.

``verify_properties_strong`` runs both for many jobs in one pool: the candidates of all jobs' parents form one list
bounded in shared chunks, each candidate's child rows taking their own job's box and property row (``gnnb_strong_rows_jobs``), and with
``imitate=N`` every N-th round the pool launches takes one step over the parents of all jobs in flight, which share the scorer.

``strong_candidates=Shortlist(babsr=M, gnn=G)`` shortlists the candidates by the GNN's own scores as well, or by
them alone (``gnnb_strong_list_union``, ``gnnb_strong_list``), so that the table always labels the scorer's own decision.

``imitate=Replay(every=N, ...)`` keeps the labelled states: a learning round stores its useful rows in a
device-resident ``ReplayBuffer`` (``gnnb_replay_push``) and its steps run on minibatches drawn from it (``gnnb_replay_sample``), which mix
depths, properties and jobs; ``steps=0`` only collects, for ``replay.train_epochs`` to train on later.

``branch_and_bound_frontier`` on a ``LayerGraphLP(..., split_depth=D)`` fills an underfilled round: while k parents leave child rows
unused, each is split on its d best-scored undecided ReLUs at once (``round_depth``; ``gnnb_strong_list`` on the scorer's scores,
``gnnb_frontier_expand_depth``, ``gnnb_frontier_commit_depth``), 2^d children per parent on the same 2K child rows.
"""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib
from .engine import table
from .lp_producer import _random_order


def _start_record():
    """The state record of a pool (or of a segment) nothing has been committed to."""
    inf = float("inf")
    return [inf, inf, inf] + [0.0] * (_lib.FRONTIER_STATE_DOUBLES - 3)


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
        self.state = torch.tensor(_start_record(), dtype=torch.float64, device=dev)

    @staticmethod
    def bytes_per_domain(sizes, R):
        """mask + alpha + beta over the R ReLU nodes, two fp64 bounds per node of graph layers 1..L+1, bound, open."""
        return R * (1 + 8 + 8) + 16 * sum(sizes[1:]) + 8 + 4

    def arrays(self):
        return [self.mask] + self.lb + self.ub + [self.alpha, self.beta, self.bound, self.open]

    def reorder(self, order):
        """Slot i takes what slot order[i] holds, in every array (torch indexing on the device, no synchronisation)."""
        ts, L = [t[order].contiguous() for t in self.arrays()], len(self.lb)
        self.mask, self.lb, self.ub = ts[0], ts[1:1 + L], ts[1 + L:1 + 2 * L]
        self.alpha, self.beta, self.bound, self.open = ts[1 + 2 * L:]

    def compact(self, n_open):
        """Move the open slots to the front, in slot order.  ``n_open``: their number, which the host knows from the state record; the
        record's slots-in-use becomes it."""
        self.reorder(torch.sort(self.open, descending=True, stable=True).indices)
        self.state[_lib.FS_IN_USE] = float(n_open)


class _Rows:
    """Dense batch rows for n domains: what the batch kernels read and write, allocated once, with the pointer tables and the argument
    structs of the batch entry points over them (the pointers never change; the B of a call does).  box: the rows' boxes and property
    rows (x_lo, x_hi (n, N_0) fp64, prop_w (n, N_L), prop_b (n,) fp32), the caller's.  child: the bounding side (gnnb_kw_bounds,
    gnnb_dual_ascent, the commit) instead of the scorer's (gnnb_dual_ascent at n_iter 0, gnnb_forward)."""

    def __init__(self, eng, fixed, n, in_shape, box, child):
        dev, R, sizes, ng = eng.device, eng.R, eng.sizes, len(eng.sizes)
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
        self.box = box
        x_lo, x_hi, pw, pb = (t.data_ptr() for t in box)
        self.t_lb, self.t_ub, self.t_dual, self.t_prims = table(self.lb), table(self.ub), table(self.dual), table(self.prims)
        self.dual_batch = _lib.DualBatch(self.t_lb, self.t_ub, x_lo, x_hi, pw, pb, self.mask.data_ptr(), ng)
        if not child:                                             # the picked parents: the scorer's side
            self.lb32 = [torch.zeros(n, s, dtype=f32, device=dev) for s in sizes]
            self.ub32 = [torch.zeros(n, s, dtype=f32, device=dev) for s in sizes]
            self.amb = torch.zeros(n, R, dtype=f32, device=dev)
            self.scores = torch.zeros(n, R, dtype=f32, device=dev)
            self.dec = torch.zeros(n, 2, dtype=i32, device=dev)
            self.t_lb32, self.t_ub32 = table(self.lb32), table(self.ub32)
            self.fwd_batch = _lib.Batch(self.t_lb32, self.t_ub32, self.t_dual, self.t_prims, self.x_lp.data_ptr(), pw, pb, self.amb.data_ptr(), ng,
                                        len(self.dual), len(self.prims))
        else:                                                     # the children: the bounding side
            self.plb = [torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]]
            self.pub = [torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]]
            self.split = torch.full((n,), -1, dtype=i32, device=dev)
            self.live = torch.zeros(n, dtype=i32, device=dev)
            self.infeasible = torch.zeros(n, dtype=i32, device=dev)
            self.ubv = torch.zeros(n, dtype=f64, device=dev)
            self.t_plb, self.t_pub = table(self.plb), table(self.pub)
            self.kw_batch = _lib.KwBatch(x_lo, x_hi, pw, pb, self.mask.data_ptr(), self.t_plb, self.t_pub, self.split.data_ptr(), ng)

    def children(self):
        """The child rows as ``ScorerEngine.frontier_commit`` takes them after the slots (the engine makes the gnnb_children of them)."""
        return self.mask, self.lb, self.ub, self.infeasible, self.bound, self.alpha, self.beta, self.ubv, self.live


class _StrongRows:
    """The child rows of a chunk of strong-branching candidates: what gnnb_frontier_expand writes and
    gnnb_kw_bounds / gnnb_dual_ascent read and write of n rows -- ``_Rows``' bounding side without the scorer's inputs, the LP point and
    the upper value, which no candidate gets; live, infeasible and bound are the run's (2n) arrays."""

    def __init__(self, eng, n, box):
        dev, R, sizes, ng = eng.device, eng.R, eng.sizes, len(eng.sizes)
        f64 = torch.float64
        self.mask = torch.zeros(n, R, dtype=torch.int8, device=dev)
        self.lb, self.ub, self.plb, self.pub = ([torch.zeros(n, s, dtype=f64, device=dev) for s in sizes[1:]] for _ in range(4))
        self.alpha, self.beta = torch.zeros(n, R, dtype=f64, device=dev), torch.zeros(n, R, dtype=f64, device=dev)
        self.split = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.box = box
        x_lo, x_hi, pw, pb = (t.data_ptr() for t in box)
        self.t_lb, self.t_ub, self.t_plb, self.t_pub = table(self.lb), table(self.ub), table(self.plb), table(self.pub)
        self.dual_batch = _lib.DualBatch(self.t_lb, self.t_ub, x_lo, x_hi, pw, pb, self.mask.data_ptr(), ng)
        self.kw_batch = _lib.KwBatch(x_lo, x_hi, pw, pb, self.mask.data_ptr(), self.t_plb, self.t_pub, self.split.data_ptr(), ng)


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


def _check_threshold(branching_threshold, kwbd_threshold):
    """The threshold mode's arguments (None: the mode is off)."""
    if branching_threshold is None:
        return
    if isinstance(branching_threshold, bool) or not isinstance(branching_threshold, (int, float)) or not 0 < branching_threshold <= 1:
        raise ValueError(f"branching_threshold = {branching_threshold!r}: None, or a number with 0 < branching_threshold <= 1")
    if not isinstance(kwbd_threshold, int) or isinstance(kwbd_threshold, bool) or kwbd_threshold < 0:
        raise ValueError(f"kwbd_threshold = {kwbd_threshold!r}: an integer >= 0")


KWBD_DEFAULT = 10                   # kwbd_threshold's default
KWBD_NEVER = 2 ** 31 - 1            # online mode: no count of inefficient points reaches it, every KW decision is bounded


def _check_online(online_threshold, branching_threshold, kwbd_threshold, choice):
    """The online mode's arguments (None: the mode is off), before a device is touched."""
    if online_threshold is None:
        return
    if not isinstance(online_threshold, int) or isinstance(online_threshold, bool) or online_threshold < 1:
        raise ValueError(f"online_threshold = {online_threshold!r}: None, or an integer >= 1")
    if branching_threshold is None:
        raise ValueError("online_threshold needs a branching_threshold: a parent learns from the KW decision the threshold mode bounds")
    if kwbd_threshold != KWBD_DEFAULT:
        raise ValueError(f"kwbd_threshold = {kwbd_threshold!r} with online_threshold: the online loop has no table of inefficient KW points "
                         "(reference plnn/relu_conv_online.py:166-177); leave kwbd_threshold at its default")
    from .graphnet.graph_score_online import GraphChoice
    if not isinstance(choice, GraphChoice):
        raise TypeError(f"online_threshold needs a graphnet.graph_score_online.GraphChoice (it owns the optimizer's lr / wd), not {type(choice).__name__}")


IMITATE_MARGIN_DEFAULT = 1.0


def _check_imitate(imitate, imitate_margin, branching, branching_threshold, online_threshold, choice):
    """The imitation options of DESIGN.md section 7.12 (None: off), before a device is touched."""
    replay = isinstance(imitate, Replay)
    if replay:
        _check_replay(imitate)
    elif imitate is not None and (not isinstance(imitate, int) or isinstance(imitate, bool) or imitate < 1):
        raise ValueError(f"imitate = {imitate!r}: None, an integer N >= 1 (every N-th round learns) or a Replay")
    if isinstance(imitate_margin, bool) or not isinstance(imitate_margin, (int, float)) or not imitate_margin >= 0:
        raise ValueError(f"imitate_margin = {imitate_margin!r}: a real number >= 0")
    if imitate is None:
        if imitate_margin != IMITATE_MARGIN_DEFAULT:
            raise ValueError(f"imitate_margin = {imitate_margin!r} without imitate: nothing would use it")
        return
    if branching == "babsr":
        raise ValueError('imitate with branching="babsr": a BaBSR run never prepares the GNN\'s inputs; imitate is legal with "gnn" and "strong"')
    if branching_threshold is not None or online_threshold is not None:
        raise ValueError("imitate takes no branching_threshold and no online_threshold: a round learns from one loss, the table's")
    if replay and imitate.steps == 0:                             # (collection only: no optimizer, any choice)
        return
    from .graphnet.graph_score_online import GraphChoice
    if not isinstance(choice, GraphChoice):
        raise TypeError(f"imitate needs a graphnet.graph_score_online.GraphChoice (it owns the optimizer's lr / wd), not {type(choice).__name__}")


BRANCHINGS = ("gnn", "babsr", "strong")
STRONG_CHUNK_DEFAULT = 256          # strong_chunk's default, candidates per bounding chunk: the best of 32..256 measured


REPACKS = ("host", "device")


def _check_repack(repack):
    """repack: where the scorer's operand packs are rebuilt after a learning step."""
    if not isinstance(repack, str) or repack not in REPACKS:
        raise ValueError(f"repack = {repack!r}: 'host' (the packs are rebuilt on the host, the step waits for the stream) or 'device' "
                         "(they are built on the stream, the step's status is read with the next round's state record)")


def _check_tighten(tighten_root):
    """tighten_root: the iterations of ``gnnb_kw_tighten`` on the root's intermediate bounds; 0: ``gnnb_kw_bounds``."""
    if isinstance(tighten_root, bool) or not isinstance(tighten_root, int) or tighten_root < 0:
        raise ValueError(f"tighten_root = {tighten_root!r}: an integer >= 0")


def _check_branching(branching, branching_threshold, online_threshold):
    """The branching mode, before a device is touched."""
    if not isinstance(branching, str) or branching not in BRANCHINGS:
        raise ValueError(f"branching = {branching!r}: one of {BRANCHINGS}")
    if branching == "babsr" and (branching_threshold is not None or online_threshold is not None):
        raise ValueError('branching="babsr" branches on the BaBSR heuristic alone (relu_bab): it takes no branching_threshold and no online_threshold, '
                         "which compare the heuristic with the GNN")
    if branching == "strong" and (branching_threshold is not None or online_threshold is not None):
        raise ValueError('branching="strong" branches where the bound improves most (DESIGN.md section 7.11): it takes no branching_threshold and no '
                         "online_threshold, which compare the heuristic with the GNN")


class Shortlist:
    """A value of ``strong_candidates`` that says where a parent's candidates come from.  babsr: None, or M >= 1,
    the M undecided nodes BaBSR ranks first -- ``Shortlist(babsr=M)`` is ``strong_candidates=M``.  gnn: None, or G >= 1, the G undecided
    nodes the run's own scorer ranks first (``gnnb_forward``'s scores of the parent rows), so that the GNN's decision always has an entry
    in the table.  Both: the union of the two sets (``gnnb_strong_list_union``).  At least one count must be given; the run checks them."""

    def __init__(self, babsr=None, gnn=None):
        self.babsr, self.gnn = babsr, gnn

    def __repr__(self):
        return f"Shortlist(babsr={self.babsr!r}, gnn={self.gnn!r})"


def _shortlist_counts(strong_candidates):
    """(M, G) of a checked ``strong_candidates``: BaBSR's count and the scorer's, 0 for none ((0, 0): every undecided node)."""
    if isinstance(strong_candidates, Shortlist):
        return strong_candidates.babsr or 0, strong_candidates.gnn or 0
    return strong_candidates or 0, 0


def _check_shortlist(s, branching, choice):
    """A ``Shortlist`` as the value of ``strong_candidates``, before a device is touched."""
    counts = (s.babsr, s.gnn)
    if s.babsr is None and s.gnn is None:
        raise ValueError(f"strong_candidates = {s!r}: a Shortlist needs a babsr count, a gnn count or both (None: every undecided node)")
    if any(c is not None and (not isinstance(c, int) or isinstance(c, bool) or c < 1) for c in counts):
        raise ValueError(f"strong_candidates = {s!r}: a count is None, or an integer >= 1")
    if s.gnn is None:
        return
    if branching == "babsr":
        raise ValueError(f'strong_candidates = {s!r} with branching="babsr": a BaBSR run never prepares the GNN\'s inputs, so there are no scores '
                         'to shortlist by; a gnn count is legal with "gnn" and "strong"')
    from .graphnet.graph_conv import GraphNet
    if not isinstance(getattr(choice, "model", None), GraphNet):
        raise ValueError(f"strong_candidates = {s!r}: a gnn count needs a choice whose model is a graphnet.graph_conv.GraphNet, the scorer to run, "
                         f"not {type(choice).__name__}")


REPLAY_BATCH_MAX = 256              # gnnb_replay_sample's n
REPLAY_CAPACITY_MAX = 65536         # gnnb_replay_push's C


class ReplayBuffer:
    """A device-resident ring of ``capacity`` labelled states of the network ``engine`` is bound to: a scorer
    batch of ``capacity`` rows -- exactly the tensors a learning step reads, ``batch`` is the ``_lib.Batch`` over them --, the
    strong-branching ``table`` (capacity, R) fp64 and the ``state`` word int32[4] = [head, filled, stored, skipped] on the device.
    ``head`` / ``filled`` / ``stored`` / ``skipped`` are the HOST's copy of that word as of the last ``read_state``.  engine: the engine
    whose handle runs the buffer's launches; any engine bound to the same network on the same device will do, and may be assigned."""

    def __init__(self, engine, capacity):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= REPLAY_CAPACITY_MAX:
            raise ValueError(f"ReplayBuffer: capacity = {capacity!r} (an integer in 1..{REPLAY_CAPACITY_MAX})")
        if getattr(engine, "sizes", None) is None:
            raise ValueError("ReplayBuffer: the engine has no network bound (ScorerEngine.bind)")
        self.engine, self.capacity, self.device = engine, capacity, engine.device
        self.sizes, self.R = list(engine.sizes), engine.R
        fixed = engine._net_keepalive
        n, dev, sizes, f32 = capacity, engine.device, self.sizes, torch.float32
        self.lb = [torch.zeros(n, s, dtype=f32, device=dev) for s in sizes]
        self.ub = [torch.zeros(n, s, dtype=f32, device=dev) for s in sizes]
        self.dual = [torch.zeros(n, 3 * s, dtype=f32, device=dev) for s in sizes[1:-1]]
        self.prims, self.prim_rows, k = [], [], 0
        for q, l in enumerate(fixed):                             # primals[q]: as ``_Rows`` holds them; the step reads those next to a ReLU
            nxt = fixed[q + 1] if q + 1 < len(fixed) else None
            if type(l) is nn.ReLU or type(nxt) is nn.ReLU:
                k += type(nxt) is nn.ReLU
                self.prims.append(torch.zeros(n, sizes[k], dtype=f32, device=dev))
                self.prim_rows.append(True)
            else:
                self.prims.append(torch.zeros(1, dtype=f32, device=dev))
                self.prim_rows.append(False)
        self.prims.append(torch.zeros(n, 1, dtype=f32, device=dev))
        self.prim_rows.append(True)
        self.x_lp = torch.zeros(n, sizes[0], dtype=f32, device=dev)
        self.prop_w = torch.zeros(n, sizes[-2], dtype=f32, device=dev)
        self.prop_b = torch.zeros(n, 1, dtype=f32, device=dev)
        self.mask = torch.zeros(n, self.R, dtype=f32, device=dev)
        self.table = torch.full((n, self.R), float("nan"), dtype=torch.float64, device=dev)
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)
        want = engine.replay_bytes(capacity)                      # the library's own list of the tensors a step reads
        have = sum(t.numel() * t.element_size() for t in self.row_tensors())
        if have != want:
            raise RuntimeError(f"ReplayBuffer: {have} bytes of row tensors, gnnb_replay_bytes says {want}")
        self._tables = [table(g) for g in (self.lb, self.ub, self.dual, self.prims)]
        self.batch = _lib.Batch(*self._tables, self.x_lp.data_ptr(), self.prop_w.data_ptr(), self.prop_b.data_ptr(), self.mask.data_ptr(),
                                len(self.lb), len(self.dual), len(self.prims))
        self.head = self.filled = self.stored = self.skipped = 0
        self._idx = torch.zeros(REPLAY_BATCH_MAX, dtype=torch.int32, device=dev)

    def row_tensors(self):
        """Every tensor with one row per slot, the table last: what ``split``, ``save`` and ``load`` move."""
        prims = [t for t, rows in zip(self.prims, self.prim_rows) if rows]
        return self.lb + self.ub + self.dual + prims + [self.x_lp, self.prop_w, self.prop_b, self.mask, self.table]

    def push(self, batch, K, rows, n, table, status=None):
        """``ScorerEngine.replay_push`` into this buffer: the useful ones of the rows ``rows[:n]`` of the K-row device batch ``batch`` and
        its (K, R) ``table``.  Device work only; ``read_state`` brings the counts over."""
        self.engine.replay_push(batch, K, rows, n, table, self.batch, self.capacity, self.table, self.state, status)

    def read_state(self):
        """The state word as [head, filled, stored, skipped]: the one 16-byte device-to-host copy.  Updates the host's copy."""
        st = self.state.cpu().tolist()
        self.head, self.filled, self.stored, self.skipped = st
        return st

    def _write_state(self, head, filled):
        self.head, self.filled, self.stored, self.skipped = head, filled, 0, 0
        self.state.copy_(torch.tensor([head, filled, 0, 0], dtype=torch.int32))

    def sample(self, n, seed, draw, out=None):
        """``ScorerEngine.replay_sample``: n (1..256) distinct filled slots of draw number ``draw`` under ``seed`` into ``out`` (None: the
        buffer's own index tensor), -1 beyond the filled part.  Device work only; returns the (n,) int32 device tensor."""
        out = self._idx[:n] if out is None else out
        self.engine.replay_sample(self.state, self.capacity, n, seed, draw, out)
        return out

    def step(self, n, margin, seed, draw, apply=True, loss=None, report=None, regret=None, status=None, out=None):
        """``sample`` and then ``ScorerEngine.imitation_step_rows`` on the sampled slots of the buffer's batch and table: one learning step
        on a minibatch (needs an engine with an optimizer).  Returns the sampled slots (device).  No host wait in repack mode "device"."""
        idx = self.sample(n, seed, draw, out)
        self.engine.imitation_step_rows(self.batch, self.capacity, idx, self.table, margin, loss=loss, report=report, regret=regret, status=status,
                                        apply=apply)
        return idx

    def evaluate(self, margin=1.0, chunk=64):
        """The numbers a step would report for every filled slot under the engine's current parameters, nothing applied: the
        ``apply=False`` step over the slots 0..filled - 1 in chunks.  Returns (loss (filled,) fp32, report (filled, 4) int32, regret
        (filled,) fp64) as CPU tensors."""
        self.read_state()
        n, dev = self.filled, self.device
        loss = torch.zeros(n, dtype=torch.float32, device=dev)
        report = torch.zeros(n, 4, dtype=torch.int32, device=dev)
        regret = torch.zeros(n, dtype=torch.float64, device=dev)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            self.engine.imitation_step_rows(self.batch, self.capacity, rows[a:b], self.table, margin, loss=loss[a:b], report=report[a:b],
                                            regret=regret[a:b], apply=False)
        return loss.cpu(), report.cpu(), regret.cpu()

    def order(self):
        """The filled slots from the oldest entry to the newest (host list; as of the last ``read_state``)."""
        return [(self.head - self.filled + i) % self.capacity for i in range(self.filled)]

    def split(self, fraction):
        """Offline: the newest floor(fraction * filled) entries move to a second buffer, which is returned (capacity: their number, 1 at
        least); this buffer keeps the others, oldest first from slot 0.  Torch indexing; reads the state first."""
        if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not 0 <= fraction <= 1:
            raise ValueError(f"split: fraction = {fraction!r} (a number in 0..1)")
        self.read_state()
        order = self.order()
        m = int(math.floor(fraction * self.filled))
        keep, move = order[:self.filled - m], order[self.filled - m:]
        other = ReplayBuffer(self.engine, max(1, m))
        dev = self.device
        ki, mi = torch.tensor(keep, dtype=torch.long, device=dev), torch.tensor(move, dtype=torch.long, device=dev)
        for mine, theirs in zip(self.row_tensors(), other.row_tensors()):
            theirs[:m] = mine[mi]
            mine[:len(keep)] = mine[ki]
        other._write_state(m % other.capacity, m)
        self._write_state(len(keep) % self.capacity, len(keep))
        return other

    def save(self, path):
        """The buffer as a file: its row tensors (CPU), the state word and the bound network's layer sizes."""
        self.read_state()
        torch.save({"format": "gnnb_replay_buffer/1", "sizes": self.sizes, "R": self.R, "capacity": self.capacity,
                    "widths": [int(t.shape[1]) for t in self.row_tensors()], "state": [self.head, self.filled, self.stored, self.skipped],
                    "tensors": [t.cpu() for t in self.row_tensors()]}, path)

    @classmethod
    def load(cls, engine, path):
        """The buffer of a ``save`` file on the network ``engine`` is bound to; a file from another network is a ValueError."""
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("format") != "gnnb_replay_buffer/1":
            raise ValueError(f"ReplayBuffer.load: {path} is no replay buffer file")
        if getattr(engine, "sizes", None) is None:
            raise ValueError("ReplayBuffer.load: the engine has no network bound (ScorerEngine.bind)")
        if list(d["sizes"]) != list(engine.sizes) or d["R"] != engine.R:
            raise ValueError(f"ReplayBuffer.load: {path} holds states of a network with layer sizes {list(d['sizes'])}, "
                             f"the engine is bound to {list(engine.sizes)}")
        buf = cls(engine, int(d["capacity"]))
        mine = buf.row_tensors()
        if [int(t.shape[1]) for t in mine] != list(d["widths"]):
            raise ValueError(f"ReplayBuffer.load: {path} holds rows of other widths than the bound network's")
        for t, src in zip(mine, d["tensors"]):
            t.copy_(src)
        st = [int(v) for v in d["state"]]
        buf._write_state(st[0], st[1])
        return buf


class Replay:
    """A value of ``imitate`` that keeps the labelled states.  every: N >= 1, every N-th launched round is a
    learning round, as ``imitate=N``.  A learning round pushes its parent rows and their table into ``buffer`` (None: the run makes a
    ``ReplayBuffer`` of ``capacity`` slots; ``run.buffer`` is it) and then takes ``steps`` steps, each on min(batch, filled) entries
    drawn afresh under ``seed`` with a draw counter that runs through the whole run.  steps = 0 only collects: no optimizer, no
    parameter moves, any choice."""

    def __init__(self, every, buffer=None, capacity=1024, batch=8, steps=1, seed=0):
        self.every, self.buffer, self.capacity, self.batch, self.steps, self.seed = every, buffer, capacity, batch, steps, seed

    def __repr__(self):
        return (f"Replay(every={self.every!r}, buffer={'None' if self.buffer is None else 'ReplayBuffer'}, capacity={self.capacity!r}, "
                f"batch={self.batch!r}, steps={self.steps!r}, seed={self.seed!r})")


def _check_replay(r):
    """A ``Replay`` as the value of ``imitate``, before a device is touched."""
    def count(v, least):
        return isinstance(v, int) and not isinstance(v, bool) and v >= least
    if not count(r.every, 1) or not count(r.capacity, 1) or not count(r.batch, 1):
        raise ValueError(f"imitate = {r!r}: every, capacity and batch are integers >= 1")
    if not count(r.steps, 0):
        raise ValueError(f"imitate = {r!r}: steps is an integer >= 0 (0: collect only)")
    if not count(r.seed, 0) or r.seed >= 2 ** 64:
        raise ValueError(f"imitate = {r!r}: seed is an integer in 0..2^64 - 1")
    if r.buffer is not None and not isinstance(r.buffer, ReplayBuffer):
        raise ValueError(f"imitate = {r!r}: buffer is None or a ReplayBuffer, not {type(r.buffer).__name__}")
    capacity = r.capacity if r.buffer is None else r.buffer.capacity
    if capacity > REPLAY_CAPACITY_MAX:
        raise ValueError(f"imitate = {r!r}: capacity {capacity} > {REPLAY_CAPACITY_MAX}")
    if r.batch > REPLAY_BATCH_MAX:
        raise ValueError(f"imitate = {r!r}: batch {r.batch} > {REPLAY_BATCH_MAX}, the most one draw holds")
    if r.batch > capacity:
        raise ValueError(f"imitate = {r!r}: batch {r.batch} > capacity {capacity}")


def _check_strong(strong_candidates, strong_chunk, strong_audit, branching, branching_threshold, online_threshold, imitate=None, choice=None):
    """The strong-branching options of DESIGN.md sections 7.11 and 7.14, before a device is touched."""
    if isinstance(strong_candidates, Shortlist):
        _check_shortlist(strong_candidates, branching, choice)
    elif strong_candidates is not None and (not isinstance(strong_candidates, int) or isinstance(strong_candidates, bool) or strong_candidates < 1):
        raise ValueError(f"strong_candidates = {strong_candidates!r}: None (every undecided node), or an integer >= 1")
    if not isinstance(strong_chunk, int) or isinstance(strong_chunk, bool) or strong_chunk < 1:
        raise ValueError(f"strong_chunk = {strong_chunk!r}: an integer >= 1, the candidates per bounding chunk")
    if strong_audit is not None and not isinstance(strong_audit, list):
        raise ValueError(f"strong_audit = {strong_audit!r}: None, or a list that receives one dict per parent")
    if branching != "strong" and strong_audit is None and imitate is None:
        if strong_candidates is not None:
            raise ValueError(f'strong_candidates = {strong_candidates!r} without branching="strong", a strong_audit or imitate: nothing would use it')
        if strong_chunk != STRONG_CHUNK_DEFAULT:
            raise ValueError(f'strong_chunk = {strong_chunk!r} without branching="strong", a strong_audit or imitate: nothing would use it')
    if strong_audit is not None and (branching_threshold is not None or online_threshold is not None):
        raise ValueError("strong_audit audits the one decision a round commits per parent: it takes no branching_threshold and no online_threshold")


PGD_STEP_DEFAULT = 1.0 / 64


def _check_witness(witness, pgd_steps, pgd_step):
    """The witness and descent options (None: off), before a device is touched."""
    if witness is not None and not isinstance(witness, list):
        raise ValueError(f"witness = {witness!r}: None, or a list that receives the point")
    if pgd_steps is not None and (not isinstance(pgd_steps, int) or isinstance(pgd_steps, bool) or pgd_steps < 0):
        raise ValueError(f"pgd_steps = {pgd_steps!r}: None, or an integer >= 0")
    if isinstance(pgd_step, bool) or not isinstance(pgd_step, (int, float)) or not 0 < pgd_step <= 1:
        raise ValueError(f"pgd_step = {pgd_step!r}: a number with 0 < pgd_step <= 1")


def _check_restarts(pgd_restarts, pgd_seed, pgd_steps):
    """The restart options of DESIGN.md section 7.9 (None: off), before a device is touched."""
    if pgd_restarts is not None and (not isinstance(pgd_restarts, int) or isinstance(pgd_restarts, bool) or pgd_restarts < 0):
        raise ValueError(f"pgd_restarts = {pgd_restarts!r}: None, or an integer >= 0")
    if pgd_restarts is not None and pgd_restarts > PGD_RESTARTS_MAX:
        raise ValueError(f"pgd_restarts = {pgd_restarts!r}: {PGD_RESTARTS_MAX} at most")
    if pgd_restarts is not None and pgd_steps is None:
        raise ValueError(f"pgd_restarts = {pgd_restarts!r} needs pgd_steps (0: the random starts and the LP point, no descent)")
    if not isinstance(pgd_seed, int) or isinstance(pgd_seed, bool) or not 0 <= pgd_seed < 2 ** 64:
        raise ValueError(f"pgd_seed = {pgd_seed!r}: an integer in 0..2^64 - 1")


PGD_RESTARTS_MAX = 4096             # gnnb_net_starts' R
SPLIT_DEPTH_MAX = 8                 # gnnb_frontier_expand_depth's depth


def _check_split_depth(split_depth, branching="gnn", branching_threshold=None, online_threshold=None, imitate=None, strong_audit=None,
                       strong_candidates=None):
    """``lp.split_depth`` (None: off) and what it does not go with, before a device is touched.  A parent's 2^d children
    come from ONE list of its d nodes, the scorer's: a mode that names one node per parent by another rule (BaBSR, the strong table), that
    compares two PAIRS of children (the threshold and online modes) or that labels one decision per parent (imitate, an audit, a
    ``Shortlist``) has no meaning for them yet."""
    if split_depth is None:
        return
    if isinstance(split_depth, bool) or not isinstance(split_depth, int) or not 1 <= split_depth <= SPLIT_DEPTH_MAX:
        raise ValueError(f"split_depth = {split_depth!r}: None, or an integer in 1..{SPLIT_DEPTH_MAX} (a bool is refused)")
    if branching != "gnn":
        raise ValueError(f'split_depth with branching={branching!r}: the nodes of a deep split are the ones the GNN scores highest; only branching="gnn"')
    for name, value in (("branching_threshold", branching_threshold), ("online_threshold", online_threshold), ("imitate", imitate),
                        ("strong_audit", strong_audit)):
        if value is not None:
            raise ValueError(f"split_depth takes no {name}: it compares or labels the two children of ONE decision per parent")
    if isinstance(strong_candidates, Shortlist):
        raise ValueError(f"split_depth takes no Shortlist (strong_candidates = {strong_candidates!r}): the run's one candidate list holds the nodes of the split")


class _Round:
    """What a one-job and a many-job run share: the rows of a round, and the existing batch entry points on them."""
    branching, strong_on, imitate, learning = "gnn", False, None, False      # (what a run is before ``_set_options``: everything off)
    strong_G, cand_src = 0, None    # (section 7.14: the scorer's count of a ``Shortlist`` and the union's sources; off unless a run sets them)
    repack, pending_step = "host", None      # (section 7.15: "device" where a run asks for it; the step whose status has not been read yet)
    replay, last_replay = None, None         # (section 7.16: the ``Replay`` of a run whose ``imitate`` is one; what its last learning round did)
    online, learn_pending = None, False      # (sections 7.7 and 7.19: the online threshold of a run that learns online; a selection not yet read)
    last_learn = online_steps = online_rows = 0      # (the learn rows of the last round that read them; the steps of the run and their rows)
    tighten_root = 0                         # (section 7.18: iterations of gnnb_kw_tighten on the roots' intermediate bounds; 0: gnnb_kw_bounds)
    split_depth, depth = None, 0             # (section 7.20: the most nodes a parent is split on in one round; the launched round's d, 0: the two-children round)

    def _set_options(self, choice, *, branching="gnn", branching_threshold=None, kwbd_threshold=KWBD_DEFAULT, sparsest_layer=0, decision_threshold=0.001,
                     online_threshold=None, witness=None, pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None, pgd_seed=0, imitate=None,
                     imitate_margin=IMITATE_MARGIN_DEFAULT, strong_candidates=None, strong_chunk=STRONG_CHUNK_DEFAULT, strong_audit=None,
                     repack="host"):
        """The options of a run, checked in ONE order -- imitate, branching, strong, witness, restarts, threshold, online, repack -- and stored with
        everything derived from them, before anything touches ``choice`` or a device; a constructor passes the keywords it has and the
        others stay off.  Everything behind it (``_engine_of``, ``_buffers``, ``_launch``, the loops) reads the run, never an argument:
        ``strong_on`` (a round computes the table of section 7.11: "strong", an audit, or ``imitate``), ``strong_M`` (BaBSR's count; 0: none) and
        ``strong_G`` (the scorer's count of a ``Shortlist``, section 7.14; both 0: every undecided node), ``witness_on`` and ``witness_to`` (the caller's list), ``restarts`` (0: off), ``threshold``, ``online``, ``learns`` (the
        scorer's parameters move: the run takes the engine with the optimizer), and the counters of a run before its first round."""
        _check_imitate(imitate, imitate_margin, branching, branching_threshold, online_threshold, choice)
        _check_branching(branching, branching_threshold, online_threshold)
        _check_strong(strong_candidates, strong_chunk, strong_audit, branching, branching_threshold, online_threshold, imitate, choice)
        _check_witness(witness, pgd_steps, pgd_step)
        _check_restarts(pgd_restarts, pgd_seed, pgd_steps)
        _check_threshold(branching_threshold, kwbd_threshold)
        _check_online(online_threshold, branching_threshold, kwbd_threshold, choice)
        _check_repack(repack)
        if repack != "host":                                      # (set only where given, as strong_G)
            self.repack = repack
        self.branching, self.threshold, self.online = branching, branching_threshold, online_threshold
        self.kwbd_threshold = kwbd_threshold if online_threshold is None else KWBD_NEVER
        self.sparsest_layer, self.decision_threshold = sparsest_layer, decision_threshold
        if branching_threshold is not None or branching == "babsr":      # (the BaBSR heuristic's: converted where a round uses them)
            self.sparsest_layer, self.decision_threshold = int(sparsest_layer), float(decision_threshold)
        self.witness_on, self.witness_to, self.pgd_steps, self.pgd_step = witness is not None, witness, pgd_steps, float(pgd_step)
        self.restarts, self.pgd_seed = pgd_restarts or 0, pgd_seed
        self.imitate, self.imitate_margin = imitate, float(imitate_margin)
        replay = imitate if isinstance(imitate, Replay) else None
        if replay is not None:                                    # (set only where given, as strong_G: section 7.16)
            self.replay, self.buffer = replay, None
        self.learns = online_threshold is not None or (imitate is not None and (replay is None or replay.steps > 0))      # (steps = 0 only collects)
        self.strong_on = branching == "strong" or strong_audit is not None or imitate is not None
        self.strong_M, G = _shortlist_counts(strong_candidates)
        self.strong_chunk, self.strong_audit = strong_chunk, strong_audit
        if G:                                                     # (set only where given: without a gnn count a run is the run it was)
            self.strong_G = G
        self.round = self.k = self.strong_n = self.imitation_steps = self.imitation_rows = self.last_imitation = 0
        self.learning, self.imitate_pending, self.cand_entry, self.im_table = False, False, None, None

    def _engine_of(self, choice):
        """The engine of the run: the model's, or for a run that learns (online or by imitation) ``choice._eng()``, the engine with its
        optimizer."""
        return choice._eng() if self.learns else choice.model.engine()

    def _use_repack(self):
        """Behind ``_engine_of``: a run that learns puts its engine into the run's repack mode.  The engine outlives the run, so every
        such run sets the mode, "host" included (``close`` puts it back when the run ends)."""
        if self.learns:
            self.eng.set_repack(self.repack)

    def close(self):
        """The end of a run for whoever drives a run class directly (``branch_and_bound_frontier`` and the ``verify_properties*`` call it):
        the engine, which outlives the run, goes back to repack mode "host"."""
        if self.learns and self.repack != "host":
            self.eng.set_repack("host")

    def _step_issued(self, keep=()):
        """Behind a learning step in "device" mode: the step was only issued.  Its status word, and what the trace shows of it, are read
        with the NEXT round's state record or at the end of the run (``_settle_step``).  keep: names of device tensors the next launch
        overwrites before that read; the trace then reads copies made here, on the stream."""
        if self.repack == "device":
            self.pending_step = {"round": self.round, "fill": [], "kept": {name: getattr(self, name).clone() for name in keep}}

    def _settle_step(self):
        """The deferred half of a "device"-mode learning step, behind a read that has already waited for the stream: the step's status
        word (bit 3 raises, naming the round that learnt) and the trace entries of that round."""
        p, self.pending_step = self.pending_step, None
        if p is None:
            return
        if int(self.step_status.cpu()[0]) & 8:
            raise RuntimeError(f"{self._refusal()} -- in the learning step of round {p['round']}")
        for fill in p["fill"]:
            fill(p["kept"])

    def _refusal(self):
        """What status bit 3 of the run's learning step means: the imitation step's text, or the online step's (``_raise_for`` raises the
        same text for a run that reads it at its end)."""
        if self.imitate is None:
            return "gnnb_online_step_rows refused a learn row (status bit 3): its KW decision names no undecided node of the row's mask"
        return ("gnnb_imitation_step_rows refused a row (status bit 3): its table names a candidate that is no undecided node of the "
                "row's mask, or holds an infinite improvement")

    def _witness_buffers(self, segments):
        """Per segment the incumbent's value (+inf: none yet; the record's global_ub after every commit) and its point."""
        if self.witness_on:
            dev = self.eng.device
            self.best_value = torch.full((segments,), float("inf"), dtype=torch.float64, device=dev)
            self.best_point = torch.zeros(segments, self.eng.sizes[0], dtype=torch.float32, device=dev)

    def _buffers(self, n_parents, n_children, in_shape, parent_side):
        """The rows and workspaces of a round of up to n_parents parents.  self.x_lo / x_hi / pw / pb: the children's boxes and property
        rows; parent_side: the parents' (the same tensors when every row has one box and one property)."""
        eng, dev, ws = self.eng, self.eng.device, self._ws
        self.in_shape = in_shape
        self.P = _Rows(eng, self.fixed, n_parents, in_shape, parent_side, child=False)
        self.Ch = self._child_rows(n_children)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.status_all = torch.zeros(1, dtype=torch.int32, device=dev)
        self.root_slot = torch.zeros(1, dtype=torch.int32, device=dev)
        # (a BaBSR or strong round runs no gnnb_forward, unless the scorer shortlists the candidates: section 7.14)
        self.ws_fwd = ws("gnnb_workspace_bytes", n_parents) if self.branching == "gnn" or self.strong_G else None
        n_bound = max(n_children, 2 * self.strong_chunk) if self.strong_on else n_children      # (the candidates' chunks share the workspaces)
        self.ws_kw = ws("gnnb_kw_workspace_bytes", n_bound)
        self.ws_dual = ws("gnnb_dual_workspace_bytes", n_bound)
        self.ws_eval, self.ws_commit = ws("gnnb_net_eval_workspace_bytes", n_children), ws("gnnb_frontier_commit_workspace_bytes", n_parents)
        if self.pgd_steps is not None:
            self.ws_descend = ws("gnnb_net_descend_workspace_bytes", n_children)
        if self.restarts:                                         # every row's start points, and the tiles' workspace
            n_starts = self.restarts + 1
            self.starts = torch.zeros(n_children, n_starts, eng.sizes[0], dtype=torch.float32, device=dev)
            self.ws_starts = torch.empty(max(1, self.lib.gnnb_net_descend_starts_workspace_bytes(eng.h, n_children, n_starts)), dtype=torch.uint8, device=dev)
        self.keep_pairs, self.pair_a = False, None

    def set_tighten_root(self, n):
        """DESIGN.md section 7.18, before the first root phase: the roots' intermediate bounds come from ``gnnb_kw_tighten`` at n iterations
        (0: ``gnnb_kw_bounds``, and nothing is allocated).  The workspace is sized for the largest root phase (``root_rows``); no round uses it."""
        _check_tighten(n)
        self.tighten_root = n
        if n:
            self.ws_tighten = self._ws("gnnb_kw_tighten_workspace_bytes", self.root_rows)

    def _ws(self, sizer, B):
        return torch.empty(max(1, getattr(self.lib, sizer)(self.eng.h, B)), dtype=torch.uint8, device=self.eng.device)

    def _child_rows(self, n_children, box=None):
        """A set of child rows on the children's boxes and property rows (box: its own, where its rows belong to other jobs than the
        children's).  A second set (pair B of the threshold mode) shares the workspaces: everything is
        stream-ordered, so the two pairs never use one at the same time."""
        rows = _Rows(self.eng, self.fixed, n_children, self.in_shape, (self.x_lo, self.x_hi, self.pw, self.pb) if box is None else box, child=True)
        if self.pgd_steps is not None:                            # the points ubv is the network's value at (x_lp stays the LP's)
            rows.x_ub = torch.zeros_like(rows.x_lp)
        return rows

    def _threshold_buffers(self, n_parents, counters, box_b, ws_sizer):
        """The threshold mode's state for rounds of up to n_parents parents (DESIGN.md sections 7.5 and 7.6).  counters: the shapes of the
        intercept counters ``icp`` (and of ``n_used``, the KW pairs taken) and of the tables ``ineff`` of inefficient KW points; box_b: pair
        B's own boxes and property rows (None: the children's); ws_sizer: the selection's workspace sizer."""
        dev, R, n = self.eng.device, self.eng.R, n_parents
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        self.random_order = _random_order(self.ng - 2, self.sparsest_layer)
        self.icp, self.ineff = torch.zeros(counters[0], dtype=i32, device=dev), torch.zeros(counters[1], dtype=i32, device=dev)
        self.n_used = torch.zeros(counters[0], dtype=torch.int64, device=dev)
        self.ChB = self._child_rows(2 * n, box_b)
        self.kw_scores, self.kw_icp = torch.zeros(n, R, dtype=f32, device=dev), torch.zeros(n, R, dtype=f32, device=dev)
        self.gnn_imp, self.kw_imp = torch.zeros(n, dtype=f64, device=dev), torch.zeros(n, dtype=f64, device=dev)
        self.kw_dec, self.sel_dec, self.dec = (torch.zeros(n, 2, dtype=i32, device=dev) for _ in range(3))
        self.sel_rows, self.sel_slots, self.used_kw = (torch.zeros(n, dtype=i32, device=dev) for _ in range(3))
        self.ws_fallback = self._ws(ws_sizer, n)

    def _babsr_buffers(self, n_parents, counters):
        """The state of ``branching="babsr"`` for rounds of up to n_parents parents.  counters: the shape of the
        intercept counters ``icp`` (one per run, or one per segment)."""
        dev, R, f32 = self.eng.device, self.eng.R, torch.float32
        self.random_order = _random_order(self.ng - 2, self.sparsest_layer)
        self.icp = torch.zeros(counters, dtype=torch.int32, device=dev)
        self.kw_scores, self.kw_icp = torch.zeros(n_parents, R, dtype=f32, device=dev), torch.zeros(n_parents, R, dtype=f32, device=dev)
        self.ws_babsr = self._ws("gnnb_frontier_babsr_decide_workspace_bytes", n_parents)

    def _strong_buffers(self, n_parents, box):
        """The state of strong branching for rounds of up to n_parents parents.  box: the boxes and property rows
        of the 2 * strong_chunk candidate child rows ``ChS``.  The dense lists hold n_parents * min(R, M + G or R) candidates (M, G:
        BaBSR's count and the scorer's, section 7.14) and the run-long arrays live / infeasible / bound two children each; BaBSR's scores
        exist only with M, the union's ``cand_src`` and workspace only with both counts; ``strong_bounded`` counts the candidate children
        bounded."""
        dev, R, n = self.eng.device, self.eng.R, n_parents
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        top, union = self.strong_M + self.strong_G, self.strong_M > 0 and self.strong_G > 0
        cap = n * (min(R, top) if top else R)
        self.ChS = _StrongRows(self.eng, 2 * self.strong_chunk, box)
        self.s_scores, self.s_icp = (torch.zeros(n, R, dtype=f32, device=dev) for _ in range(2)) if self.strong_M else (None, None)
        self.cand0 = torch.zeros(n + 1, dtype=i32, device=dev)
        self.cand_row, self.cand_slot, self.cand_dec = (torch.zeros(s, dtype=i32, device=dev) for s in ((cap,), (cap,), (cap, 2)))
        self.s_live, self.s_infeasible = torch.zeros(2 * cap, dtype=i32, device=dev), torch.zeros(2 * cap, dtype=i32, device=dev)
        self.s_bound, self.s_imp = torch.zeros(2 * cap, dtype=f64, device=dev), torch.zeros(cap, dtype=f64, device=dev)
        self.s_best, self.s_dec = torch.zeros(n, dtype=f64, device=dev), torch.zeros(n, 2, dtype=i32, device=dev)
        self.ws_strong = self._ws("gnnb_strong_list_union_workspace_bytes" if union else "gnnb_strong_list_workspace_bytes", n)
        if union:
            self.cand_src = torch.zeros(cap, dtype=i32, device=dev)
        self.strong_bounded = 0

    def _depth_buffers(self, n_parents):
        """The state of a run with ``split_depth`` = D for rounds of up to n_parents parents: the candidate lists
        ``gnnb_strong_list`` writes at top_m = d <= D and its workspace.  The child side keeps its size: a round has k 2^d <= 2K child rows,
        and the commit's workspace is sized by the rows."""
        if self.split_depth is None:
            return
        dev, n, i32 = self.eng.device, n_parents, torch.int32
        cap = n * min(self.eng.R, self.split_depth)
        self.cand0 = torch.zeros(n + 1, dtype=i32, device=dev)
        self.cand_row, self.cand_slot, self.cand_dec = (torch.zeros(s, dtype=i32, device=dev) for s in ((cap,), (cap,), (cap, 2)))
        self.ws_strong = self._ws("gnnb_strong_list_workspace_bytes", n)

    def _imitation_buffers(self, n_parents):
        """The state of a run with ``imitate`` for learning rounds of up to n_parents parent rows: the table a
        learning round keeps, the rows its step takes (all of them, in row order) and what the step reports per row."""
        if self.imitate is None:
            return
        dev, n = self.eng.device, n_parents
        self.im_table = torch.zeros(n, self.eng.R, dtype=torch.float64, device=dev)
        self.im_rows = torch.arange(n, dtype=torch.int32, device=dev)
        self.im_loss, self.im_regret = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        self.im_report = torch.zeros(n, 4, dtype=torch.int32, device=dev)
        self.step_status = torch.zeros(1, dtype=torch.int32, device=dev)
        rp = self.replay
        if rp is None:
            return
        # section 7.16: the buffer (the caller's, or the run's own), the word a push reports refused rows in, per step of a learning
        # round the drawn slots and what the step reports of them, and the run's draw counter and totals
        buf = rp.buffer
        if buf is None:
            buf = ReplayBuffer(self.eng, rp.capacity)
        elif buf.sizes != list(self.eng.sizes) or buf.device != dev:
            raise ValueError(f"imitate = {rp!r}: the buffer holds states of a network with layer sizes {buf.sizes} on {buf.device}, the run's "
                             f"has {list(self.eng.sizes)} on {dev}")
        else:
            buf.engine = self.eng
        if n_parents > buf.capacity:
            raise ValueError(f"imitate = {rp!r}: a round has up to {n_parents} parent rows, the buffer {buf.capacity} slots; one push takes "
                             "at most as many rows as the buffer holds")
        self.buffer, S, b = buf, max(1, rp.steps), rp.batch
        self.push_status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rp_idx = torch.full((S, b), -1, dtype=torch.int32, device=dev)
        self.rp_loss, self.rp_regret = torch.zeros(S, b, dtype=torch.float32, device=dev), torch.zeros(S, b, dtype=torch.float64, device=dev)
        self.rp_report = torch.zeros(S, b, 4, dtype=torch.int32, device=dev)
        self.draw = self.replay_stored = self.replay_skipped = self.replay_filled = 0

    def _begin_round(self, k):
        """The top of ``launch_round``: launched round number ``round`` of the run (1-based; root phases do not count), of k parent rows over
        all its entries.  With ``imitate`` = N it is a learning round when that number is a multiple of N: its table stays, and its step
        runs behind the read of the state.  No candidate has been counted yet (``cand_entry``)."""
        self.round += 1
        every = self.replay.every if self.replay is not None else self.imitate
        self.learning = self.imitate_pending = every is not None and self.round % every == 0
        self.k, self.last_imitation, self.cand_entry, self.last_replay = k, 0, None, None

    def _step_behind_read(self):
        """Behind the read of the state: a learning round takes its step (``_imitate``)."""
        if self.imitate_pending:
            self._imitate()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def read_candidates(self, n):
        """cand0[n], the number of candidates of a round of n parents: the 4 bytes a strong round reads between the list and its chunks.
        ``cand_entry`` keeps it as the candidate range of the round's one entry."""
        self.cand_entry = [0, int(self.cand0[n:n + 1].cpu()[0])]
        return self.cand_entry[-1]

    def _strong_table(self, slots, n, dec, table=None):
        """Steps 2-6 of a strong round over the n parent rows the gather wrote: gnnb_babsr for the pre-filter (with
        a BaBSR count), gnnb_strong_list on BaBSR's scores or on the scorer's (``P.scores``, with a gnn count alone) or
        gnnb_strong_list_union on both (section 7.14), the read of the number of candidates, per chunk of ``strong_chunk`` candidates
        gnnb_frontier_expand into ``ChS``, gnnb_kw_bounds and gnnb_dual_ascent (no scorer inputs, no LP point; live, infeasible and bound go
        to the run-long arrays at the chunk's offset), and gnnb_strong_pick into ``dec`` ((n, 2) int32) and, on a learning round (section
        7.12), into ``table`` ((n, R) fp64).  No gnnb_net_eval, no PGD, no witness: a candidate is only ever a lower bound."""
        P, S, eng, pool, lib, h = self.P, self.ChS, self.eng, self.pool, self.lib, self.eng.h
        M, G = self.strong_M, self.strong_G
        lists = (self.cand0, self.cand_row, self.cand_slot, self.cand_dec)
        if M:
            eng.babsr_rows(P.lb32, P.ub32, P.box[2], P.amb, n, self.s_scores, self.s_icp)
        if M and G:                                               # (section 7.14: P.scores are the round's gnnb_forward's, already there)
            eng.strong_list_union(pool, slots, P.amb, self.s_scores, M, P.scores, G, *lists, self.cand_src, workspace=self.ws_strong)
        elif G:
            eng.strong_list(pool, slots, P.amb, P.scores, G, *lists, workspace=self.ws_strong)
        else:
            eng.strong_list(pool, slots, P.amb, self.s_scores, M, *lists, workspace=self.ws_strong)
        n_c = self.strong_n = self.read_candidates(n)
        for q0 in range(0, n_c, self.strong_chunk):               # a chunk may span parents
            c = min(self.strong_chunk, n_c - q0)
            self._strong_chunk_rows(q0, c)
            eng.frontier_expand(pool, self.cand_slot[q0:q0 + c], self.cand_dec[q0:q0 + c], S.mask, S.plb, S.pub, S.split, S.alpha, S.beta,
                                self.s_live[2 * q0:])
            with torch.cuda.device(eng.device):
                _lib.check(lib.gnnb_kw_bounds(h, C.byref(S.kw_batch), 2 * c, S.t_lb, S.t_ub, None, None, self.s_infeasible[2 * q0:].data_ptr(),
                                              self.ws_kw.data_ptr(), self.ws_kw.numel(), self._stream()), "gnnb_kw_bounds")
                _lib.check(lib.gnnb_dual_ascent(h, C.byref(S.dual_batch), 2 * c, self.n_iter, self.lr, S.alpha.data_ptr(), S.beta.data_ptr(), 1,
                                                self.s_bound[2 * q0:].data_ptr(), None, None, None, None, None, None, self.ws_dual.data_ptr(),
                                                self.ws_dual.numel(), self._stream()), "gnnb_dual_ascent")
        self.strong_bounded += 2 * n_c
        eng.strong_pick(pool, slots, self.cand0, self.cand_dec, n_c, self.s_live, self.s_infeasible, self.s_bound, dec, self.s_best, self.s_imp, table)

    def _strong_chunk_rows(self, q0, c):
        """The boxes and property rows of ``ChS`` for the chunk of candidates [q0, q0 + c), in front of its gnnb_frontier_expand.  A
        one-job run has nothing to do: every row holds the run's one box and property, filled once.  ``StrongJobsRun`` (DESIGN.md section
        7.13) copies each candidate's own job's."""

    def _strong_parents(self, n):
        """``branching="strong"`` in ``_score_parents``' place: the table of the n parent rows the gather wrote and
        its arg-max per row into ``P.dec``.  No gnnb_dual_ascent at n_iter = 0, no gnnb_forward.  A learning round (section 7.12) keeps the
        table and then runs gnnb_dual_ascent at n_iter = 0 on the parent rows, so that the scorer inputs the step reads exist; still no
        gnnb_forward.  With a gnn count (section 7.14) the scorer shortlists the candidates: ``_score_parents`` runs in front of the list
        (its decisions in ``P.dec`` are overwritten by the pick), and a learning round has its scorer inputs from that one ascent."""
        if self.strong_G:
            self._score_parents(n)
        self._strong_table(self.slots[:n], n, self.P.dec, self.im_table if self.learning else None)      # (a one-job run's slots are its n)
        if self.learning and not self.strong_G:
            self._scorer_inputs(n)

    def _bound_children(self, Ch, B, warm, tighten=0):
        """gnnb_kw_bounds (with ``tighten`` = n > 0, the root phase's: gnnb_kw_tighten at n iterations),
        gnnb_dual_ascent and gnnb_net_eval over the first B rows of the child rows ``Ch``.  With ``pgd_steps``
        gnnb_net_descend from the rows' x_lp takes gnnb_net_eval's place: its f(x0) is that value, ubv the best value
        it reached and x_ub the point.  With ``pgd_restarts`` gnnb_net_starts and gnnb_net_descend_starts take its place in turn (section 7.9):
        the descent from the LP point and from ``restarts`` uniform points of the row's box, ubv the least of their best values."""
        lib, h = self.lib, self.eng.h
        with torch.cuda.device(self.eng.device):
            if tighten:
                _lib.check(lib.gnnb_kw_tighten(h, C.byref(Ch.kw_batch), B, tighten, self.lr, Ch.t_lb, Ch.t_ub, None, None, Ch.infeasible.data_ptr(), None,
                                               self.ws_kw.data_ptr(), self.ws_kw.numel(), self.ws_tighten.data_ptr(), self.ws_tighten.numel(),
                                               self._stream()), "gnnb_kw_tighten")
            else:
                _lib.check(lib.gnnb_kw_bounds(h, C.byref(Ch.kw_batch), B, Ch.t_lb, Ch.t_ub, None, None, Ch.infeasible.data_ptr(), self.ws_kw.data_ptr(),
                                              self.ws_kw.numel(), self._stream()), "gnnb_kw_bounds")
            _lib.check(lib.gnnb_dual_ascent(h, C.byref(Ch.dual_batch), B, self.n_iter, self.lr, Ch.alpha.data_ptr(), Ch.beta.data_ptr(), int(warm),
                                            Ch.bound.data_ptr(), None, None, Ch.t_dual, Ch.t_prims, Ch.x_lp.data_ptr(), None, self.ws_dual.data_ptr(),
                                            self.ws_dual.numel(), self._stream()), "gnnb_dual_ascent")
        if self.pgd_steps is None:
            self.eng.net_eval(self.fixed, None, Ch.x_lp[:B], out=Ch.ubv, prop=Ch.box[2:], workspace=self.ws_eval)
        elif not self.restarts:
            self.eng.net_descend(self.fixed, None, Ch.x_lp[:B], Ch.box[0], Ch.box[1], self.pgd_steps, self.pgd_step, x_best=Ch.x_ub, value=Ch.ubv,
                                 prop=Ch.box[2:], workspace=self.ws_descend)
        else:                                                     # the seed of every launch is pgd_seed: rows differ through their keys
            self.eng.net_starts(self.fixed, Ch.x_lp[:B], Ch.box[0], Ch.box[1], self.restarts, self.pgd_seed, starts=self.starts)
            self.eng.net_descend_starts(self.fixed, None, self.starts[:B], Ch.box[0], Ch.box[1], self.pgd_steps, self.pgd_step, x_best=Ch.x_ub,
                                        value=Ch.ubv, prop=Ch.box[2:], workspace=self.ws_starts, in_shape=self.in_shape)

    def _at_least_the_parent_s(self, Ch, slots, n, C=2):
        """Behind the bounding of the C n children of the n parents in ``slots`` (C = 2 but in a round of section 7.20): a child's bound is at least its parent's.  The child is a
        part of the parent, so the parent's bound holds for it; the 20 warm-started steps can end below it (the split node's new
        multiplier starts at 0), and without this the lowest open bound falls when such a parent is replaced by its children.  Device
        work only."""
        parent = self.pool.bound[slots[:n].long().clamp(min=0)].repeat_interleave(C)
        torch.maximum(Ch.bound[:C * n], parent, out=Ch.bound[:C * n])

    def _ub_points(self, Ch):
        """The points the rows' ubv are the network's values at."""
        return Ch.x_lp if self.pgd_steps is None else Ch.x_ub

    def _pair_b_source(self, M):
        """The witness step's view of pair B: nothing without a selected parent (no choice was launched, used_kw is a past round's)."""
        if self.threshold is None or M == 0:
            return {}
        return {"x_b": self._ub_points(self.ChB), "used_kw": self.used_kw, "sel_rows": self.sel_rows}

    def _scorer_inputs(self, B):
        """gnnb_dual_ascent at n_iter = 0 over the first B parent rows: the scorer's inputs at the stored best point (one evaluation of g
        instead of ~120 KB of fp32 inputs per open domain)."""
        P, lib, h = self.P, self.lib, self.eng.h
        with torch.cuda.device(self.eng.device):
            _lib.check(lib.gnnb_dual_ascent(h, C.byref(P.dual_batch), B, 0, self.lr, P.alpha.data_ptr(), P.beta.data_ptr(), 1, P.bound.data_ptr(), None, None,
                                            P.t_dual, P.t_prims, P.x_lp.data_ptr(), P.lb32[-1].data_ptr(), self.ws_dual.data_ptr(), self.ws_dual.numel(),
                                            self._stream()), "gnnb_dual_ascent")

    def _score_parents(self, B):
        """``_scorer_inputs`` and gnnb_forward over the first B parent rows."""
        P, lib, h = self.P, self.lib, self.eng.h
        self._scorer_inputs(B)
        with torch.cuda.device(self.eng.device):
            _lib.check(lib.gnnb_forward(h, C.byref(P.fwd_batch), B, P.scores.data_ptr(), P.dec.data_ptr(), self.status.data_ptr(), self.ws_fwd.data_ptr(),
                                        self.ws_fwd.numel(), self._stream()), "gnnb_forward")
        self.status_all |= self.status

    def _babsr_parents(self, n):
        """``branching="babsr"`` in ``_score_parents``' place: gnnb_babsr on the n parent rows the gather wrote and
        the BaBSR decision of every row (``_decide``) into ``P.dec``.  No gnnb_dual_ascent at n_iter = 0, no gnnb_forward."""
        P = self.P
        self.eng.babsr_rows(P.lb32, P.ub32, P.box[2], P.amb, n, self.kw_scores, self.kw_icp)
        self._decide(n)

    def _launch(self, slots, n):
        """The launches of a round over the n parents in ``slots`` (their boxes: the parent rows' own), from the gather to the commit."""
        P, Ch, eng, pool = self.P, self.Ch, self.eng, self.pool
        eng.frontier_gather(pool, slots, P.box[0], P.box[1], P.mask, P.lb, P.ub, P.lb32, P.ub32, P.alpha, P.beta, P.amb)
        if self.depth:
            return self._launch_depth(slots, n, self.depth)
        if self.branching == "gnn":
            self._score_parents(n)
        else:
            if self.branching == "strong":
                self._strong_parents(n)
            else:
                self._babsr_parents(n)
            if self.keep_pairs:                                   # (a traced run: "parent_bounds", which gnnb_dual_ascent at n_iter 0 would have left)
                P.bound[:n] = pool.bound[slots[:n].long().clamp(min=0)]
        if (self.strong_audit is not None or self.learning) and self.branching != "strong":      # the same table next to the round's own decisions (P.dec untouched)
            self._strong_table(slots, n, self.s_dec, self.im_table if self.learning else None)
        if self.strong_on and (self.keep_pairs or self.strong_audit is not None):      # (a traced or audited run: the bounds the commit overwrites)
            self.parent_bound = pool.bound[slots[:n].long().clamp(min=0)]
        eng.frontier_expand(pool, slots, P.dec, Ch.mask, Ch.plb, Ch.pub, Ch.split, Ch.alpha, Ch.beta, Ch.live)
        self._bound_children(Ch, 2 * n, warm=True)
        self._at_least_the_parent_s(Ch, slots, n)
        if self.threshold is not None:
            self._fall_back(n)
        if self.witness_on:
            self._witness(n, self.M)
        self._commit(slots)
        if self.learning and self.replay is not None:             # section 7.16: the round's labelled rows go into the buffer, device work only
            self.buffer.push(P.fwd_batch, n, self.im_rows[:n], n, self.im_table, status=self.push_status)
            self.status_all |= self.push_status

    def _launch_depth(self, slots, n, d):
        """A round of a ``split_depth`` run behind its gather: every one of the n parents is split on its d
        best-scored undecided nodes -- ``gnnb_strong_list`` on the scores ``gnnb_forward`` just wrote, whose first-ranked node is the
        forward's own decision -- into C = 2^d child rows, which are bounded, held to the parent's bound and committed as any round's
        are.  The witness is a minimum over the C n rows (``gnnb_frontier_witness`` with C n / 2 row pairs and no pair B)."""
        P, Ch, eng, pool, C = self.P, self.Ch, self.eng, self.pool, 1 << d
        self._score_parents(n)
        eng.strong_list(pool, slots, P.amb, P.scores, d, self.cand0, self.cand_row, self.cand_slot, self.cand_dec, workspace=self.ws_strong)
        eng.frontier_expand_depth(pool, slots, d, self.cand0, self.cand_dec, Ch.mask, Ch.plb, Ch.pub, Ch.split, Ch.alpha, Ch.beta, Ch.live)
        self._bound_children(Ch, C * n, warm=True)
        self._at_least_the_parent_s(Ch, slots, n, C)
        if self.witness_on:
            self._witness(C * n // 2, 0)
        self.eng.frontier_commit_depth(pool, slots, d, *Ch.children(), pool.state, eps=self.eps, decision_bound=self.decision_bound,
                                       workspace=self.ws_commit)

    def _fall_back(self, n):
        """The threshold mode between the bounding of pair A and the commit (DESIGN.md sections 7.5 and 7.6): BaBSR on the n parent rows,
        the improvement test and the selection (``_select``), the read of the number M of selected parents (``_read_selected``), and for
        M > 0 ONE pair B chain for all of them and the choice with what the run keeps of its outcome (``_choose``)."""
        P, Ch, ChB, eng, pool = self.P, self.Ch, self.ChB, self.eng, self.pool
        eng.babsr_rows(P.lb32, P.ub32, P.box[2], P.amb, n, self.kw_scores, self.kw_icp)
        self._select(n)
        if self.keep_pairs:                                       # (a traced run: pair A as it was bounded, before the choice overwrites rows)
            self.pair_a = (Ch.bound[:2 * n].clone(), Ch.infeasible[:2 * n].clone())
        M = self._read_selected()
        if M == 0:
            return
        eng.frontier_expand(pool, self.sel_slots[:M], self.sel_dec, ChB.mask, ChB.plb, ChB.pub, ChB.split, ChB.alpha, ChB.beta, ChB.live)
        self._bound_children(ChB, 2 * M, warm=True)
        self._at_least_the_parent_s(ChB, self.sel_slots, M)
        self._choose(n, M)

    def check_status(self):
        self._settle_step()
        self._raise_for(int(self.status_all.cpu()[0]))

    def _raise_for(self, st):
        if st & 8 and (self.imitate is not None or self.online is not None):      # (bit 3 is a learning step's: the imitation step's, or the online step's)
            raise RuntimeError(_Round._refusal(self))
        from .engine import _raise_for_status
        _raise_for_status(st)

    def _online_buffers(self, n_parents, tables, counts):
        """The online mode's state for rounds of up to n_parents parent rows (DESIGN.md sections 7.7 and 7.19).  tables: the shape of
        ``wrong``, the wrong-point table(s) -- (R,) for one job, (segments, R) for a pool; counts: the length of ``learn_count``, the count
        array a round with M > 0 reads behind the state record (1: n_learn; segments + 1: learn_entry).  The dense lists of a round's learn
        rows, what the step reports per learn row, and the step's status word."""
        dev, n, i32, f32 = self.eng.device, n_parents, torch.int32, torch.float32
        self.wrong = torch.zeros(tables, dtype=i32, device=dev)
        self.learn_rows, self.learn_kw, self.learn_count = (torch.zeros(c, dtype=i32, device=dev) for c in (n, n, counts))
        self.learn_imp, self.loss = torch.zeros(n, dtype=f32, device=dev), torch.zeros(n, dtype=f32, device=dev)
        self.step_status = torch.zeros(1, dtype=i32, device=dev)

    def _learn(self):
        """The learning half of an online round with M > 0 (DESIGN.md sections 7.7 and 7.19), behind the commit and the read of the state
        record: the read of the count array (``read_learn``: 4 bytes of n_learn in a one-job run, 4 (entries + 1) bytes of learn_entry in a
        pool) and, with N > 0 learn rows, ONE step over them on the parent rows' scorer inputs, which the round's gather and
        gnnb_dual_ascent(n_iter 0) left in ``P`` (intact until the next gather).  ``k``: the parent rows of the round (of all its entries,
        in a many-jobs run), which the learn rows are rows of.  The next round's forward scores with the new parameters."""
        self.learn_pending = False
        n = self.last_learn = self.read_learn()
        if n == 0:
            return
        self.step_status.zero_()
        self.eng.online_step_rows(self.P.fwd_batch, self.k, self.learn_rows[:n], self.learn_kw[:n], self.learn_imp[:n], loss=self.loss[:n],
                                  status=self.step_status)
        self.status_all |= self.step_status
        self.online_steps, self.online_rows = self.online_steps + 1, self.online_rows + n
        self._step_issued(("learn_rows", "learn_kw", "learn_imp"))

    def _imitate(self):
        """The learning half of a learning round, behind the commit and the read of the state record.  When the
        round listed a candidate -- ``strong_n``, the 4 bytes the round already read -- ONE step over ALL k parent rows on the scorer inputs
        the round left in ``P`` (intact until the next gather), every row scored with the round's opening parameters; a row without a
        candidate contributes nothing.  If every candidate's improvement is NaN (a dead child each) the gradient is zero and the step is
        weight decay alone.  The next round's forward scores with the new parameters.  ``k``: the number of parent rows of the round (of
        all its entries, in a many-jobs run)."""
        self.imitate_pending, self.last_imitation = False, 0
        if self.replay is not None:
            return self._replay_steps()
        if self.strong_n <= 0:
            return
        k = self.last_imitation = self.k
        self.step_status.zero_()
        self.eng.imitation_step_rows(self.P.fwd_batch, k, self.im_rows[:k], self.im_table, self.imitate_margin, loss=self.im_loss[:k],
                                     report=self.im_report[:k], regret=self.im_regret[:k], status=self.step_status)
        self.status_all |= self.step_status
        self.imitation_steps, self.imitation_rows = self.imitation_steps + 1, self.imitation_rows + k
        self._step_issued()


    def _replay_steps(self):
        """``_imitate`` of a run with ``imitate=Replay(...)``.  The round's push is already on the stream
        (``_launch``).  When the round listed a candidate the host reads the buffer's state word -- 16 bytes right behind the state
        record -- and with ``filled`` >= 1 issues ``steps`` steps, each on min(batch, filled) entries drawn afresh with the run's draw
        counter.  In repack mode "device" the steps are issued back to back without a host wait; status, losses and reports are read
        with the next round's record (``_step_issued``)."""
        rp, buf = self.replay, self.buffer
        if self.strong_n <= 0:                                    # (no candidate anywhere: the push stored nothing)
            self.replay_skipped += self.k
            return
        _, filled, stored, skipped = buf.read_state()
        self.replay_stored, self.replay_skipped, self.replay_filled = self.replay_stored + stored, self.replay_skipped + skipped, filled
        self.last_replay = {"stored": stored, "skipped": skipped, "filled": filled, "steps": 0, "batch": 0}
        if rp.steps == 0 or filled < 1:
            return
        b = self.last_imitation = min(rp.batch, filled)
        self.step_status.zero_()
        for s in range(rp.steps):
            buf.step(b, self.imitate_margin, rp.seed, self.draw, loss=self.rp_loss[s, :b], report=self.rp_report[s, :b], regret=self.rp_regret[s, :b],
                     status=self.step_status, out=self.rp_idx[s, :b])
            self.draw += 1
        self.status_all |= self.step_status
        self.last_replay.update(steps=rp.steps, batch=b)
        self.imitation_steps, self.imitation_rows = self.imitation_steps + rp.steps, self.imitation_rows + rp.steps * b
        self._step_issued()


class FrontierRun(_Round):
    """The device side of ``branch_and_bound_frontier``: ``root()`` once, then per round ``launch_round(k)`` (device work only, nothing
    synchronises) and ``read_state()`` (the round's one device-to-host copy).

    With a ``branching_threshold`` the run also owns a second set of child rows, the table ``ineff`` of
    inefficient KW points and the intercept counter ``icp``, and a round reads one more number, the count of selected parents
    (``read_selected``, 4 bytes), between its two halves.

    With an ``online_threshold`` it also owns the table ``wrong`` of wrong GNN points, the dense lists of a round's
    learn rows and their number ``n_learn``; a round with m > 0 reads ``n_learn`` (4 bytes) behind the state record and, when it is not
    zero, takes one learning step over those rows (``gnnb_online_step_rows``, which synchronises).

    With ``imitate`` = N every round whose 1-based number is a multiple of N is a learning round: its table stays
    in ``im_table`` ((K, R) fp64) and, behind the state record, when the round listed a candidate, ONE ``gnnb_imitation_step_rows`` (which
    synchronises) runs over all its parent rows."""

    def __init__(self, lp, choice, layers, K=16, n_iter=20, lr=0.1, eps=1e-4, decision_bound=None, capacity=None, branching_threshold=None,
                 kwbd_threshold=KWBD_DEFAULT, sparsest_layer=0, decision_threshold=0.001, online_threshold=None, max_rounds=0, witness=None,
                 pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None, pgd_seed=0, repack="host", imitate=None,
                 imitate_margin=IMITATE_MARGIN_DEFAULT, strong_candidates=None, strong_chunk=STRONG_CHUNK_DEFAULT, strong_audit=None, branching="gnn"):
        self.capacity = _check_args(K, n_iter, lr, eps, max_rounds, capacity)       # (max_rounds: the loop's, checked here with the rest)
        self._set_options(choice, branching=branching, branching_threshold=branching_threshold, kwbd_threshold=kwbd_threshold, sparsest_layer=sparsest_layer,
                          decision_threshold=decision_threshold, online_threshold=online_threshold, witness=witness, pgd_steps=pgd_steps, pgd_step=pgd_step,
                          pgd_restarts=pgd_restarts, pgd_seed=pgd_seed, imitate=imitate, imitate_margin=imitate_margin,
                          strong_candidates=strong_candidates, strong_chunk=strong_chunk, strong_audit=strong_audit, repack=repack)
        split_depth = getattr(lp, "split_depth", None)            # (section 7.20: the option travels on the root's description, as tighten_root does)
        _check_split_depth(split_depth, branching, branching_threshold, online_threshold, imitate, strong_audit, strong_candidates)
        if split_depth is not None:                               # (set only where given, as strong_G)
            self.split_depth = split_depth
        layers = list(layers)
        if type(layers[-1]) is not nn.Linear or layers[-1].out_features != 1:
            raise ValueError("the last layer must be the folded property layer Linear(., 1)")
        tighten_root = getattr(lp, "tighten_root", 0)             # (section 7.18: the option travels on the root's description)
        _check_tighten(tighten_root)
        self.K, self.n_iter, self.lr, self.eps, self.decision_bound = K, n_iter, float(lr), float(eps), decision_bound
        self.fixed, self.prop_layer = layers[:-1], layers[-1]
        eng = self.eng = self._engine_of(choice)
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
        self._buffers(K, n, in_shape, (self.x_lo, self.x_hi, self.pw, self.pb))
        self.root_rows = 1
        self.set_tighten_root(tighten_root)
        self._witness_buffers(1)
        self.slots = None
        self.m, self.m_e, self.M = 0, [0], 0                      # (m_e, M: the round as a plan of one entry)
        if self.threshold is not None:
            self._threshold_buffers(K, ((1,), (eng.R,)), None, "gnnb_frontier_fallback_workspace_bytes")
            self.m_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        if branching == "babsr":                                  # one intercept counter per run, zero at its start (relu_conv_any_kw.py:100)
            self._babsr_buffers(K, (1,))
        if self.strong_on:                                        # the candidates' rows: the run's one box and property, 2 * strong_chunk times
            self._strong_buffers(K, tuple(t[:1].expand(2 * strong_chunk, *t.shape[1:]).contiguous() for t in (self.x_lo, self.x_hi, self.pw, self.pb)))
        if self.online is not None:                               # one table for the run's one job, one count: n_learn
            self._online_buffers(K, (eng.R,), 1)
            self.n_learn = self.learn_count
        self._imitation_buffers(K)
        self._depth_buffers(K)
        self._use_repack()                                        # last: nothing behind it can fail and leave the engine in the run's mode

    def _commit(self, slots):
        self.eng.frontier_commit(self.pool, slots, *self.Ch.children(), self.pool.state, eps=self.eps, decision_bound=self.decision_bound,
                                 workspace=self.ws_commit)

    def root(self):
        """Bound the domain with every ReLU undecided (no parent, the default start of the ascent) and commit it as the first open domain:
        child row 0 of a commit with K = 1, slot 0, live = [1, 0]."""
        Ch = self.Ch
        Ch.mask[:1].fill_(-1)
        Ch.split[:2].fill_(-1)
        Ch.live[:2] = torch.tensor([1, 0], dtype=torch.int32).to(Ch.live.device)
        self._bound_children(Ch, 1, warm=False, tighten=self.tighten_root)
        if self.witness_on:
            self._witness(1, 0)
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

    def launch_round(self, k, in_use, depth=0):
        """One round over the k <= K open domains of lowest bound.  Device work only.  depth: 0, or in a ``split_depth`` run the round's d
        (``round_depth``): 2^d children per parent."""
        self.slots = self.pick(k, in_use)
        self.depth = depth
        self._begin_round(k)
        self._launch(self.slots, k)

    # ``_Round._fall_back``'s steps for one job: gnnb_frontier_fallback, the read of m, gnnb_frontier_choose
    def _select(self, k):
        Ch = self.Ch
        self.eng.frontier_fallback(self.pool, self.slots, Ch.live, Ch.infeasible, Ch.bound, self.kw_scores, self.kw_icp, self.P.amb, self.icp, self.ineff,
                                   self.gnn_imp, self.kw_dec, self.sel_rows, self.sel_slots, self.sel_dec, self.m_dev, self.threshold, self.kwbd_threshold,
                                   self.sparsest_layer, self.decision_threshold, self.random_order, workspace=self.ws_fallback)

    def _decide(self, k):
        self.eng.frontier_babsr_decide(self.kw_scores, self.kw_icp, self.P.amb, self.icp, self.P.dec, k, self.sparsest_layer, self.decision_threshold,
                                       self.random_order, workspace=self.ws_babsr)

    def _read_selected(self):
        m = self.m = self.M = self.read_selected()
        self.m_e = [m]
        return m

    def _choose(self, k, m):
        self.eng.frontier_choose(self.pool, k, m, self.sel_rows, self.sel_slots, self.sel_dec, self.P.dec, self.gnn_imp, self.Ch, self.ChB, self.ineff,
                                 self.kw_imp, self.used_kw, self.dec)
        self.n_used += self.used_kw[:k].sum()
        if self.online is not None:                               # the learn rows of the round (section 7.7): read behind the state record
            self.eng.frontier_learn(k, self.P.dec, self.kw_dec, self.used_kw, self.gnn_imp, self.kw_imp, self.online, self.wrong, self.learn_rows,
                                    self.learn_kw, self.learn_imp, self.n_learn)
            self.learn_pending = True                             # (k: the round's, ``_begin_round`` kept it)

    def _witness(self, k, M):
        """gnnb_frontier_witness on the rows the commit will see."""
        self.eng.frontier_witness(k, self.Ch, self._ub_points(self.Ch), self.best_value, self.best_point, m=M, **self._pair_b_source(M))

    def witness(self):
        """The incumbent's point as a CPU fp32 tensor of the input shape (None while global_ub is +inf): N_0 floats, read once per run."""
        if not self.witness_on or math.isinf(float(self.best_value.cpu()[0])):
            return None
        return self.best_point[0].cpu().reshape(self.in_shape)

    def read_learn(self):
        """n_learn, the number of learn rows: the 4 bytes an online round with m > 0 reads behind the state record."""
        return int(self.n_learn.cpu()[0])

    def read_selected(self):
        """m, the number of parents whose KW decision gets bounded: the 4 bytes a threshold round reads between its halves."""
        return int(self.m_dev.cpu()[0])

    def read_state(self):
        """The state record as a list of Python floats: the one device-to-host copy of a round (of its second half, in threshold mode).
        An online round with m > 0 then reads n_learn and takes its learning step (``_learn``); a learning round of ``imitate`` takes its
        step (``_imitate``)."""
        st = self.pool.state.cpu().tolist()
        self._settle_step()                                       # ("device" mode: the previous round's step, read behind this record)
        if self.learn_pending:
            self._learn()
        self._step_behind_read()
        return st


def branch_and_bound_frontier(lp, choice, layers, K=16, n_iter=20, lr=0.1, eps=1e-4, max_rounds=50, decision_bound=None, capacity=None, log=print,
                              trace=None, branching_threshold=None, kwbd_threshold=KWBD_DEFAULT, sparsest_layer=0, decision_threshold=0.001, stats=None,
                              online_threshold=None, witness=None, pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None, pgd_seed=0,
                              repack="host", imitate=None, imitate_margin=IMITATE_MARGIN_DEFAULT, strong_candidates=None,
                              strong_chunk=STRONG_CHUNK_DEFAULT, strong_audit=None, branching="gnn"):
    """Branch and bound with the open domains in device memory, K of them expanded per round.

    lp: a ``LayerGraphLP`` (its input box is the root); choice: a ``GraphChoice`` (the GNN; its engine runs every step);
    layers: the network's layers with the folded property layer last.  Per round the up-to-K open domains of lowest bound (equal bounds:
    lowest slot) are split at the GNN's decision, their 2K children bounded by ``gnnb_kw_bounds`` and ``n_iter`` warm-started steps of
    ``gnnb_dual_ascent`` (a child whose steps end below its parent's bound takes the parent's: it holds for every part of the parent, and
    global_lb then never falls from round to round), and kept or closed by ``branch_and_bound``'s rule against the global upper bound after the round's minimum.
    The loop stops under ``branch_and_bound``'s conditions: no open domain ("exhausted"), global_ub - global_lb <= eps ("gap"), the
    sign of (minimum - decision_bound) known ("decision"), or after ``max_rounds`` ("max_rounds").  capacity: slots of the pool (None:
    max(1024, 4K + 1)).  A round of k parents needs k slots above the slots in use (its 2k children reuse the parents' slots first): when
    they are not there the pool is compacted, and when the open domains themselves leave no room for k more the loop stops ("capacity") -- global_lb stays sound either way: it is the minimum over the open bounds, closed_lb
    and global_ub.  trace: None, or a list that receives per round a dict of the picked slots, their bounds, the decisions, the
    children's bounds / upper values / live and infeasible flags (extra device-to-host copies: off in a timed run).

    branching_threshold (None: off, and nothing below applies): the control flow of ``lp_producer.branch_and_bound_threshold`` (reference
    plnn/relu_conv_gnnkwthreshold.py:151-195) inside a round, DESIGN.md section 7.5.  A parent whose GNN split improves the bound by less
    than ``branching_threshold`` (0 < . <= 1) asks the BaBSR heuristic (``sparsest_layer``, ``decision_threshold``: ``kw_score_conv.decide``'s);
    unless that point was inefficient ``kwbd_threshold`` times its two children are bounded too, and the better pair is committed.  The
    intercept counter and the inefficiency counts are read and updated in parent row order within a round.  A parent whose BaBSR scores
    hold a NaN, or that has no undecided node, keeps its GNN pair (the host rule would raise).  The trace's "decisions" are then the
    final ones and it also carries "gnn_decisions", "gnn_improvement", "kw_decisions" ([-1, -1]: not asked), "kw_improvement" (-1: not
    bounded), "selected" (rows), "used_kw" and both pairs' bounds as they were bounded ("gnn_child_bounds" / "gnn_child_infeasible",
    "kw_child_bounds" / "kw_child_infeasible", two per selected row).  stats: None, or a dict that receives "branches" (parents
    expanded), "kw_bounded", "kw_used" and "domains_bounded"; domains_bounded counts the children of both pairs.

    online_threshold (None: off, and nothing below applies; needs a ``branching_threshold`` and the default ``kwbd_threshold``): the control
    flow of ``lp_producer.branch_and_bound_online`` (reference plnn/relu_conv_online.py:126-276) inside a round, DESIGN.md section 7.7.
    ``choice`` must be a ``graphnet.graph_score_online.GraphChoice``.  Every parent with a KW decision gets its second pair bounded (the
    online loop has no table of inefficient points); a parent that took its KW pair counts its GNN decision as a wrong point, and once a
    node has been wrong ``online_threshold`` times the parent is a learn row: behind the commit the round takes ONE Adam step on the summed
    loss (max score - score of the KW node + improve) of its learn rows, all scored with the round's opening parameters, and the next
    round's forward uses the new ones.  With K = 1 that is the reference's step per parent.  When the run ends (or raises) after a step,
    ``choice.model`` receives the device's parameters.  stats then also holds "online_steps" and "online_rows", and a round's trace
    "learn_rows", "learn_kw" (flat ReLU indices), "learn_improve" and "loss" (per learn row), and the bounds after the round, "global_lb"
    and "global_ub".

    witness, pgd_steps, pgd_step (with ``witness`` and ``pgd_steps`` at None no launch, read or argument of a round
    changes).  witness: None, or a list that receives, when the run ends, the point global_ub is the network's value at -- one CPU fp32
    tensor of the input shape, or None while global_ub is +inf -- as every loop of the reference returns global_ub_point
    (plnn/branch_and_bound.py:157): per round one more launch keeps the point on the device, and N_0 floats cross the link once.
    pgd_steps: None, or an integer >= 0: every child's upper value is the best of up to ``pgd_steps`` projected signed-gradient steps on
    the network from its LP point (``gnnb_net_descend``; reference plnn/conv_kwinter_gen.py:54-135 without its restarts), each moving a
    coordinate by ``pgd_step`` (0 < . <= 1) times its box width; 0 computes what None computes.  A traced round of a run with a witness
    also carries "global_ub" and "witness_value", the device's copy of it.

    pgd_restarts, pgd_seed (with ``pgd_restarts`` at None or 0 no launch, read or argument of a round changes).
    pgd_restarts: None, or an integer R >= 0 (it needs ``pgd_steps``): every child descends from its LP point and from R uniform points of
    its box (``gnnb_net_starts``, ``gnnb_net_descend_starts``), and its upper value is the least of their best values.  With
    ``pgd_steps=0`` that is the reference's get_upper_bound_random (plnn/conv_kwinter_gen.py:20-52) with the LP point added; with
    ``pgd_steps=N`` the restarts of get_upper_bound_pgd (:54-135) under ``pgd_steps``' per-row rule.  pgd_seed: an integer in 0..2^64 - 1,
    the seed of every launch: a row's points depend on its own LP point, box and the seed only, so a run repeats itself and a job in a pool
    gets what it gets alone.

    branching (with "gnn", the default, no launch, read or argument of a round changes).  "babsr": the reference's
    relu_bab (plnn/relu_conv_any_kw.py:45-181 with split_decision='kw'): every parent is split at the BaBSR heuristic's decision
    (``gnnb_babsr`` on the parent rows, then ``gnnb_frontier_babsr_decide``: ``kw_score_conv.decide`` with ``sparsest_layer`` and
    ``decision_threshold``, the layer order ``lp_producer._random_order``), one intercept counter starting at 0 and carried through the
    rows of a round and from round to round.  The round runs no ``gnnb_dual_ascent`` at n_iter 0 on the parents and no ``gnnb_forward``:
    ``choice`` supplies the engine, its GNN is never run.  Bounding, the witness, PGD, the restarts and the commit are unchanged.  A parent
    whose scores hold a NaN, or that has no undecided node, gets no decision and is closed at its own bound (the host rule would raise).  It
    takes no ``branching_threshold`` and no ``online_threshold``.  A traced round's "decisions" are BaBSR's.

    branching="strong", strong_candidates, strong_chunk, strong_audit (with ``branching`` "gnn" or "babsr" and
    ``strong_audit`` at None no launch, read, buffer or argument of a round changes).  "strong": strong branching, the strategy the GNN was
    trained to imitate: for every parent both children of every CANDIDATE split are bounded exactly as a round bounds children
    (``gnnb_kw_bounds``, ``n_iter`` warm-started steps of ``gnnb_dual_ascent``) and the parent is split at the candidate whose
    ``bab_caller.gnn_improvement`` is largest (equal values: the lowest flat ReLU index).  strong_candidates: None, every undecided node,
    or an integer M >= 1, the M undecided nodes of highest BaBSR score (``gnnb_babsr``; equal scores: the lowest index).  The candidates of
    all parents form one dense list (``gnnb_strong_list``) that is bounded in chunks of ``strong_chunk`` candidates (2 * strong_chunk child
    rows per launch chain; a chunk may span parents), then ``gnnb_strong_pick`` writes the decisions; the round's one extra read is the
    number of candidates (``FrontierRun.read_candidates``, 4 bytes).  The winners' children are then bounded again as any round's are,
    which gives them their LP points and upper values: by the batch kernels' row independence their bounds are the candidates' bit for
    bit.  ``choice`` supplies the engine, its GNN is never run.  A parent without a candidate (no undecided node, a NaN BaBSR score at an
    undecided node) or whose every candidate has a dead child gets no decision and is closed at its own bound.  It takes no
    ``branching_threshold`` and no ``online_threshold``.  A traced round also carries "strong_candidates" (flat indices) and
    "strong_improvement", one list per parent; stats gains "strong_bounded", the candidate children bounded -- ``domains_bounded`` keeps
    its meaning, the rounds' 2k children.  strong_audit: None, or a list; legal with every ``branching``, not with a threshold or online
    learning.  Every round then also computes the table of its parents (in "strong" mode the one already there; otherwise the steps
    above into buffers of their own, the round's decisions untouched) and appends one dict per parent: "slot", "decision" (the one
    committed), "improvement" (of that decision, from the round's own children through ``bab_caller.gnn_improvement``; NaN for a dead
    pair), "strong_decision", "best_improvement", "candidates" (flat indices) and "improvements" -- extra device-to-host copies, like
    ``trace``'s: off in a timed run.

    imitate, imitate_margin (with ``imitate`` at None no launch, read, buffer or argument of a round changes).
    imitate: None, an integer N >= 1, or a ``Replay`` (``Replay(every=N, buffer=None, capacity=1024, batch=8, steps=1,
    seed=0)`` -- a learning round pushes its parent rows and their table into a device-resident ``ReplayBuffer``, reads the buffer's 16-byte
    state word behind the state record and takes ``steps`` steps on min(batch, filled) freshly drawn entries; ``steps=0`` only collects, with
    any choice and no optimizer; stats gain "replay_stored", "replay_skipped" and "replay_filled", a traced learning round "replay_idx",
    "replay_loss", "replay_report" and "replay_regret" per step).  With an integer: every round whose 1-based number is a multiple of N is a LEARNING round.  Legal with ``branching``
    "gnn" and "strong" and together with ``strong_audit``, ``strong_candidates`` and ``strong_chunk``, which shape the table as they shape
    a strong round's; not with "babsr", a ``branching_threshold`` or an ``online_threshold``.  ``choice`` must be a
    ``graphnet.graph_score_online.GraphChoice`` (it owns lr and wd).  A learning round leaves its table -- per parent the improvement of
    every candidate, NaN elsewhere -- in device memory: in "strong" mode the round's own, in "gnn" mode the audit's steps next to the
    round's decisions (other rounds do not compute it unless an audit asks); in "strong" mode it also runs ``gnnb_dual_ascent`` at n_iter 0
    on the parents, so that the scorer inputs exist, and still no ``gnnb_forward``.  Commit first, then learn: behind the read of the state
    record, when the round listed a candidate, ONE ``gnnb_imitation_step_rows`` takes an Adam step on the summed loss of all k parent rows
    -- a margin-rescaled ranking hinge that asks the GNN to score the table's best candidate above every other by ``imitate_margin`` times
    the difference of their improvements (include/gnnb.h states it) -- all scored with the round's opening parameters; the next round's
    forward uses the new ones.  A row without a candidate contributes nothing; if every candidate of the round has a NaN improvement (a
    dead child each) the gradient is zero and the step is weight decay alone.  When the run ends (or raises) after a step ``choice.model``
    receives the device's parameters.  stats then also holds "imitation_steps" and "imitation_rows" (the parent rows handed to the steps),
    and a traced learning round "imitation_loss", "imitation_regret" (the table's best improvement minus that of the GNN's best candidate)
    and "imitation_report" ([teacher, pick, candidates, violators] as flat ReLU indices and counts), one per parent row; every traced round
    of such a run carries the bounds after it, "global_lb" and "global_ub".

    strong_candidates=Shortlist(babsr=M, gnn=G) (with an integer or None no launch, read, buffer or argument of a
    round changes, and ``Shortlist(babsr=M)`` is the run ``strong_candidates=M``).  gnn=G: the candidates of a parent are its G undecided
    nodes of highest GNN score -- ``gnnb_forward``'s scores of the parent rows, through the same ``gnnb_strong_list`` --, with both counts
    the union of the two shortlists (``gnnb_strong_list_union``; at most M + G per parent).  In a "gnn" run the committed decision, the
    scorer's arg-max, is then always a candidate: its table row has an entry there, and a learning round's report ``pick`` is the decision
    that was made.  In a "strong" run the round runs ``gnnb_dual_ascent`` at n_iter 0 and ``gnnb_forward`` on the parents in front of the
    list ("the GNN proposes, the bounds dispose"); a learning round does not run that ascent a second time.  A gnn count needs a choice
    whose model is a GraphNet and is refused with "babsr".  No read is added.  Audit dicts of such a run also hold "sources" (per candidate
    1: BaBSR's shortlist only, 2: the GNN's only, 3: both) and a traced strong round "strong_sources".

    repack (it matters to a run that learns, with ``online_threshold`` or ``imitate``): "host" (default) rebuilds
    the scorer's operand packs on the host after every learning step, which waits for the stream.  "device" builds them on the stream:
    the step is only issued, and a learning round adds no host wait of its own.  Its status word, and the loss, report and regret a traced
    round shows, are then read with the NEXT round's state record, or at the end of the run for the last round; the RuntimeError for
    status bit 3 is raised at that read and names the round that learnt.  Decisions, bounds, losses and parameters are those of "host"
    wherever the two builders' packs give the same scores (a folded pack entry may differ by one fp32 unit in the last place).

    lp.tighten_root (``LayerGraphLP(..., tighten_root=n)`` -- this parameter list is fixed, so the option travels on
    the root's description; with 0, the default, no launch, read, buffer or argument of the run changes).  An integer n >= 1: the root's
    intermediate bounds come from ``gnnb_kw_tighten`` at n iterations (step ``lr``) -- every ambiguous node of graph layers 2..L
    bounded by its own slope-optimised dual ascent -- in place of ``gnnb_kw_bounds``.  Every child copies or intersects its parent's bounds,
    so the whole tree inherits them; no round runs the tightening, and it adds no read.

    lp.split_depth (``LayerGraphLP(..., split_depth=D)`` -- this parameter list is fixed, so the option travels on
    the root's description, as ``tighten_root`` does; with None, the default, no launch, read, buffer or argument of a round changes).  An
    integer D in 1..8 (a bool is refused): the most ReLUs a parent is split on in one round.  A round of k parents runs at the depth d = ``round_depth(k, K, D, open,
    capacity)``, the largest d <= D whose k 2^d children fit the round's 2K child rows and the pool; a full round (k = K) is depth 1.  Parent
    i is split on the first d undecided nodes in the order (score descending, flat index ascending) of ``gnnb_forward``'s scores
    (``gnnb_strong_list``; the first of them is the forward's own decision; a parent with m < d undecided nodes on its m) and gets the 2^d
    children of every assignment of those nodes (``gnnb_frontier_expand_depth``), all bounded, held to the parent's bound and kept or closed
    by the round's one rule (``gnnb_frontier_commit_depth``); the children of a deep split are not re-scored in between.  The pool is
    compacted when the slots in use leave no room for the (2^d - 1) k children beyond the parents' slots, and the run stops ("capacity")
    when not even d = 1 fits.  No read is added.  A traced round also carries "depth" and "nodes" (per parent the [layer, idx] pairs of its
    split, in ascending flat index) and its children's lists hold 2^d entries per parent; "decisions" stay ``gnnb_forward``'s.  Only with
    ``branching="gnn"``; it takes no ``branching_threshold``, ``online_threshold``, ``imitate``, ``strong_audit`` or ``Shortlist``, with or
    without ``witness``, ``pgd_steps``, ``pgd_restarts``, ``decision_bound`` and ``lp.tighten_root``.

    Returns (global_lb, global_ub, rounds, domains_bounded, reason)."""
    run = FrontierRun(lp, choice, layers, K, n_iter, lr, eps, decision_bound, capacity, branching_threshold, kwbd_threshold, sparsest_layer,
                      decision_threshold, online_threshold, max_rounds, witness, pgd_steps, pgd_step, pgd_restarts, pgd_seed, repack, imitate,
                      imitate_margin, strong_candidates, strong_chunk, strong_audit, branching)      # (checks every argument before it touches a device)
    run.keep_pairs = trace is not None
    try:
        out = _one_job_loop(run, max_rounds, log, trace, stats)
        if witness is not None:
            witness.append(run.witness())
        return out
    finally:
        if run.online_steps or run.imitation_steps:               # the nn.Module mirrors the device, as GraphChoice.online_learning leaves it
            choice.model.load_blob(run.eng.get_weights())
        run.close()


def _one_job_loop(run, max_rounds, log, trace, stats):
    """``branch_and_bound_frontier``'s loop on a checked ``FrontierRun``: every round is a plan of the one entry (segment 0, row 0, k)."""
    S = _lib
    st = run.root()
    tally = _new_tally()
    log(f"root lb {_global_lb(st):.5f} ub {st[S.FS_GLOBAL_UB]:.5f}")
    while True:
        global_lb, global_ub, n_open, in_use = _global_lb(st), st[S.FS_GLOBAL_UB], int(st[S.FS_N_OPEN]), int(st[S.FS_IN_USE])
        if run.split_depth is None:
            (reason, k, compact), d = _one_job_round(st, run.K, run.capacity, run.eps, run.decision_bound, tally["rounds"], max_rounds), 0
        else:                                                     # section 7.20: the round's depth and its capacity arithmetic
            reason, k, compact, d = _one_job_round_depth(st, run.K, run.split_depth, run.capacity, run.eps, run.decision_bound, tally["rounds"], max_rounds)
        if reason is not None:
            break
        if compact:                                               # the kept children beyond the k parents' slots go above in_use
            run.pool.compact(n_open)
            in_use = n_open
        run.launch_round(k, in_use, d) if d else run.launch_round(k, in_use)
        t = _report_launched(run, trace, 0, 0, k, {})
        st = run.read_state()
        if t is not None:
            if run.online is not None:
                t.update(_online_trace(run, st, t))
            _report_read(run, t, 0, 0, k, st, _witness_values(run))
        _check_record(st)
        _tally_entry(run, tally, 0, k, st)
        log(f"round {tally['rounds']} picked {k} kept {int(st[S.FS_KEPT])} closed {int(st[S.FS_CLOSED])} infeasible {int(st[S.FS_INFEASIBLE])} "
            f"open {int(st[S.FS_N_OPEN])} lb {_global_lb(st):.5f} ub {st[S.FS_GLOBAL_UB]:.5f}")
    run.check_status()
    if stats is not None:
        stats.update({key: tally[key] for key in ("branches", "kw_bounded", "domains_bounded")},
                     kw_used=int(run.n_used.cpu()[0]) if run.threshold is not None else 0)
        if run.online is not None:
            stats.update(online_steps=run.online_steps, online_rows=run.online_rows)
        if run.strong_on:
            stats.update(strong_bounded=tally["strong_bounded"])
        if run.imitate is not None:
            stats.update(imitation_steps=run.imitation_steps, imitation_rows=run.imitation_rows)
        if run.replay is not None:
            stats.update(replay_stored=run.replay_stored, replay_skipped=run.replay_skipped, replay_filled=run.replay_filled)
    return global_lb, global_ub, tally["rounds"], tally["domains_bounded"], reason


# ---- the report of a round, per plan entry: a one-job round is the entry (segment 0, row 0, k) -------------------------------------------
def _report_launched(run, trace, e, row0, k, tag):
    """The first half of the report of entry number ``e`` of the round just launched, the parent rows [row0, row0 + k), before
    ``read_state`` (device-to-host copies; a traced or audited run only).  Appends the entry's dict to ``trace`` (unless None) and returns
    it: ``tag``, ``_trace_rows``, the threshold part, and in "strong" mode the candidates and their improvements per parent; extends
    ``run.strong_audit`` (unless None) by ``_strong_rows``' dicts with ``tag``.  tag: {} in a one-job run, the entry's "job", "segment"
    and "round" in a many-jobs run.  (A round that computed no table -- ``cand_entry`` None -- has no strong rows.)"""
    t = None
    if trace is not None:
        t = {**tag, **_trace_rows(run, row0, row0 + k)}
        if run.threshold is not None:
            t.update(_threshold_trace(run, k, e, row0))
        trace.append(t)
    traced_strong = t is not None and run.branching == "strong"
    if (traced_strong or run.strong_audit is not None) and run.cand_entry is not None:
        rows = _strong_rows(run, k, row0)
        if traced_strong:
            t.update(strong_candidates=[r["candidates"] for r in rows], strong_improvement=[r["improvements"] for r in rows])
            if rows and "sources" in rows[0]:                     # (a run with a gnn count, section 7.14)
                t.update(strong_sources=[r["sources"] for r in rows])
        if run.strong_audit is not None:
            run.strong_audit.extend({**r, **tag} for r in rows)
    return t


def _witness_values(run):
    """The ONE host copy of ``best_value`` a traced round of a run with a witness makes, behind ``read_state`` (None without a witness)."""
    return run.best_value.cpu().tolist() if run.witness_on else None


def _report_read(run, t, seg, row0, k, st, values):
    """The second half, behind ``read_state``, into the entry's trace dict ``t``: on a learning round that took a step the loss, regret
    and report of the entry's rows; in a run with ``imitate`` the bounds of the entry's record ``st`` after the round; in a run with a
    witness global_ub and the device's copy of it, element ``seg`` of ``values`` (``_witness_values``)."""
    a, b = row0, row0 + k
    replay = getattr(run, "last_replay", None)                    # (section 7.16: a learning round of a run with a buffer that read its state)
    if replay is not None:
        t.update(replay_stored=replay["stored"], replay_skipped=replay["skipped"], replay_filled=replay["filled"])
        if replay["steps"]:
            S, n = replay["steps"], replay["batch"]

            def fill_replay(kept=None):                           # the per-step draws and what each step reported of them
                t.update(replay_idx=run.rp_idx[:S, :n].cpu().tolist(), replay_loss=run.rp_loss[:S, :n].cpu().tolist(),
                         replay_regret=run.rp_regret[:S, :n].cpu().tolist(), replay_report=run.rp_report[:S, :n].cpu().tolist())
            pending = getattr(run, "pending_step", None)
            if pending is not None:
                pending["fill"].append(fill_replay)
            else:
                fill_replay()
        t.update(global_lb=_global_lb(st), global_ub=st[_lib.FS_GLOBAL_UB])
    elif run.imitate is not None:
        if run.last_imitation:
            def fill(kept=None):
                t.update(imitation_loss=run.im_loss[a:b].cpu().tolist(), imitation_regret=run.im_regret[a:b].cpu().tolist(),
                         imitation_report=run.im_report[a:b].cpu().tolist())
            # repack "device": with the next round's state record.  (getattr: tests/test_frontier_cpu.py reports through a stand-in run
            # that is no _Round and holds only what the report read before this option)
            pending = getattr(run, "pending_step", None)
            if pending is not None:
                pending["fill"].append(fill)
            else:
                fill()
        t.update(global_lb=_global_lb(st), global_ub=st[_lib.FS_GLOBAL_UB])
    if run.witness_on:
        t.update(global_ub=st[_lib.FS_GLOBAL_UB], witness_value=values[seg])


def _new_tally():
    """The tally of a job whose root has been bounded."""
    return {"rounds": 0, "domains_bounded": 1, "branches": 0, "kw_bounded": 0, "strong_bounded": 0}


def _tally_entry(run, tally, e, k, st):
    """Entry number ``e`` of the round just read, k parents with the record ``st``, added to its job's tally: the round, the domains
    bounded (what the commit kept, closed or found infeasible, and in threshold mode both children of the entry's m KW pairs), the
    parents branched, the KW pairs bounded and the candidate children (none in a round without a table)."""
    m = run.m_e[e] if run.threshold is not None else 0
    c = run.cand_entry
    tally["rounds"] += 1
    tally["domains_bounded"] += int(st[_lib.FS_KEPT] + st[_lib.FS_CLOSED] + st[_lib.FS_INFEASIBLE]) + 2 * m
    tally["branches"], tally["kw_bounded"] = tally["branches"] + k, tally["kw_bounded"] + m
    if c is not None:
        tally["strong_bounded"] += 2 * (c[e + 1] - c[e])


def _strong_rows(run, k, row0=0):
    """One dict per parent of the rows [row0, row0 + k) of the round just launched (device-to-host copies; a traced or audited run
    only): its slot, the decision the round committed and that decision's improvement from the round's own children, the table's decision
    and best improvement, and the row's candidates (flat ReLU indices) with their improvements and, in a run with a gnn count (DESIGN.md section
    7.14), their "sources" (1: BaBSR's shortlist only, 2: the scorer's only, 3: both).  A one-job round is the rows [0, k); an
    entry of a many-jobs round its own, whose candidates are the range [cand0[row0], cand0[row0 + k]) of the lists."""
    from .bab_caller import gnn_improvement
    inf, nan = float("inf"), float("nan")
    Ch, r1 = run.Ch, row0 + k
    off = [0]
    for s in run.eng.sizes[1:-1]:
        off.append(off[-1] + s)
    slots = run.slots[row0:r1].cpu().tolist()
    dec = run.P.dec[row0:r1].cpu().tolist()
    s_dec = dec if run.branching == "strong" else run.s_dec[row0:r1].cpu().tolist()
    parent = run.parent_bound[row0:r1].cpu().tolist()
    live, infeasible, bound = (t[2 * row0:2 * r1].cpu().tolist() for t in (Ch.live, Ch.infeasible, Ch.bound))
    cand0, best = run.cand0[row0:r1 + 1].cpu().tolist(), run.s_best[row0:r1].cpu().tolist()
    q0 = cand0[0]
    cand0 = [q - q0 for q in cand0]
    cand_dec, imp = run.cand_dec[q0:q0 + cand0[-1]].cpu().tolist(), run.s_imp[q0:q0 + cand0[-1]].cpu().tolist()
    src = None                                                    # (a run without a gnn count is the run it was: no "sources")
    if getattr(run, "strong_G", 0):                               # the union's cand_src; the scorer's shortlist alone: every candidate is its own
        src = [2] * cand0[-1] if getattr(run, "cand_src", None) is None else run.cand_src[q0:q0 + cand0[-1]].cpu().tolist()
    rows = []
    for i in range(k):
        lbs = [inf if infeasible[c] else bound[c] for c in (2 * i, 2 * i + 1)]
        own = nan if not (live[2 * i] and live[2 * i + 1]) else (gnn_improvement(lbs[0], lbs[1], parent[i]) if parent[i] < 0 else 1.0)
        a, b = cand0[i], cand0[i + 1]
        rows.append({"slot": slots[i], "decision": dec[i], "improvement": own, "strong_decision": s_dec[i], "best_improvement": best[i],
                     "candidates": [off[l] + j for l, j in cand_dec[a:b]], "improvements": imp[a:b]})
        if src is not None:
            rows[-1]["sources"] = src[a:b]
    return rows


def _online_trace(run, st, t=None):
    """The online mode's part of a round's trace, behind ``read_state`` (device-to-host copies): the learn rows of the round just read, the
    flat indices of their KW nodes, improve and the loss of each row in the step; the bounds of the record ``st``.  Behind a step that was
    only issued (repack "device") the step's four keys go into the round's dict ``t`` with the next round's state record, from the
    copies ``_step_issued`` kept (the next launch overwrites the learn rows)."""
    n = run.last_learn if run.m else 0
    out = {"global_lb": _global_lb(st), "global_ub": st[_lib.FS_GLOBAL_UB]}

    def step_part(kept):
        return {"learn_rows": kept["learn_rows"][:n].cpu().tolist(), "learn_kw": kept["learn_kw"][:n].cpu().tolist(),
                "learn_improve": kept["learn_imp"][:n].cpu().tolist(), "loss": run.loss[:n].cpu().tolist()}
    pending = getattr(run, "pending_step", None)                  # (as in _report_read)
    if pending is not None and n and t is not None:
        pending["fill"].append(lambda kept: t.update(step_part(kept)))
    else:
        out.update(step_part({"learn_rows": run.learn_rows, "learn_kw": run.learn_kw, "learn_imp": run.learn_imp}))
    return out


def _online_entry_trace(run, t, e, row0, st):
    """``_online_trace`` for entry number ``e`` of a many-jobs round, into the entry's dict ``t``: the entry's
    slice of the dense lists -- it starts at the sum of the counts of the entries before it (``learn_e``), and "learn_rows" count from
    the entry's first row ``row0``, as "selected" does -- and the bounds of the entry's record ``st``.  Behind a step that was only issued
    the four keys arrive with the next round's records, from the copies ``_step_issued`` kept."""
    a = sum(run.learn_e[:e])
    b = a + run.learn_e[e]
    t.update(global_lb=_global_lb(st), global_ub=st[_lib.FS_GLOBAL_UB])

    def fill(kept):
        t.update(learn_rows=[r - row0 for r in kept["learn_rows"][a:b].cpu().tolist()], learn_kw=kept["learn_kw"][a:b].cpu().tolist(),
                 learn_improve=kept["learn_imp"][a:b].cpu().tolist(), loss=run.loss[a:b].cpu().tolist())
    if run.pending_step is not None and run.learn_e[-1]:
        run.pending_step["fill"].append(fill)
    else:
        fill({"learn_rows": run.learn_rows, "learn_kw": run.learn_kw, "learn_imp": run.learn_imp})


def _threshold_trace(run, k, e=0, row0=0):
    """The threshold mode's part of a round's trace (device-to-host copies) for entry number ``e`` of the round's plan, the parent rows
    [row0, row0 + k); a one-job round is a plan of one entry.  The entry's range of the dense lists starts at the sum of the m of the
    entries before it, and "selected" counts from the entry's first row.  With M = 0 no choice was launched: every row kept its GNN pair."""
    P, ChB, M, m = run.P, run.ChB, run.M, run.m_e[e]
    a, b, q0 = row0, row0 + k, sum(run.m_e[:e])
    q1 = q0 + m
    gnn_dec = P.dec[a:b].cpu().tolist()
    a_bound, a_inf = run.pair_a
    return {"gnn_decisions": gnn_dec, "gnn_improvement": run.gnn_imp[a:b].cpu().tolist(), "kw_decisions": run.kw_dec[a:b].cpu().tolist(),
            "kw_improvement": run.kw_imp[a:b].cpu().tolist() if M else [-1.0] * k, "selected": [r - row0 for r in run.sel_rows[q0:q1].cpu().tolist()],
            "used_kw": run.used_kw[a:b].cpu().tolist() if M else [0] * k, "decisions": run.dec[a:b].cpu().tolist() if M else gnn_dec,
            "gnn_child_bounds": a_bound[2 * a:2 * b].cpu().tolist(), "gnn_child_infeasible": a_inf[2 * a:2 * b].cpu().tolist(),
            "kw_child_bounds": ChB.bound[2 * q0:2 * q1].cpu().tolist(), "kw_child_infeasible": ChB.infeasible[2 * q0:2 * q1].cpu().tolist()}


# ---- many jobs in one pool --------------------------------------------------------------------------------------
class FrontierJob:
    """One verification job on the bound network: the box [input_lb, input_ub], the folded property layer Linear(N_L, 1) and the decision
    bound (None: run to the gap)."""

    def __init__(self, input_lb, input_ub, prop_layer, decision_bound=None):
        self.input_lb, self.input_ub, self.prop_layer, self.decision_bound = input_lb, input_ub, prop_layer, decision_bound


def _global_lb(st):
    return min(st[_lib.FS_LOWEST_OPEN], st[_lib.FS_CLOSED_LB], st[_lib.FS_GLOBAL_UB])


def _stop_reason(st, eps, decision_bound, rounds, max_rounds):
    """``branch_and_bound_frontier``'s stop conditions on a record, but for "capacity", which ``plan_round`` decides."""
    global_lb, global_ub = _global_lb(st), st[_lib.FS_GLOBAL_UB]
    if int(st[_lib.FS_N_OPEN]) == 0:
        return "exhausted"
    if not global_ub - global_lb > eps:
        return "gap"
    if decision_bound is not None and (global_lb >= decision_bound or global_ub < decision_bound):
        return "decision"
    if rounds >= max_rounds:
        return "max_rounds"
    return None


def plan_round(records, K, cap):
    """The plan of a round from the host's copy of the records: a pure function.  records: per segment its record (a sequence of
    ``_lib.FRONTIER_STATE_DOUBLES`` numbers), or None for a segment that takes no part (free, or its job has stopped).

    Returns (entries, compact, stopped).  entries: [(segment, row0, k)] in segment order with k = min(K, open domains of the segment) and
    row0 the running sum of k; compact: per segment, whether it must be compacted before the round (slots in use + k > cap, as
    ``branch_and_bound_frontier`` does for its pool); stopped: the segments whose open domains leave no room for k more (open + k > cap:
    the "capacity" stop), which get no entry.  A segment without an open domain gets no entry either."""
    entries, compact, stopped, row0 = [], [False] * len(records), [], 0
    for s, st in enumerate(records):
        if st is None:
            continue
        n_open, in_use = int(st[_lib.FS_N_OPEN]), int(st[_lib.FS_IN_USE])
        k = min(K, n_open)
        if k < 1:
            continue
        if n_open + k > cap:
            stopped.append(s)
            continue
        compact[s] = in_use + k > cap
        entries.append((s, row0, k))
        row0 += k
    return entries, compact, stopped


def _one_job_round(st, K, capacity, eps, decision_bound, rounds, max_rounds):
    """What ``branch_and_bound_frontier`` does on the record ``st``: (reason, k, compact) -- a stop reason, or None and a round of k parents
    after a compaction of the pool if ``compact``.  The rule is ``verify_properties``' for a pool of one segment."""
    reason = _stop_reason(st, eps, decision_bound, rounds, max_rounds)
    if reason is not None:
        return reason, 0, False
    entries, compact, stopped = plan_round([st], K, capacity)
    if stopped:
        return "capacity", 0, False
    return None, entries[0][2], compact[0]


def round_depth(k, K, D, n_open, cap):
    """The depth of a round of k parents in a run with ``split_depth`` = D: a pure function of what the host
    holds.  The largest d in 1..D with k 2^d <= 2K (the round's child rows) and n_open + (2^d - 1) k <= cap (a compacted pool holds every
    child: k of them reuse the parents' slots); 0 when not even d = 1 fits -- the "capacity" stop.  k = K gives 1 at most."""
    best = 0
    for d in range(1, D + 1):
        if k << d <= 2 * K and n_open + ((1 << d) - 1) * k <= cap:
            best = d
    return best


def _one_job_round_depth(st, K, D, capacity, eps, decision_bound, rounds, max_rounds):
    """``_one_job_round`` for a run with ``split_depth`` = D: (reason, k, compact, d) -- a stop reason, or None and a round of k parents at
    depth d after a compaction of the pool if ``compact`` (slots in use + (2^d - 1) k > capacity).  At D = 1 it is ``_one_job_round``."""
    reason = _stop_reason(st, eps, decision_bound, rounds, max_rounds)
    if reason is not None:
        return reason, 0, False, 0
    n_open, in_use = int(st[_lib.FS_N_OPEN]), int(st[_lib.FS_IN_USE])
    k = min(K, n_open)
    d = round_depth(k, K, D, n_open, capacity)
    if d == 0:
        return "capacity", 0, False, 0
    return None, k, in_use + ((1 << d) - 1) * k > capacity, d


def _check_record(st):
    if st[_lib.FS_OVERFLOW] != 0 or math.isnan(st[_lib.FS_GLOBAL_UB]):
        raise RuntimeError(f"frontier state record is inconsistent: {st}")


def _trace_rows(run, a, b):
    """A round's trace of the parent rows [a, b) and their children (device-to-host copies)."""
    depth = getattr(run, "depth", 0)                               # (section 7.20: 2^depth children per parent; a stand-in run has none)
    P, Ch, C = run.P, run.Ch, 1 << depth if depth else 2
    c, d = C * a, C * b
    t = {"slots": run.slots[a:b].cpu().tolist(), "parent_bounds": P.bound[a:b].cpu().tolist(), "decisions": P.dec[a:b].cpu().tolist(),
         "child_bounds": Ch.bound[c:d].cpu().tolist(), "child_ub": Ch.ubv[c:d].cpu().tolist(), "live": Ch.live[c:d].cpu().tolist(),
         "infeasible": Ch.infeasible[c:d].cpu().tolist()}
    if depth:
        c0 = run.cand0[a:b + 1].cpu().tolist()
        dec = run.cand_dec[c0[0]:c0[-1]].cpu().tolist()
        t.update(depth=depth, nodes=[dec[q0 - c0[0]:q1 - c0[0]] for q0, q1 in zip(c0, c0[1:])])
    return t


class RoundPlan:
    """A plan on both sides of the link: ``host`` is pinned, ``device`` receives it by a non_blocking copy (3 int32 per entry)."""

    def __init__(self, device, max_entries, segments, seg_cap):
        self.host = torch.zeros(max_entries, 3, dtype=torch.int32).pin_memory()
        self.device = torch.zeros(max_entries, 3, dtype=torch.int32, device=device)
        self.n_entries, self.n, self.segments, self.seg_cap = 0, 0, segments, seg_cap

    def send(self, entries):
        self.n_entries, self.n = len(entries), sum(e[2] for e in entries)
        self.host[:len(entries)] = torch.tensor(entries, dtype=torch.int32).reshape(-1, 3)
        self.device.copy_(self.host, non_blocking=True)


def _check_jobs_args(jobs, K, segments, capacity, n_iter, lr, eps, max_rounds):
    jobs = list(jobs)
    if not jobs:
        raise ValueError("no job")
    if not isinstance(K, int) or isinstance(K, bool) or K < 1:
        raise ValueError(f"K = {K!r}: a positive integer")
    if capacity is None:
        capacity = max(256, 4 * K + 1)
    capacity = _check_args(K, n_iter, lr, eps, max_rounds, capacity)
    if segments is None:
        segments = max(1, min(len(jobs), 64, 16383 // K))
    if not isinstance(segments, int) or isinstance(segments, bool) or segments < 1 or segments * K > 16383:
        raise ValueError(f"segments = {segments!r}: a positive integer with segments * K <= 16383 (a full round's 2n child rows stay within 32767)")
    if segments * capacity > 2 ** 31 - 1:
        raise ValueError(f"{segments} segments of {capacity} slots: more than 2^31 - 1 slots")
    shape = None
    for j, job in enumerate(jobs):
        if type(job.prop_layer) is not nn.Linear or job.prop_layer.out_features != 1:
            raise ValueError(f"job {j}: the property layer must be the folded Linear(., 1)")
        if tuple(job.input_lb.shape) != tuple(job.input_ub.shape) or (shape is not None and tuple(job.input_lb.shape) != shape):
            raise ValueError(f"job {j}: every box must have one input shape")
        shape = tuple(job.input_lb.shape)
    return jobs, segments, capacity, shape


class JobsRun(_Round):
    """The device side of ``verify_properties``: a pool of ``segments`` segments of ``cap`` slots with one record each, the jobs' boxes and
    property rows as device tables, and the rows of a round of up to segments * K parents.  ``launch_roots`` / ``launch_round`` are device
    work only; ``read_state`` is the one synchronising copy.

    With a ``branching_threshold`` (``verify_properties_threshold``) the run also owns, per segment, the intercept
    counter ``icp`` and the table ``ineff`` of inefficient KW points, a second set of child rows with boxes of its own, and a round reads
    one more array, ``m_entry`` (``read_selected``), between its two halves."""

    def __init__(self, choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps, branching_threshold=None, kwbd_threshold=KWBD_DEFAULT,
                 sparsest_layer=0, decision_threshold=0.001, witness=None, pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None,
                 pgd_seed=0, branching="gnn"):
        self._set_options(choice, branching=branching, branching_threshold=branching_threshold, kwbd_threshold=kwbd_threshold, sparsest_layer=sparsest_layer,
                          decision_threshold=decision_threshold, witness=witness, pgd_steps=pgd_steps, pgd_step=pgd_step, pgd_restarts=pgd_restarts,
                          pgd_seed=pgd_seed)
        self._make(choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps)

    def _make(self, choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps):
        """The pool, the jobs' tables and the rows of a run whose options are set (``_set_options``)."""
        self.K, self.S, self.cap, self.n_iter, self.lr, self.eps = K, segments, cap, n_iter, float(lr), float(eps)
        self.fixed = list(fixed_layers)
        eng = self.eng = self._engine_of(choice)
        self._use_repack()
        eng.bind(self.fixed, in_shape)
        dev, self.lib, self.ng = eng.device, eng.lib, len(eng.sizes)
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        N0, NL, S, n = eng.sizes[0], eng.sizes[-2], segments, segments * K
        self.pool = DomainPool(eng, S * cap)
        self.start = torch.tensor(_start_record(), dtype=f64, device=dev)
        self.pool.state = self.start.repeat(S, 1)
        # the jobs (J, .) and what the segments hold of them (S, .)
        self.job_x_lo = torch.stack([j.input_lb.reshape(-1) for j in jobs]).to(dev, f64)
        self.job_x_hi = torch.stack([j.input_ub.reshape(-1) for j in jobs]).to(dev, f64)
        self.job_pw = torch.stack([j.prop_layer.weight.detach().reshape(-1) for j in jobs]).to(dev, f32)
        self.job_pb = torch.stack([j.prop_layer.bias.detach().reshape(()) for j in jobs]).to(dev, f32)
        self.job_db = torch.tensor([float("nan") if j.decision_bound is None else float(j.decision_bound) for j in jobs], dtype=f64).to(dev)
        self.seg_x_lo, self.seg_x_hi = torch.zeros(S, N0, dtype=f64, device=dev), torch.zeros(S, N0, dtype=f64, device=dev)
        self.seg_pw, self.seg_pb = torch.zeros(S, NL, dtype=f32, device=dev), torch.zeros(S, dtype=f32, device=dev)
        self.seg_db = torch.full((S,), float("nan"), dtype=f64, device=dev)
        # the rows' boxes and property rows: the parents' and the children's (k_frontier_rows_jobs fills both)
        self.px_lo, self.px_hi = torch.zeros(n, N0, dtype=f64, device=dev), torch.zeros(n, N0, dtype=f64, device=dev)
        self.ppw, self.ppb = torch.zeros(n, NL, dtype=f32, device=dev), torch.zeros(n, dtype=f32, device=dev)
        self.x_lo, self.x_hi = torch.zeros(2 * n, N0, dtype=f64, device=dev), torch.zeros(2 * n, N0, dtype=f64, device=dev)
        self.pw, self.pb = torch.zeros(2 * n, NL, dtype=f32, device=dev), torch.zeros(2 * n, dtype=f32, device=dev)
        self._buffers(n, 2 * n, in_shape, (self.px_lo, self.px_hi, self.ppw, self.ppb))
        self.root_rows = 2 * S
        self.ws_commit = self._ws("gnnb_frontier_commit_jobs_workspace_bytes", n)
        self._witness_buffers(S)
        if self.witness_on:
            self.job_point = torch.zeros(len(jobs), N0, dtype=f32, device=dev)       # a job's witness, once it has left
        self.slots, self.row_seg = torch.zeros(n, dtype=i32, device=dev), torch.zeros(n, dtype=i32, device=dev)
        self.plan = RoundPlan(dev, S, S, cap)
        self.root_live = torch.tensor([1, 0] * S, dtype=i32).to(dev)
        self.flags_host = torch.zeros(S, dtype=i32).pin_memory()
        self.flags = torch.zeros(S, dtype=i32, device=dev)
        self.slot_seg = torch.arange(S * cap, device=dev) // cap
        self.m_e, self.M = [0], 0
        if self.threshold is not None:
            # pair B's rows belong to the selected parents' jobs: boxes and property rows of their own (gnnb_frontier_fallback_jobs fills them)
            self.bx_lo, self.bx_hi = torch.zeros(2 * n, N0, dtype=f64, device=dev), torch.zeros(2 * n, N0, dtype=f64, device=dev)
            self.bpw, self.bpb = torch.zeros(2 * n, NL, dtype=f32, device=dev), torch.zeros(2 * n, dtype=f32, device=dev)
            # per segment: the counter, the table and n_used, the KW pairs taken since its job was admitted
            self._threshold_buffers(n, ((S,), (S, eng.R)), (self.bx_lo, self.bx_hi, self.bpw, self.bpb), "gnnb_frontier_fallback_jobs_workspace_bytes")
            self.m_entry = torch.zeros(S + 1, dtype=i32, device=dev)
            self.job_used = torch.zeros(len(jobs), dtype=torch.int64, device=dev)    # KW pairs taken per job, once it has left
        if self.branching == "babsr":                             # per segment: the intercept counter of its job (section 7.10)
            self._babsr_buffers(n, (S,))

    def release(self, seg):
        """The job of segment ``seg`` leaves: no open slot, the start record."""
        self.pool.open[seg * self.cap:(seg + 1) * self.cap].zero_()
        self.pool.state[seg].copy_(self.start)

    def admit(self, seg, job):
        """Job number ``job`` takes the (released) segment ``seg``: its box, property row and decision bound, device to device."""
        self.seg_x_lo[seg].copy_(self.job_x_lo[job])
        self.seg_x_hi[seg].copy_(self.job_x_hi[job])
        self.seg_pw[seg].copy_(self.job_pw[job])
        self.seg_pb[seg].copy_(self.job_pb[job])
        self.seg_db[seg].copy_(self.job_db[job])
        if self.witness_on:                                       # no incumbent yet
            self.best_value[seg].fill_(float("inf"))
        if self.threshold is not None:                            # the job starts with its own counter and table: zero, device-side
            self.icp[seg].zero_()
            self.ineff[seg].zero_()
            self.n_used[seg].zero_()
        if self.branching == "babsr":                             # the job starts with its own counter: zero, device-side
            self.icp[seg].zero_()

    def keep_used(self, seg, job):
        """The job of segment ``seg`` leaves: its count of KW pairs taken, device to device (read once, when the run ends)."""
        self.job_used[job].copy_(self.n_used[seg])

    def keep_witness(self, seg, job):
        """The job of segment ``seg`` leaves: its incumbent's point, device to device (read once, when the run ends)."""
        self.job_point[job].copy_(self.best_point[seg])

    def _witness(self, n, M):
        """gnnb_frontier_witness_jobs on the rows the commit will see."""
        self.eng.frontier_witness_jobs(self.plan, self.Ch, self._ub_points(self.Ch), self.best_value, self.best_point, M=M,
                                       m_entry=self.m_entry if M else None, **self._pair_b_source(M))

    def _commit(self, slots):
        self.eng.frontier_commit_jobs(self.pool, self.plan, slots, *self.Ch.children(), self.pool.state, self.seg_db, eps=self.eps,
                                      workspace=self.ws_commit)

    def _rows_of_plan(self):
        self.eng.frontier_rows_jobs(self.plan, self.row_seg, self.seg_x_lo, self.seg_x_hi, self.seg_pw, self.seg_pb, self.px_lo, self.px_hi, self.ppw,
                                    self.ppb, self.x_lo, self.x_hi, self.pw, self.pb)

    def launch_roots(self, segs):
        """The root phase: the roots of the jobs just admitted to ``segs`` (ascending), one plan entry of k = 1 each.  Child row 2e is the
        root of entry e -- every ReLU undecided, no parent, the default start of the ascent -- and row 2e + 1 its dead sibling (the same
        problem, live = 0); the commit puts the root into the segment's first slot, as ``FrontierRun.root`` enters its pool."""
        E, Ch = len(segs), self.Ch
        self.plan.send([(s, e, 1) for e, s in enumerate(segs)])
        self.row_seg[:E] = self.plan.device[:E, 0]
        self.slots[:E] = self.plan.device[:E, 0] * self.cap
        self._rows_of_plan()
        Ch.mask[:2 * E].fill_(-1)
        Ch.split[:2 * E].fill_(-1)
        Ch.live[:2 * E] = self.root_live[:2 * E]
        self._bound_children(Ch, 2 * E, warm=False, tighten=self.tighten_root)
        if self.witness_on:
            self._witness(E, 0)
        self._commit(self.slots[:E])

    def compact(self, flagged):
        """``DomainPool.compact``'s rule inside every segment of ``flagged`` (a list of booleans per segment), the others left in place: one
        stable sort of the whole pool on the key 2 segment + (segment flagged and slot closed), then indexing.  No synchronisation."""
        pool = self.pool
        self.flags_host.copy_(torch.tensor(flagged, dtype=torch.int32))
        self.flags.copy_(self.flags_host, non_blocking=True)
        flag = self.flags[self.slot_seg] > 0
        pool.reorder(torch.sort(2 * self.slot_seg + (flag & (pool.open == 0)), stable=True).indices)
        pool.state[:, _lib.FS_IN_USE] = torch.where(self.flags > 0, pool.state[:, _lib.FS_N_OPEN], pool.state[:, _lib.FS_IN_USE])

    def launch_round(self, entries):
        """One round over the plan's entries [(segment, row0, k)], launched round number ``round`` of the run (``_begin_round``).  Device
        work only -- but for the one read of a run with a table, ``StrongJobsRun.read_candidates``."""
        self.plan.send(entries)
        self._begin_round(self.plan.n)
        self.eng.frontier_pick_jobs(self.pool, self.plan, self.pool.state, self.slots, self.row_seg)
        self._rows_of_plan()
        self._launch(self.slots[:self.plan.n], self.plan.n)

    # ``_Round._fall_back``'s steps for the jobs of a plan: the selection and the choice per entry, the read of m_entry
    def _select(self, n):
        Ch = self.Ch
        self.eng.frontier_fallback_jobs(self.pool, self.plan, self.slots, Ch.live, Ch.infeasible, Ch.bound, self.kw_scores, self.kw_icp, self.P.amb, self.icp,
                                        self.ineff, self.seg_x_lo, self.seg_x_hi, self.seg_pw, self.seg_pb, self.gnn_imp, self.kw_dec, self.sel_rows,
                                        self.sel_slots, self.sel_dec, self.m_entry, self.bx_lo, self.bx_hi, self.bpw, self.bpb, self.threshold,
                                        self.kwbd_threshold, self.sparsest_layer, self.decision_threshold, self.random_order, workspace=self.ws_fallback)

    def _decide(self, n):
        self.eng.frontier_babsr_decide_jobs(self.plan, self.kw_scores, self.kw_icp, self.P.amb, self.icp, self.P.dec, self.sparsest_layer,
                                            self.decision_threshold, self.random_order, workspace=self.ws_babsr)

    def _read_selected(self):
        self.m_e = self.read_selected()
        self.M = self.m_e[-1]
        return self.M

    def _choose(self, n, M):
        self.eng.frontier_choose_jobs(self.pool, self.plan, M, self.m_entry, self.sel_rows, self.sel_slots, self.sel_dec, self.P.dec, self.gnn_imp, self.Ch,
                                      self.ChB, self.ineff, self.kw_imp, self.used_kw, self.dec)
        self.n_used.index_add_(0, self.row_seg[:n].long(), self.used_kw[:n].long())

    def read_selected(self):
        """m per plan entry, then their sum M: the 4 (entries + 1) bytes a threshold round reads between its halves."""
        return self.m_entry[:self.plan.n_entries + 1].cpu().tolist()

    def read_state(self):
        """The (segments, 9) records as lists of Python floats: the one device-to-host copy of a round (of its second half, in threshold
        mode)."""
        return self.pool.state.cpu().tolist()


def _check_jobs_strong(branching, strong_audit, imitate):
    """The modes of a many-jobs run with a table: "strong", or "gnn" next to an audit or the imitation step."""
    if branching == "babsr":
        raise ValueError('branching="babsr": verify_properties_babsr runs the jobs on BaBSR alone; a table next to it is not built for many jobs')
    if branching == "gnn" and strong_audit is None and imitate is None:
        raise ValueError('branching="gnn" with neither strong_audit nor imitate: nothing would compute a table; verify_properties runs the jobs on the GNN')


class StrongJobsRun(JobsRun):
    """The device side of ``verify_properties_strong``: ``JobsRun`` with the table of section 7.11 over the parent
    rows of ALL entries of a round and, with ``imitate`` = N, the step of section 7.12 behind every N-th launched round.  The candidates
    of a round form one dense list over all its jobs; a chunk may span parents and jobs, so in front of every chunk
    ``gnnb_strong_rows_jobs`` gives each candidate's two child rows their own job's box and property row.  ``launch_round`` is device work
    only but for the round's one extra read, ``read_candidates``: 4 (entries + 1) bytes."""

    def __init__(self, choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps, branching_threshold=None, kwbd_threshold=KWBD_DEFAULT,
                 sparsest_layer=0, decision_threshold=0.001, witness=None, pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None,
                 pgd_seed=0, imitate=None, imitate_margin=IMITATE_MARGIN_DEFAULT, strong_candidates=None, strong_chunk=STRONG_CHUNK_DEFAULT,
                 strong_audit=None, branching="strong"):
        self._set_options(choice, branching=branching, branching_threshold=branching_threshold, kwbd_threshold=kwbd_threshold, sparsest_layer=sparsest_layer,
                          decision_threshold=decision_threshold, witness=witness, pgd_steps=pgd_steps, pgd_step=pgd_step, pgd_restarts=pgd_restarts,
                          pgd_seed=pgd_seed, imitate=imitate, imitate_margin=imitate_margin, strong_candidates=strong_candidates,
                          strong_chunk=strong_chunk, strong_audit=strong_audit)
        _check_jobs_strong(branching, strong_audit, imitate)
        self._make(choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps)      # (``JobsRun``'s, on the options set here)
        eng, dev, n = self.eng, self.eng.device, segments * K
        f64, f32 = torch.float64, torch.float32
        N0, NL, rows = eng.sizes[0], eng.sizes[-2], 2 * strong_chunk
        # the candidates' rows belong to the jobs of their parents: boxes and property rows of their own (gnnb_strong_rows_jobs fills them)
        self._strong_buffers(n, (torch.zeros(rows, N0, dtype=f64, device=dev), torch.zeros(rows, N0, dtype=f64, device=dev),
                                 torch.zeros(rows, NL, dtype=f32, device=dev), torch.zeros(rows, dtype=f32, device=dev)))
        self.cand_idx = torch.zeros(segments + 1, dtype=torch.int64, device=dev)      # the rows of cand0 a round reads: every entry's row0, and n
        self._imitation_buffers(n)

    def _strong_chunk_rows(self, q0, c):
        box = self.ChS.box
        self.eng.strong_rows_jobs(self.cand_slot[q0:q0 + c], c, self.S, self.cap, self.seg_x_lo, self.seg_x_hi, self.seg_pw, self.seg_pb, *box)

    def read_candidates(self, n):
        """cand0 at every entry's first row and cand0[n]: the 4 (entries + 1) bytes a round with a table reads between the list and its
        chunks, in ONE copy.  The differences are the entries' candidates (``cand_entry`` keeps the list); the last is the round's."""
        E, idx = self.plan.n_entries, self.cand_idx
        idx[:E] = self.plan.device[:E, 1]
        idx[E] = n
        self.cand_entry = self.cand0[idx[:E + 1]].cpu().tolist()
        return self.cand_entry[-1]

    def _imitate(self):
        try:
            super()._imitate()
        except RuntimeError as e:                                 # (GNNB_E_NOMEM: the step's buffers grow with the rows of a round)
            if "(-4)" not in str(e):
                raise
            raise RuntimeError(f"the imitation step over the {self.k} parent rows of a round found no device memory: lower segments or K "
                               f"(segments * K = {self.S * self.K} rows at most per step)") from e

    def read_state(self):
        """``JobsRun.read_state``; a learning round then takes its step (``_imitate``), behind the records."""
        st = super().read_state()
        self._settle_step()                                       # ("device" mode: the previous round's step, read behind these records)
        self._step_behind_read()
        return st


class OnlineJobsRun(JobsRun):
    """The device side of ``verify_properties_online``: ``JobsRun`` in threshold mode with section 7.7's online
    learning per job.  Every segment owns a wrong-point table ``wrong[segment]`` ((R,) int32, zero when its job is admitted); behind the
    choice ``gnnb_frontier_learn_jobs`` selects the learn rows per plan entry into ONE dense list over all jobs, and a round with M > 0
    reads ``learn_entry`` (4 (entries + 1) bytes) behind the records and, with N > 0, takes ONE ``gnnb_online_step_rows`` over the learn
    rows of all jobs in flight, which share the scorer.  The constructor takes ``JobsRun``'s parameters, then ``online_threshold`` and
    ``repack``; ``kwbd_threshold`` stays at its default (the online loop has no table of inefficient KW points: the run uses KWBD_NEVER)."""

    def __init__(self, choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps, branching_threshold=None, kwbd_threshold=KWBD_DEFAULT,
                 sparsest_layer=0, decision_threshold=0.001, witness=None, pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None,
                 pgd_seed=0, branching="gnn", online_threshold=None, repack="host"):
        if online_threshold is None:
            raise ValueError("online_threshold = None: an integer >= 1 (JobsRun runs the jobs without online learning)")
        self._set_options(choice, branching=branching, branching_threshold=branching_threshold, kwbd_threshold=kwbd_threshold, sparsest_layer=sparsest_layer,
                          decision_threshold=decision_threshold, online_threshold=online_threshold, witness=witness, pgd_steps=pgd_steps, pgd_step=pgd_step,
                          pgd_restarts=pgd_restarts, pgd_seed=pgd_seed, repack=repack)
        self._make(choice, fixed_layers, jobs, in_shape, K, segments, cap, n_iter, lr, eps)      # (``JobsRun``'s, on the options set here)
        n = segments * K
        self._online_buffers(n, (segments, self.eng.R), segments + 1)      # one table per segment; the count array is learn_entry
        self.learn_entry, self.learn_e = self.learn_count, [0]
        self.ws_learn = self._ws("gnnb_frontier_learn_jobs_workspace_bytes", n)

    def admit(self, seg, job):
        """``JobsRun.admit``; the job starts with its own table of wrong points: zero, device-side."""
        super().admit(seg, job)
        self.wrong[seg].zero_()

    def launch_round(self, entries):
        self.learn_e, self.last_learn = [0] * (len(entries) + 1), 0      # (a round with M = 0 selects nothing and reads nothing)
        super().launch_round(entries)

    def _choose(self, n, M):
        """``JobsRun._choose``, then the learn rows of every entry (section 7.19): read behind the records."""
        super()._choose(n, M)
        self.eng.frontier_learn_jobs(self.plan, self.P.dec, self.kw_dec, self.used_kw, self.gnn_imp, self.kw_imp, self.online, self.wrong,
                                     self.learn_rows, self.learn_kw, self.learn_imp, self.learn_entry, workspace=self.ws_learn)
        self.learn_pending = True

    def read_learn(self):
        """The learn rows per plan entry, then their sum N: the 4 (entries + 1) bytes an online round with M > 0 reads behind the records
        (``learn_e`` keeps the list)."""
        self.learn_e = self.learn_entry[:self.plan.n_entries + 1].cpu().tolist()
        return self.learn_e[-1]

    def _learn(self):
        try:
            super()._learn()
        except RuntimeError as e:                                 # (GNNB_E_NOMEM: the step's buffers grow with the rows of a round)
            if "(-4)" not in str(e):
                raise
            raise RuntimeError(f"the online step over {self.last_learn} learn rows of the {self.k} parent rows of a round found no device memory: "
                               f"lower segments or K (segments * K = {self.S * self.K} rows at most per step)") from e

    def read_state(self):
        """``JobsRun.read_state``; an online round with M > 0 then reads learn_entry and takes its learning step (``_learn``)."""
        st = super().read_state()
        self._settle_step()                                       # ("device" mode: the previous round's step, read behind these records)
        if self.learn_pending:
            self._learn()
        return st


class FrontierJobs(list):
    """A list of ``FrontierJob`` together with the upper-bound options of the run that verifies them: how
    ``verify_properties`` and ``verify_properties_threshold`` take ``branch_and_bound_frontier``'s witness, pgd_steps and pgd_step.  (Their
    own parameter lists are fixed.)  pgd_restarts / pgd_seed: the restart options of section 7.9.  witness: None, or a list that receives one entry per job, in job order, when the run ends.
    tighten_root: ``branch_and_bound_frontier``'s (section 7.18), for the root of every job."""

    def __init__(self, jobs, witness=None, pgd_steps=None, pgd_step=PGD_STEP_DEFAULT, pgd_restarts=None, pgd_seed=0, tighten_root=0):
        super().__init__(jobs)
        _check_tighten(tighten_root)
        self.tighten_root = tighten_root                                       # (section 7.18)
        self.witness, self.pgd_steps, self.pgd_step = witness, pgd_steps, pgd_step
        self.pgd_restarts, self.pgd_seed = pgd_restarts, pgd_seed              # (section 7.9)


def _options_of(jobs):
    """The keywords of ``JobsRun`` a ``FrontierJobs`` carries ({} for any other sequence of jobs: everything off).  The run checks them."""
    if not isinstance(jobs, FrontierJobs):
        return {}
    return {"witness": jobs.witness, "pgd_steps": jobs.pgd_steps, "pgd_step": jobs.pgd_step, "pgd_restarts": jobs.pgd_restarts, "pgd_seed": jobs.pgd_seed}


def _tighten_of(jobs):
    """``FrontierJobs.tighten_root`` (0 for any other sequence of jobs); ``_Round.set_tighten_root`` checks it."""
    return jobs.tighten_root if isinstance(jobs, FrontierJobs) else 0


def verify_properties(choice, fixed_layers, jobs, K=16, segments=None, capacity=None, n_iter=20, lr=0.1, eps=1e-4, max_rounds=50, log=print, trace=None):
    """Branch and bound on many jobs at once: every job gets the result ``branch_and_bound_frontier`` gives it alone with
    ``capacity=capacity``, bit for bit, while a round's launches serve all the jobs in flight.

    choice: a ``GraphChoice``; fixed_layers: the network without a property layer (bound once); jobs: ``FrontierJob``s of one input shape.
    The pool is ``segments`` segments (None: min(len(jobs), 64, 16383 // K)) of ``capacity`` slots (None: max(256, 4K + 1)); a segment
    holds one job at a time.  Per iteration: the finished jobs leave, waiting jobs take the free segments in list order (lowest segment
    first) and their roots are bounded in a root phase; then one round expands the up-to-K open domains of lowest bound of every job in
    flight (``plan_round``).  K, n_iter, lr, eps, max_rounds are ``branch_and_bound_frontier``'s, per job.  A job whose root is infeasible
    ends with the reason "infeasible_root" and the bounds (+inf, +inf).  trace: None, or a list that receives per round and per entry a
    dict of the one-job trace's keys (slots are global: segment * capacity + the job's own) plus "job", "segment" and "round" (extra
    device-to-host copies: off in a timed run).  jobs given as ``FrontierJobs(jobs, witness=[], pgd_steps=N, pgd_step=s)`` run with
    ``branch_and_bound_frontier``'s options of those names: ``witness`` receives one entry per job, in job order,
    and a job's witness and bounds are what it gets alone with the same options.

    Returns a list, in job order, of (global_lb, global_ub, rounds, domains_bounded, reason)."""
    options, tighten_root = _options_of(jobs), _tighten_of(jobs)
    _check_tighten(tighten_root)                                 # (before the run touches a device, as every option)
    jobs, S, cap, in_shape = _check_jobs_args(jobs, K, segments, capacity, n_iter, lr, eps, max_rounds)
    run = JobsRun(choice, fixed_layers, jobs, in_shape, K, S, cap, n_iter, lr, eps, **options)
    return _verify_jobs(run, choice, jobs, max_rounds, log, trace, tighten_root=tighten_root)


def verify_properties_threshold(choice, fixed_layers, jobs, branching_threshold, K=16, segments=None, capacity=None, n_iter=20, lr=0.1, eps=1e-4,
                                max_rounds=50, kwbd_threshold=KWBD_DEFAULT, sparsest_layer=0, decision_threshold=0.001, log=print, trace=None, stats=None):
    """``verify_properties`` with the BaBSR fall-back below ``branching_threshold`` for every job: every job gets
    the result ``branch_and_bound_frontier(..., capacity=capacity, branching_threshold=branching_threshold, kwbd_threshold=...,
    sparsest_layer=..., decision_threshold=...)`` gives it alone, bit for bit, whatever else is in flight, whichever segment it got and
    whenever it was admitted.

    Every job has its own intercept counter and its own table of inefficient KW points, both zero when it is admitted, read and updated
    in the job's parent row order within a round and carried from round to round.  A round bounds the second pairs of the selected
    parents of ALL jobs in one chain of launches, and reads one more array than ``verify_properties``' round: m per plan entry and their
    sum.  stats: None, or a list that receives per job, in job order, the dict ``branch_and_bound_frontier`` fills ("branches",
    "kw_bounded", "kw_used", "domains_bounded").  trace: ``verify_properties``' keys per round and per entry plus the keys of the one-job
    threshold trace ("gnn_decisions", "gnn_improvement", "kw_decisions", "kw_improvement", "selected" -- rows counted from the entry's
    first --, "used_kw", both pairs' bounds and infeasible flags; "decisions" are the final ones).  A ``FrontierJobs`` carries
    the witness and descent options, as for ``verify_properties``.

    Returns a list, in job order, of (global_lb, global_ub, rounds, domains_bounded, reason)."""
    options, tighten_root = _options_of(jobs), _tighten_of(jobs)
    _check_tighten(tighten_root)                                 # (before the run touches a device, as every option)
    jobs, S, cap, in_shape = _check_jobs_args(jobs, K, segments, capacity, n_iter, lr, eps, max_rounds)
    if branching_threshold is None:
        raise ValueError("branching_threshold = None: a number with 0 < branching_threshold <= 1 (verify_properties runs without the fall-back)")
    run = JobsRun(choice, fixed_layers, jobs, in_shape, K, S, cap, n_iter, lr, eps, branching_threshold=branching_threshold, kwbd_threshold=kwbd_threshold,
                  sparsest_layer=sparsest_layer, decision_threshold=decision_threshold, **options)
    return _verify_jobs(run, choice, jobs, max_rounds, log, trace, stats, tighten_root=tighten_root)


def verify_properties_babsr(choice, fixed_layers, jobs, K=16, segments=None, capacity=None, n_iter=20, lr=0.1, eps=1e-4, max_rounds=50, sparsest_layer=0,
                            decision_threshold=0.001, log=print, trace=None, stats=None):
    """``verify_properties`` with every job branching on the BaBSR heuristic alone: every job gets the result
    ``branch_and_bound_frontier(..., branching="babsr", capacity=capacity, sparsest_layer=..., decision_threshold=...)`` gives it alone, bit
    for bit, whatever else is in flight, whichever segment it got and whenever it was admitted.

    Every job has its own intercept counter, zero when it is admitted, read and updated in the job's parent row order within a round and
    carried from round to round.  ``choice`` supplies the engine; its GNN is never run.  stats: None, or a list that receives per job, in
    job order, a dict of "branches" (parents expanded) and "domains_bounded".  trace: ``verify_properties``' keys per round and per entry;
    "decisions" are BaBSR's.  A ``FrontierJobs`` carries the witness and descent options, as for ``verify_properties``.

    Returns a list, in job order, of (global_lb, global_ub, rounds, domains_bounded, reason)."""
    options, tighten_root = _options_of(jobs), _tighten_of(jobs)
    _check_tighten(tighten_root)                                 # (before the run touches a device, as every option)
    jobs, S, cap, in_shape = _check_jobs_args(jobs, K, segments, capacity, n_iter, lr, eps, max_rounds)
    run = JobsRun(choice, fixed_layers, jobs, in_shape, K, S, cap, n_iter, lr, eps, sparsest_layer=sparsest_layer, decision_threshold=decision_threshold,
                  branching="babsr", **options)
    return _verify_jobs(run, choice, jobs, max_rounds, log, trace, stats, tighten_root=tighten_root)


def verify_properties_strong(choice, fixed_layers, jobs, K=16, segments=None, capacity=None, n_iter=20, lr=0.1, eps=1e-4, max_rounds=50, log=print,
                             trace=None, stats=None, learned=None, imitate=None, imitate_margin=IMITATE_MARGIN_DEFAULT, strong_candidates=None,
                             strong_chunk=STRONG_CHUNK_DEFAULT, strong_audit=None, branching="strong"):
    """``verify_properties`` with strong branching, its audit and the imitation step for every job.  WITHOUT
    ``imitate`` every job gets the result ``branch_and_bound_frontier(..., branching=branching, capacity=capacity, strong_candidates=...,
    strong_chunk=...)`` gives it alone, bit for bit, whatever else is in flight, whichever segment it got, whenever it was admitted and
    wherever the chunks fall.

    branching: "strong" -- every parent of every job is split where its bound improves most over its candidates -- or "gnn", legal only
    with ``strong_audit`` or ``imitate`` (``verify_properties`` runs the jobs on the GNN without a table; ``verify_properties_babsr`` on
    BaBSR).  strong_candidates (a ``Shortlist`` included: the jobs of a pool share the scorer that shortlists, as they share it for
    ``imitate``), strong_chunk, strong_audit, imitate, imitate_margin: ``branch_and_bound_frontier``'s.  The candidates of
    all parent rows of a round, of all jobs, form ONE dense list that is bounded in chunks of ``strong_chunk``; a chunk may span parents
    and jobs, and ``gnnb_strong_rows_jobs`` gives every candidate's child rows their own job's box and property row first.  The round's
    one extra read is cand0 at every entry's first row and the total (``StrongJobsRun.read_candidates``, 4 (entries + 1) bytes).

    imitate = N: the LEARNING rounds are the run's launched rounds (root phases do not count) whose 1-based number is a multiple of N.
    Every parent row of every entry then gets the table, and behind the commit and the read of the records, when the round listed a
    candidate, ONE ``gnnb_imitation_step_rows`` runs over all the round's rows in plan row order; the next round of every job scores with
    the new parameters.  The jobs of a pool share ONE scorer: with ``imitate`` a job's result depends on what else is in flight (which
    rows shared its steps, and when it was admitted); without ``imitate`` it does not.  ``choice`` must then be a
    ``graphnet.graph_score_online.GraphChoice``, and when the run ends (or raises) after a step ``choice.model`` receives the device's
    parameters.  A step that finds no device memory raises a RuntimeError that says to lower ``segments`` or ``K``.

    stats: None, or a list that receives per job, in job order, {"branches", "domains_bounded", "strong_bounded"} (the job's candidate
    children).  learned: None, or a dict that receives "imitation_steps", "imitation_rows" and "rounds" (launched) of the run.  trace:
    ``verify_properties``' keys per round and per entry; in "strong" mode also "strong_candidates" and "strong_improvement" per parent, on a
    learning round "imitation_loss" / "imitation_report" / "imitation_regret" of the entry's rows, and in a run with ``imitate`` the
    entry's "global_lb" / "global_ub" after the round.  strong_audit receives per parent the one-job audit's dict plus "job", "segment"
    and "round".  A ``FrontierJobs`` carries the witness and descent options, as for ``verify_properties``.

    Returns a list, in job order, of (global_lb, global_ub, rounds, domains_bounded, reason)."""
    options, tighten_root = _options_of(jobs), _tighten_of(jobs)
    _check_tighten(tighten_root)                                 # (before the run touches a device, as every option)
    jobs, S, cap, in_shape = _check_jobs_args(jobs, K, segments, capacity, n_iter, lr, eps, max_rounds)
    if learned is not None and not isinstance(learned, dict):
        raise ValueError(f"learned = {learned!r}: None, or a dict that receives the run's learning counts")
    run = StrongJobsRun(choice, fixed_layers, jobs, in_shape, K, S, cap, n_iter, lr, eps, imitate=imitate, imitate_margin=imitate_margin,
                        strong_candidates=strong_candidates, strong_chunk=strong_chunk, strong_audit=strong_audit, branching=branching, **options)
    return _verify_jobs(run, choice, jobs, max_rounds, log, trace, stats, learned, tighten_root)


def verify_properties_online(choice, fixed_layers, jobs, branching_threshold, online_threshold, K=16, segments=None, capacity=None, n_iter=20, lr=0.1,
                             eps=1e-4, max_rounds=50, sparsest_layer=0, decision_threshold=0.001, repack="host", log=print, trace=None, stats=None,
                             learned=None):
    """``verify_properties_threshold`` with the reference's online learning for every job: the many-jobs form of
    ``branch_and_bound_frontier(..., branching_threshold=T, online_threshold=N)``.  A round is the threshold round with
    ``kwbd_threshold = 2**31 - 1`` (the online loop has no table of inefficient KW points, so the function takes no ``kwbd_threshold``:
    every parent with a KW decision gets its second pair bounded) plus section 7.7's learning per job.

    Every job has its own table of wrong GNN points (the reference builds one ``GraphChoice``, and with it one ``wrong_pts_dc``, per
    property), zero when it is admitted, read and updated in the job's parent row order within a round and carried from round to round:
    a parent that took its KW pair counts its GNN decision, and from the ``online_threshold``-th count of a node on it is a learn row
    (``gnnb_frontier_learn_jobs``).  The learn rows of all jobs form ONE dense list in plan-entry order.  Commit first, then learn: a round
    with M > 0 selected parents reads one more array behind the records -- the learn rows per plan entry and their sum N, 4 (entries + 1)
    bytes -- and with N > 0 ONE ``gnnb_online_step_rows`` takes an Adam step on the summed loss of the learn rows of all jobs, all scored
    with the round's opening parameters; the next round of every job scores with the new ones.  A round with M = 0 launches and reads
    nothing new.

    The jobs of a pool share ONE scorer: from the run's first step on a job's result depends on what else is in flight (which rows shared
    its steps, and when it was admitted); before that step, and in a run that never learns, it does not, and every job gets the result
    ``branch_and_bound_frontier(..., branching_threshold=T, online_threshold=N)`` gives it alone.  ``choice`` must be a
    ``graphnet.graph_score_online.GraphChoice``; when the run ends (or raises) after a step ``choice.model`` receives the device's
    parameters.  repack: ``branch_and_bound_frontier``'s (section 7.15): with "device" the step is only issued, and its status and traced
    losses are read with the next round's records.  A step that finds no device memory raises a RuntimeError that says to lower
    ``segments`` or ``K``.

    stats: None, or a list that receives per job, in job order, the threshold mode's dict plus "online_rows", the learn rows that were
    the job's.  learned: None, or a dict that receives "online_steps", "online_rows" and "rounds" (launched) of the run.  trace:
    ``verify_properties_threshold``'s keys per round and per entry plus the entry's slice of the lists -- "learn_rows" (counted from the
    entry's first row, as "selected"), "learn_kw", "learn_improve", "loss" -- and the entry's "global_lb" / "global_ub" after the round.
    A ``FrontierJobs`` carries the witness and descent options, as for ``verify_properties``.

    Returns a list, in job order, of (global_lb, global_ub, rounds, domains_bounded, reason)."""
    options, tighten_root = _options_of(jobs), _tighten_of(jobs)
    _check_tighten(tighten_root)                                 # (before the run touches a device, as every option)
    jobs, S, cap, in_shape = _check_jobs_args(jobs, K, segments, capacity, n_iter, lr, eps, max_rounds)
    if branching_threshold is None:
        raise ValueError("branching_threshold = None: a number with 0 < branching_threshold <= 1 (verify_properties runs without the fall-back)")
    _check_threshold(branching_threshold, KWBD_DEFAULT)
    if online_threshold is None:
        raise ValueError("online_threshold = None: an integer >= 1 (verify_properties_threshold runs without online learning)")
    _check_online(online_threshold, branching_threshold, KWBD_DEFAULT, choice)
    _check_repack(repack)
    if learned is not None and not isinstance(learned, dict):
        raise ValueError(f"learned = {learned!r}: None, or a dict that receives the run's learning counts")
    run = OnlineJobsRun(choice, fixed_layers, jobs, in_shape, K, S, cap, n_iter, lr, eps, branching_threshold=branching_threshold,
                        sparsest_layer=sparsest_layer, decision_threshold=decision_threshold, online_threshold=online_threshold, repack=repack, **options)
    return _verify_jobs(run, choice, jobs, max_rounds, log, trace, stats, learned, tighten_root)


def _verify_jobs(run, choice, jobs, max_rounds, log, trace, stats=None, learned=None, tighten_root=0):
    """``_jobs_loop`` on a checked run, for ``verify_properties``, ``verify_properties_threshold``, ``verify_properties_babsr``,
    ``verify_properties_strong`` and ``verify_properties_online``; when the run ends (or raises) after a learning step, ``choice.model`` receives the device's parameters.
    tighten_root: the ``FrontierJobs``' (``_tighten_of``)."""
    run.keep_pairs = trace is not None
    try:
        run.set_tighten_root(tighten_root)
        return _jobs_loop(run, jobs, max_rounds, log, trace, stats, learned)
    finally:
        if run.imitation_steps or getattr(run, "online_steps", 0):             # the nn.Module mirrors the device, as branch_and_bound_frontier leaves it
            choice.model.load_blob(run.eng.get_weights())
        run.close()


def _jobs_loop(run, jobs, max_rounds, log, trace, stats, learned):
    """``_verify_jobs``' loop on its run, which knows the rest: K, the segments and their capacity, eps, and what is on -- ``threshold``
    (a round has a second half, and stats are the threshold mode's), ``branching`` and ``strong_on`` (theirs), ``witness_on``.  stats:
    None, or the list that receives per job the mode's part of its tally (in an online run, section 7.19, the threshold mode's plus
    "online_rows", the job's learn rows summed from ``learn_e``); learned: None, or the dict that receives the run's "imitation_steps",
    "imitation_rows" and launched "rounds" (an online run's: "online_steps", "online_rows", "rounds")."""
    F, K, S, cap, thr = _lib, run.K, run.S, run.cap, run.threshold is not None
    results, tally = [None] * len(jobs), [None] * len(jobs)
    online, online_rows = getattr(run, "online", None) is not None, [0] * len(jobs)      # (section 7.19: the learn rows that were each job's)
    seg_job, rec, capacity_stop = [None] * S, [None] * S, [False] * S
    waiting = list(range(len(jobs)))

    def reason_of(s):
        j = seg_job[s]
        if rec[s][F.FS_INFEASIBLE] > 0 and tally[j]["rounds"] == 0:
            return "infeasible_root"
        return "capacity" if capacity_stop[s] else _stop_reason(rec[s], run.eps, jobs[j].decision_bound, tally[j]["rounds"], max_rounds)

    while True:
        for s in range(S):                                        # 1. the finished jobs leave
            j = seg_job[s]
            reason = None if j is None else reason_of(s)
            if reason is not None:
                inf, rounds = float("inf"), tally[j]["rounds"]
                results[j] = ((inf, inf, 0, 1, reason) if reason == "infeasible_root" else
                              (_global_lb(rec[s]), rec[s][F.FS_GLOBAL_UB], rounds, tally[j]["domains_bounded"], reason))
                log(f"job {j} segment {s}: {reason} after {rounds} rounds, lb {results[j][0]:.5f} ub {results[j][1]:.5f}")
                if thr:
                    run.keep_used(s, j)
                if run.witness_on:
                    run.keep_witness(s, j)
                run.release(s)
                seg_job[s], rec[s], capacity_stop[s] = None, None, False
        admitted = []
        for s in range(S):                                        # 2. waiting jobs take the free segments, lowest first
            if seg_job[s] is None and waiting:
                seg_job[s] = waiting.pop(0)
                run.admit(s, seg_job[s])
                admitted.append(s)
        if admitted:                                              # 3. the root phase
            run.launch_roots(admitted)
            st = run.read_state()
            for s in admitted:
                rec[s], tally[seg_job[s]] = st[s], _new_tally()
                if not rec[s][F.FS_INFEASIBLE] > 0:
                    _check_record(rec[s])
                log(f"job {seg_job[s]} segment {s}: root lb {_global_lb(rec[s]):.5f} ub {rec[s][F.FS_GLOBAL_UB]:.5f}")
        if all(j is None for j in seg_job):
            break
        entries, compact, stopped = plan_round([None if seg_job[s] is None or reason_of(s) is not None else rec[s] for s in range(S)], K, cap)
        for s in stopped:
            capacity_stop[s] = True
        if not entries:
            continue
        if any(compact):
            run.compact(compact)
        run.launch_round(entries)
        traced = [_report_launched(run, trace, e, row0, k, {"job": seg_job[s], "segment": s, "round": tally[seg_job[s]]["rounds"]})
                  for e, (s, row0, k) in enumerate(entries)]
        st = run.read_state()
        if trace is not None:
            values = _witness_values(run)
            for e, ((s, row0, k), t) in enumerate(zip(entries, traced)):
                if online:
                    _online_entry_trace(run, t, e, row0, st[s])
                _report_read(run, t, s, row0, k, st[s], values)
        for e, (s, _, k) in enumerate(entries):
            j = seg_job[s]
            rec[s] = st[s]
            if online:
                online_rows[j] += run.learn_e[e]
            _check_record(rec[s])
            _tally_entry(run, tally[j], e, k, rec[s])
            log(f"job {j} round {tally[j]['rounds']} picked {k} kept {int(rec[s][F.FS_KEPT])} closed {int(rec[s][F.FS_CLOSED])} "
                f"infeasible {int(rec[s][F.FS_INFEASIBLE])} open {int(rec[s][F.FS_N_OPEN])} lb {_global_lb(rec[s]):.5f} ub {rec[s][F.FS_GLOBAL_UB]:.5f}")
    run.check_status()
    if run.witness_on:                                            # N_0 floats per job, read once
        points = run.job_point.cpu()
        run.witness_to.extend(None if math.isinf(results[j][1]) else points[j].reshape(run.in_shape) for j in range(len(jobs)))
    if stats is not None and thr:
        used = run.job_used.cpu().tolist()
        stats.extend({**{key: t[key] for key in ("branches", "kw_bounded", "domains_bounded")}, "kw_used": int(used[j]),
                      **({"online_rows": online_rows[j]} if online else {})} for j, t in enumerate(tally))
    elif stats is not None:                                       # BaBSR: the first two; a run with a table: all three
        keys = ("branches", "domains_bounded", "strong_bounded")[:3 if run.strong_on else 2]
        stats.extend({key: t[key] for key in keys} for t in tally)
    if learned is not None and online:
        learned.update(online_steps=run.online_steps, online_rows=run.online_rows, rounds=run.round)
    elif learned is not None:
        learned.update(imitation_steps=run.imitation_steps, imitation_rows=run.imitation_rows, rounds=run.round)
        if run.replay is not None:
            learned.update(replay_stored=run.replay_stored, replay_skipped=run.replay_skipped, replay_filled=run.replay_filled)
    return results
