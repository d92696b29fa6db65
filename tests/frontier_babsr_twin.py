"""Host twins for tests/test_gpu_frontier_babsr.py:

* ``crafted_rows`` / ``rule_reference``: (K, R) matrices that take every branch of the BaBSR decision rule, and the rule restated with
  ``plnn.kw_score_conv.decide`` row by row with one carried counter;
* ``babsr_twin``: the plain mode of ``tests.frontier_twin.twin`` with ``BatchedGraphChoice.kw_decision_many`` in row order and one carried
  intercept counter in the GNN decision's place -- relu_bab's loop made of public pieces."""
import numpy as np
import torch

from gnn_branching_amd import bab_caller, lp_producer
from gnn_branching_amd.plnn.kw_score_conv import decide
from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, at_least_the_parents, toy, ub64

SPARSEST = 0
DTHR = 2.0 ** -10                   # a threshold fp32 holds exactly: a score AT it is a case of its own
# The kinds of row, in an order that carries the counter through 0, 1, 2 and its resets, with the device-defined rows (NaN, nothing
# undecided), which must leave it alone, while it is not zero.
SEQ = ["score", "sparsest_max", "at_threshold", "below_threshold", "tie_layer", "tie_across_hi", "tie_across_lo", "tie_across_same",
       "icp0", "icp0", "icp0", "icp0", "icp_late", "popped", "icp0", "nan", "no_open", "nan_icp", "icp0", "icp0"]


def crafted_rows(relu, seed=5):
    """One row per kind of SEQ on ReLU layers of the sizes ``relu`` (at least three, layer 1 wider than 600).  Returns a dict of CPU
    tensors scores / icps / amb (K, R) and "kinds"."""
    g = torch.Generator().manual_seed(seed)
    K, L, R = len(SEQ), len(relu), sum(relu)
    assert L >= 3 and relu[1] > 600
    off = [0] + list(np.cumsum(relu))
    hi, lo = L - 1, L - 2
    scores = torch.rand(K, R, generator=g) * 5e-4          # all below DTHR
    icps = -torch.rand(K, R, generator=g) * 5e-5           # all above -1e-4
    amb = (torch.rand(K, R, generator=g) < 0.5).float()
    amb[:, [o for o in off[:-1]]] = 0.0                    # the first undecided node of a layer is not node 0 ...
    amb[:, [o + 2 for o in off[:-1]]] = 1.0                # ... but node 1 or 2
    for i, kind in enumerate(SEQ):
        if kind == "score":
            scores[i, off[hi] + 11] = 0.5
        elif kind == "sparsest_max":                       # the maximum lies in the sparsest layer: not taken, whatever its value
            scores[i, off[SPARSEST] + 2] = 0.7
        elif kind == "at_threshold":                       # equal to the threshold is not above it
            scores[i, off[hi] + 9] = DTHR
        elif kind == "below_threshold":
            scores[i, off[hi] + 9] = DTHR * 0.75
        elif kind == "tie_layer":                          # equal maxima in one layer: neighbours, and one thread stride apart; the first wins
            for j in (270, 14, 15, 526):
                scores[i, off[1] + j] = 0.25
        elif kind == "tie_across_hi":                      # equal maxima in two layers: the larger tuple (value, index) wins
            scores[i, off[lo] + 3], scores[i, off[hi] + 6] = 0.125, 0.125
        elif kind == "tie_across_lo":
            scores[i, off[lo] + 6], scores[i, off[hi] + 3] = 0.125, 0.125
        elif kind == "tie_across_same":                    # equal tuples: the first layer
            scores[i, off[lo] + 5], scores[i, off[hi] + 5] = 0.125, 0.125
        elif kind == "icp0":
            icps[i, off[0] + 5] = -0.5
            icps[i, off[0] + 9] = -0.5                     # (an equal minimum later in the layer: the first one counts)
            icps[i, off[0] + 261] = -0.5                   # (and one a thread stride behind the first)
        elif kind == "icp_late":                           # the LAST layer with an intercept; not layer 0: the counter goes back to 0
            icps[i, off[0] + 5] = -0.5
            icps[i, off[1] + 4] = -0.25
        elif kind == "popped":                             # the layer the order prefers has no undecided node
            amb[i, off[hi]:off[hi + 1]] = 0.0
        elif kind == "nan":
            scores[i, off[hi] + 1] = float("nan")
            icps[i, off[0] + 5] = -0.5
        elif kind == "nan_icp":
            icps[i, off[1] + 700] = float("nan")
            scores[i, off[hi] + 11] = 0.5
        elif kind == "no_open":
            amb[i] = 0.0
            scores[i, off[hi] + 11] = 0.5
    return {"scores": scores, "icps": icps, "amb": amb, "kinds": list(SEQ)}


def rule_reference(relu, rows, idx, icp, sparsest=SPARSEST, dthr=DTHR, order=None):
    """``decide`` for the rows ``idx`` in order, the counter carried.  A row with a NaN, a row without an undecided node and a row whose
    order runs out (the host rule raises on them) get [-1, -1] and leave the counter alone.  order: the layers popped from the end (None:
    ``lp_producer._random_order``).  Returns (decisions, the counter after, the counter before every row)."""
    order = lp_producer._random_order(len(relu), sparsest) if order is None else list(order)
    decs, before = [], []
    for i in idx:
        before.append(icp)
        decs.append([-1, -1])
        if bool(torch.isnan(rows["scores"][i]).any()) or bool(torch.isnan(rows["icps"][i]).any()) or not bool((rows["amb"][i] != 0).any()):
            continue
        s, t, m = (list(torch.split(rows[k][i], relu)) for k in ("scores", "icps", "amb"))
        try:
            d, icp = decide(s, t, m, icp, order, sparsest, dthr)
        except IndexError:
            continue
        decs[-1] = [int(d[0]), int(d[1])]
    return decs, icp, before


def babsr_twin(K, rounds, prop=None, eps=None, sparsest=0, dthr=0.001):
    """relu_bab's loop on toy_kw as a host loop of public pieces: per round the K open domains of lowest bound, each split at
    ``kw_decision_many``'s decision (row order, ONE counter carried through the rows and the rounds, starting at 0), the children bounded by
    solve_many(lp="dual_device"), then the keep-or-close rule.  Returns per-round "decisions", "child_bounds" and "parent_bounds", "branches", "global_lb",
    "global_ub" and the counter "icp".

    Asserts ITS OWN conditions: no two open bounds equal at a pick; no keep-or-close comparison within 1e-9 of its threshold."""
    lp, choice, root_mask = toy(False, prop, eps)
    fixed = {"fixed_layers": lp.layers[:-1], "prop_layers": [lp.layers[-1]]}
    n_layers, order = len(lp.layers), lp_producer._random_order(len(lp.pre_relu_indices), sparsest)

    def as_sub(d):
        return bab_caller.Subproblem(*d.graph_bounds(lp.pre_relu_indices, n_layers), d.dual_vars, d.ub_point, d.primals, d.mask)

    def children_of(pairs):
        items = []
        for d, dec in pairs:
            for c in (0, 1):
                m = [t.clone() for t in d.mask]
                m[dec[0]][dec[1]] = c
                items.append((m, d, dec[0]))
        return lp.solve_many(items, lp="dual_device", n_iter=N_ITER, lr=LR)

    root = lp.solve_many([(root_mask, None, None)], lp="dual_device", n_iter=N_ITER, lr=LR)[0]
    gub, closed, domains = ub64(lp, root), INF, []

    def keep_or_close(subs, gub, closed):
        for c in subs:
            if c is None:
                continue
            assert abs(c.lb - (gub - EPS_BAB)) > 1e-9, ("the twin's comparison is within 1e-9 of its threshold", c.lb, gub - EPS_BAB)
            if any(bool((m == -1).any()) for m in c.mask) and c.lb < gub - EPS_BAB:
                domains.append(c)
            else:
                closed = min(closed, c.lb)
        return closed

    def global_lb():
        return min([d.lb for d in domains] + [closed, gub])
    closed = keep_or_close([root], gub, closed)
    out = {"decisions": [], "child_bounds": [], "parent_bounds": []}
    icp = branches = 0
    for _ in range(rounds):
        if not domains or not gub - global_lb() > EPS_BAB:
            break
        domains.sort(key=lambda d: d.lb)
        assert len({d.lb for d in domains}) == len(domains), "two open bounds are equal at a pick"
        picked, domains[:] = domains[:K], domains[K:]
        decs = []
        for d in picked:                                   # row order: the counter is carried from parent to parent
            (kw,), (icp,) = bab_caller.BatchedGraphChoice.kw_decision_many(choice, [as_sub(d)], fixed, [icp], order, sparsest, dthr)
            decs.append([int(kw[0]), int(kw[1])])
        children = at_least_the_parents(children_of(zip(picked, decs)), [d for d in picked for _ in (0, 1)])
        gub = min([gub] + [ub64(lp, c) for c in children if c is not None])
        closed = keep_or_close(children, gub, closed)
        branches += len(picked)
        out["decisions"].append(decs)
        out["parent_bounds"].append([d.lb for d in picked])
        out["child_bounds"].append([INF if c is None else c.lb for c in children])
    out.update(branches=branches, global_lb=global_lb(), global_ub=gub, icp=icp)
    return out
