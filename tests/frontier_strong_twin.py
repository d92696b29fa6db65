"""Host twins for tests/test_gpu_frontier_strong.py:

* ``list_reference`` / ``pick_reference``: the rule of gnnb_strong_list and gnnb_strong_pick restated on CPU tensors with Python floats
  (fp64) in the same operation order -- a sort on (score descending, flat index ascending), ``bab_caller.gnn_improvement``, a first
  maximum;
* ``strong_twin``: the plain mode of ``tests.frontier_twin.twin`` with the decision of each picked domain taken from candidates bounded
  through ``lp.solve_many(lp="dual_device")`` and ``gnn_improvement`` -- strong branching made of public pieces."""
import math

import numpy as np
import torch

from gnn_branching_amd import bab_caller
from gnn_branching_amd.bab_caller import gnn_improvement
from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, at_least_the_parents, toy, ub64

NAN = float("nan")


def offsets(relu):
    return [0] + [int(v) for v in np.cumsum(relu)]


def node_of(relu, r):
    """[layer, idx] of the flat ReLU index r."""
    off = offsets(relu)
    k = max(l for l in range(len(relu)) if off[l] <= r)
    return [k, r - off[k]]


def candidates_of(amb_row, score_row, top_m):
    """The candidates of one row (flat indices, ascending): every node with a non-zero mask entry, or the ``top_m`` first of them on
    (score descending, index ascending), scores compared as values (-0.0 == 0.0); none if an undecided node's score is NaN."""
    open_ = [r for r, m in enumerate(amb_row.tolist()) if m != 0.0]
    if top_m == 0:
        return open_
    sc = score_row.tolist()
    if any(math.isnan(sc[r]) for r in open_):
        return []
    return sorted(sorted(open_, key=lambda r: (-(sc[r] + 0.0), r))[:top_m])      # (+ 0.0: -0.0 becomes 0.0; the tuple compares values anyway)


def list_reference(relu, amb, scores, top_m, slots, capacity):
    """gnnb_strong_list on CPU tensors amb / scores (K, R) and the list ``slots``.  Returns (cand0, cand_row, cand_slot, cand_dec) as
    Python lists."""
    cand0, rows, cslots, decs = [0], [], [], []
    for i, s in enumerate(slots):
        cands = candidates_of(amb[i], None if scores is None else scores[i], top_m) if 0 <= s < capacity else []
        for r in cands:
            rows.append(i)
            cslots.append(s)
            decs.append(node_of(relu, r))
        cand0.append(cand0[-1] + len(cands))
    return cand0, rows, cslots, decs


def improvement_of(live0, live1, inf0, inf1, lb0, lb1, b):
    """imp of one candidate: NaN with a dead child row; 1.0 for a parent bound >= 0; else gnn_improvement, an infeasible child at +inf."""
    if not (live0 and live1):
        return NAN
    if not b < 0:
        return 1.0
    return gnn_improvement(INF if inf0 else lb0, INF if inf1 else lb1, b)


def pick_reference(relu, cand0, cand_dec, live, infeasible, bound, parent_bounds):
    """gnnb_strong_pick on Python lists; parent_bounds[i]: the pool bound of row i's slot.  Returns (decisions, best_improvement,
    improvement, table) with the table a (K, R) list of lists, NaN where no candidate stands."""
    off, R, K = offsets(relu), sum(relu), len(cand0) - 1
    decisions, best, imp, table = [], [], [], [[NAN] * R for _ in range(K)]
    for i in range(K):
        bq, bv = -1, 0.0
        for q in range(cand0[i], cand0[i + 1]):
            v = improvement_of(live[2 * q], live[2 * q + 1], infeasible[2 * q], infeasible[2 * q + 1], bound[2 * q], bound[2 * q + 1], parent_bounds[i])
            imp.append(v)
            table[i][off[cand_dec[q][0]] + cand_dec[q][1]] = v
            if not math.isnan(v) and (bq < 0 or v > bv):      # a strict comparison: the first of equal values; NaN below every number
                bq, bv = q, v
        decisions.append(list(cand_dec[bq]) if bq >= 0 else [-1, -1])
        best.append(bv if bq >= 0 else NAN)
    return decisions, best, imp, table


def same(a, b):
    """Equality of two nested lists, tuples and dicts of floats that counts NaN == NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(v, b[k]) for k, v in a.items())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


# ---- the host loop ------------------------------------------------------------------------------------------------------------------------
def host_pieces(prop=None, eps=None):
    """(lp, choice, root_mask, as_sub, children_of, babsr_scores) on toy_kw: the public pieces the twin is made of."""
    lp, choice, root_mask = toy(False, prop, eps)
    fixed = {"fixed_layers": lp.layers[:-1], "prop_layers": [lp.layers[-1]]}
    n_layers = len(lp.layers)

    def as_sub(d):
        return bab_caller.Subproblem(*d.graph_bounds(lp.pre_relu_indices, n_layers), d.dual_vars, d.ub_point, d.primals, d.mask)

    def children_of(pairs):
        items = []
        for d, dec in pairs:
            for c in (0, 1):
                m = [t.clone() for t in d.mask]
                m[dec[0]][dec[1]] = c
                items.append((m, d, dec[0]))
        return lp.solve_many(items, lp="dual_device", n_iter=N_ITER, lr=LR) if items else []

    def babsr_scores(d):
        """gnnb_babsr's scores of one domain, (R,) fp32 on the CPU (``BatchedGraphChoice.kw_decision_many``'s marshalling)."""
        sub = as_sub(d)
        ng = len(sub.lower_bounds_all)
        lbs = [torch.as_tensor(sub.lower_bounds_all[k]).float().reshape((1,) + tuple(sub.lower_bounds_all[k].shape[1:])) for k in range(ng)]
        ubs = [torch.as_tensor(sub.upper_bounds_all[k]).float().reshape((1,) + tuple(sub.upper_bounds_all[k].shape[1:])) for k in range(ng)]
        masks = torch.cat([(m == -1).float().reshape(-1) for m in sub.mask])[None]
        with torch.no_grad():
            return choice.model.engine().babsr(lbs, ubs, fixed, masks).scores[0].cpu()
    return lp, choice, root_mask, as_sub, children_of, babsr_scores


def strong_decision(d, relu, children_of, babsr_scores, top_m):
    """The strong-branching table of one domain: (decision, best improvement, candidates as flat indices, their improvements, their
    children's bounds with an infeasible child at +inf)."""
    amb = torch.cat([(m == -1).float().reshape(-1) for m in d.mask])
    cands = candidates_of(amb, babsr_scores(d) if top_m else None, top_m)
    decs = [node_of(relu, r) for r in cands]
    children = children_of([(d, dec) for dec in decs])
    lbs = [INF if c is None else c.lb for c in children]
    imps = [improvement_of(1, 1, 0, 0, lbs[2 * q], lbs[2 * q + 1], d.lb) for q in range(len(cands))]
    bq = -1
    for q, v in enumerate(imps):
        if not math.isnan(v) and (bq < 0 or v > imps[bq]):
            bq = q
    return (decs[bq] if bq >= 0 else [-1, -1]), (imps[bq] if bq >= 0 else NAN), cands, imps, lbs


def strong_twin(K, rounds, top_m=0, prop=None, eps=None, commit=None):
    """Strong branching on toy_kw as a host loop of public pieces: per round the K open domains of lowest bound, each split at
    ``strong_decision``'s node, the winners' children bounded by solve_many(lp="dual_device"), then the keep-or-close rule.  Returns
    per-round "decisions", "child_bounds", "parent_bounds", "candidates", "improvements", "best", "strong_decisions"; "branches",
    "global_lb", "global_ub".  commit: None, or per round the decisions to split at in the winners' place (an audited run of another
    branching mode: the tables are those of the domains that run picks).

    Asserts ITS OWN conditions: no two open bounds equal at a pick; no keep-or-close comparison within 1e-9 of its threshold; every
    picked domain has a decision."""
    lp, choice, root_mask, as_sub, children_of, babsr_scores = host_pieces(prop, eps)
    relu = [int(m.numel()) for m in root_mask]
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
    keys = ("decisions", "child_bounds", "parent_bounds", "candidates", "improvements", "best", "strong_decisions")
    out = {k: [] for k in keys}
    branches = 0
    for _ in range(rounds):
        if not domains or not gub - global_lb() > EPS_BAB:
            break
        domains.sort(key=lambda d: d.lb)
        assert len({d.lb for d in domains}) == len(domains), "two open bounds are equal at a pick"
        picked, domains[:] = domains[:K], domains[K:]
        tables = [strong_decision(d, relu, children_of, babsr_scores, top_m) for d in picked]
        decs = [t[0] for t in tables] if commit is None else [list(d) for d in commit[len(out["decisions"])]]
        assert all(d != [-1, -1] for d in decs), "a picked domain of the twin has no decision"
        children = at_least_the_parents(children_of(zip(picked, decs)), [d for d in picked for _ in (0, 1)])
        gub = min([gub] + [ub64(lp, c) for c in children if c is not None])
        closed = keep_or_close(children, gub, closed)
        branches += len(picked)
        row = {"decisions": decs, "child_bounds": [INF if c is None else c.lb for c in children], "parent_bounds": [d.lb for d in picked],
               "candidates": [t[2] for t in tables], "improvements": [t[3] for t in tables], "best": [t[1] for t in tables],
               "strong_decisions": [t[0] for t in tables]}
        for k in keys:
            out[k].append(row[k])
    out.update(branches=branches, global_lb=global_lb(), global_ub=gub)
    return out
