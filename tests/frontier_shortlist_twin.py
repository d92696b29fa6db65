"""Host twins for tests/test_gpu_shortlist.py and tests/test_frontier_shortlist_cpu.py:

* ``union_of`` / ``union_reference``: the rule of gnnb_strong_list_union in Python -- two sorts (``frontier_strong_twin.candidates_of``,
  the rule of gnnb_strong_list) and a set union;
* ``shortlist_twin``: ``frontier_strong_twin.strong_twin``'s host loop with the candidates of each picked domain taken from BaBSR's
  scores, from the GNN's (``BatchedGraphChoice.decision_many``'s forward, with its scores) or from both."""
import math

import torch

from gnn_branching_amd import bab_caller
from tests.frontier_strong_twin import NAN, candidates_of, host_pieces, improvement_of, node_of
from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, at_least_the_parents, ub64


def union_of(amb_row, score_a, top_a, score_b, top_b):
    """The candidates of one row (flat indices, ascending) and their sources (1: in A's set only, 2: in B's only, 3: in both).  A NaN at
    an undecided node of either array empties the row (then ``candidates_of`` gives no candidate for that array, as it does for a row
    without an undecided node)."""
    a, b = candidates_of(amb_row, score_a, top_a), candidates_of(amb_row, score_b, top_b)
    if not a or not b:
        return [], []
    cands = sorted(set(a) | set(b))
    return cands, [(r in a) + 2 * (r in b) for r in cands]


def union_reference(relu, amb, scores_a, top_a, scores_b, top_b, slots, capacity):
    """gnnb_strong_list_union on CPU tensors amb / scores_a / scores_b (K, R) and the list ``slots``.  Returns (cand0, cand_row,
    cand_slot, cand_dec, cand_src) as Python lists."""
    cand0, rows, cslots, decs, srcs = [0], [], [], [], []
    for i, s in enumerate(slots):
        cands, src = union_of(amb[i], scores_a[i], top_a, scores_b[i], top_b) if 0 <= s < capacity else ([], [])
        for r in cands:
            rows.append(i)
            cslots.append(s)
            decs.append(node_of(relu, r))
        srcs += src
        cand0.append(cand0[-1] + len(cands))
    return cand0, rows, cslots, decs, srcs


def shortlist_of(amb_row, babsr_row, M, gnn_row, G):
    """The candidates and sources of one parent under ``Shortlist(babsr=M, gnn=G)`` (None: that list is off; one list alone is
    gnnb_strong_list on its scores, every source its own)."""
    if M and G:
        return union_of(amb_row, babsr_row, M, gnn_row, G)
    cands = candidates_of(amb_row, babsr_row if M else gnn_row, M or G)
    return cands, [1 if M else 2] * len(cands)


def shortlist_twin(K, rounds, babsr=None, gnn=None, prop=None, eps=None, commit="strong"):
    """Strong branching over a shortlist on toy_kw as a host loop of public pieces (``strong_twin``'s loop): per round the K open domains
    of lowest bound, their BaBSR scores (``gnnb_babsr``) and GNN scores (one ``forward_host`` over the picked domains, the call
    ``BatchedGraphChoice.decision_many`` makes, with its scores), the candidates of ``shortlist_of``, both children of every candidate
    bounded by solve_many(lp="dual_device"), the table's best candidate.  commit: "strong" splits at the table's decision, "gnn" at the
    GNN's own (the forward's decisions: an audited "gnn" run).  Returns per round "decisions", "gnn_decisions", "child_bounds",
    "parent_bounds", "candidates", "sources", "improvements", "best", "strong_decisions", "global_lb" (after the round); "branches",
    "global_ub".

    Asserts ITS OWN conditions: no two open bounds equal at a pick; no keep-or-close comparison within 1e-9 of its threshold; every
    picked domain has a decision."""
    lp, choice, root_mask, as_sub, children_of, babsr_scores = host_pieces(prop, eps)
    fixed = {"fixed_layers": lp.layers[:-1], "prop_layers": [lp.layers[-1]]}
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

    def table_of(d, cands):
        decs = [node_of(relu, r) for r in cands]
        lbs = [INF if c is None else c.lb for c in children_of([(d, dec) for dec in decs])]
        imps = [improvement_of(1, 1, 0, 0, lbs[2 * q], lbs[2 * q + 1], d.lb) for q in range(len(cands))]
        bq = -1
        for q, v in enumerate(imps):
            if not math.isnan(v) and (bq < 0 or v > imps[bq]):
                bq = q
        return (decs[bq] if bq >= 0 else [-1, -1]), (imps[bq] if bq >= 0 else NAN), imps
    closed = keep_or_close([root], gub, closed)
    keys = ("decisions", "gnn_decisions", "child_bounds", "parent_bounds", "candidates", "sources", "improvements", "best", "strong_decisions",
            "global_lb")
    out = {k: [] for k in keys}
    branches = 0
    for _ in range(rounds):
        if not domains or not gub - global_lb() > EPS_BAB:
            break
        domains.sort(key=lambda d: d.lb)
        assert len({d.lb for d in domains}) == len(domains), "two open bounds are equal at a pick"
        picked, domains[:] = domains[:K], domains[K:]
        gnn_decs, gnn_scores = [None] * len(picked), [None] * len(picked)
        if gnn or commit == "gnn":
            args, _ = bab_caller.collate([as_sub(d) for d in picked], fixed)
            with torch.no_grad():
                dec, sc = choice.model.engine().forward_host(*args, want_scores=True)
            gnn_decs, gnn_scores = [[int(a), int(b)] for a, b in dec.tolist()], [torch.from_numpy(row) for row in sc]
        lists = []
        for i, d in enumerate(picked):
            amb = torch.cat([(m == -1).float().reshape(-1) for m in d.mask])
            lists.append(shortlist_of(amb, babsr_scores(d) if babsr else None, babsr, gnn_scores[i], gnn))
        tables = [table_of(d, cands) for d, (cands, _) in zip(picked, lists)]
        decs = [t[0] for t in tables] if commit == "strong" else gnn_decs
        assert all(d != [-1, -1] for d in decs), "a picked domain of the twin has no decision"
        children = at_least_the_parents(children_of(zip(picked, decs)), [d for d in picked for _ in (0, 1)])
        gub = min([gub] + [ub64(lp, c) for c in children if c is not None])
        closed = keep_or_close(children, gub, closed)
        branches += len(picked)
        row = {"decisions": decs, "gnn_decisions": gnn_decs, "child_bounds": [INF if c is None else c.lb for c in children],
               "parent_bounds": [d.lb for d in picked], "candidates": [l[0] for l in lists], "sources": [l[1] for l in lists],
               "improvements": [t[2] for t in tables], "best": [t[1] for t in tables], "strong_decisions": [t[0] for t in tables],
               "global_lb": global_lb()}
        for k in keys:
            out[k].append(row[k])
    out.update(branches=branches, global_ub=gub)
    return out
