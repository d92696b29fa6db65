"""Plain Python / torch restatements of a frontier round that splits each parent on several ReLUs, for
tests/test_frontier_depth_cpu.py and tests/test_gpu_frontier_depth.py: the rows gnnb_frontier_expand_depth writes from a candidate list,
the commit rule of section 7.3 for C children per parent (gnnb_frontier_commit_depth), the node list of a parent (gnnb_strong_list's
rule on one score row) and the depth of a round (frontier.round_depth).  Nothing here calls the package."""
import numpy as np
import torch

INF = float("inf")
FS_GLOBAL_UB, FS_CLOSED_LB, FS_LOWEST_OPEN, FS_N_OPEN, FS_IN_USE, FS_KEPT, FS_CLOSED, FS_INFEASIBLE, FS_OVERFLOW = range(9)


def offsets(sizes):
    """Flat ReLU index of the first node of every ReLU layer, and R last.  sizes: graph layers 0..L+1."""
    return [0] + [int(v) for v in np.cumsum(sizes[1:-1])]


def depth_of_round(k, K, D, n_open, cap):
    """The largest d in 1..D whose k 2^d children fit the round's 2K child rows and, with the parents' k slots reused, a pool of ``cap``
    slots that holds ``n_open`` domains; 0: none does."""
    fits = [d for d in range(1, D + 1) if k * 2 ** d <= 2 * K and n_open + (2 ** d - 1) * k <= cap]
    return max(fits) if fits else 0


def top_nodes(scores, undecided, d, sizes):
    """The first d undecided nodes of one parent in the order (score descending as float values, flat index ascending), as [layer, idx]
    pairs in ascending flat index; fewer than d undecided nodes: all of them; a NaN score at an undecided node: none.  scores: (R,)
    fp32; undecided: (R,) bool."""
    off = offsets(sizes)
    nodes = [r for r in range(len(scores)) if bool(undecided[r])]
    vals = {r: float(scores[r]) for r in nodes}
    if any(v != v for v in vals.values()):
        return []
    first = sorted(sorted(nodes, key=lambda r: (-vals[r], r))[:d])          # (-0.0 and 0.0 compare equal: the index decides)
    out = []
    for r in first:
        lay = max(l for l in range(len(off) - 1) if off[l] <= r)
        out.append([lay, r - off[lay]])
    return out


def expand(pool, slots, depth, cand0, cand_dec, sizes, out):
    """gnnb_frontier_expand_depth on host tensors.  pool: dict of CPU tensors (mask, lb, ub, alpha, beta; lb / ub lists over graph layers
    1..L+1); cand0: K + 1 ints; cand_dec: list of [layer, idx]; out: dict of the child rows' CPU tensors (mask, plb, pub, alpha, beta,
    split, live), changed in place -- rows the entry point does not write keep what they hold."""
    C, L, off, cap, n = 2 ** depth, len(sizes) - 2, offsets(sizes), int(pool["mask"].shape[0]), cand0[len(slots)]
    for i, s in enumerate(slots):
        rows = range(C * i, C * i + C)
        if not 0 <= s < cap:                                      # no such parent: rows nobody reads
            for c in rows:
                out["live"][c], out["split"][c] = 0, -1
            continue
        q0, m = cand0[i], cand0[i + 1] - cand0[i]
        listed = q0 >= 0 and 1 <= m <= depth and q0 + m <= n
        nodes = [cand_dec[q] for q in range(q0, q0 + m)] if listed else []
        if any(not (0 <= lay < L and 0 <= idx < sizes[lay + 1]) for lay, idx in nodes):
            listed, nodes = False, []
        for j, c in enumerate(rows):
            live = listed and j < 2 ** m
            out["mask"][c] = pool["mask"][s]
            out["alpha"][c], out["beta"][c] = pool["alpha"][s], pool["beta"][s]
            for k in range(L + 1):
                out["plb"][k][c], out["pub"][k][c] = pool["lb"][k][s], pool["ub"][k][s]
            if live:
                for b, (lay, idx) in enumerate(nodes):
                    out["mask"][c, off[lay] + idx] = (j >> b) & 1
            out["live"][c] = 1 if live else 0
            out["split"][c] = min(lay for lay, _ in nodes) if live else L - 1


def commit(pool, state, slots, C, ch, eps, decision_bound, sizes):
    """The commit rule of DESIGN.md section 7.3 for C children per parent (gnnb_frontier_commit_depth; C = 2: gnnb_frontier_commit) on
    host tensors.  pool: dict of CPU tensors (mask, lb, ub, alpha, beta, bound, open), changed in place; state: the record, 9 floats;
    ch: dict of the C K children's CPU tensors (mask, lb, ub, infeasible, bound, alpha, beta, ub_value, live).  Returns the new record.
    A kept child of rank r goes to slots[r] for r < K, else to in_use + (r - K); one whose slot is not in the pool is dropped: counted in
    [8] and among the closed, its bound lowers closed_lb."""
    K, n, L, off, cap = len(slots), C * len(slots), len(sizes) - 2, offsets(sizes), int(pool["mask"].shape[0])
    rmask, undecided = ch["mask"].clone(), [False] * n
    for c in range(n):
        if not ch["live"][c]:
            continue
        for k in range(L):
            m = rmask[c, off[k]:off[k + 1]]
            lo, up = ch["lb"][k][c], ch["ub"][k][c]
            m = torch.where((m == -1) & (lo >= 0), torch.ones_like(m), m)
            m = torch.where((m == -1) & (up <= 0), torch.zeros_like(m), m)
            rmask[c, off[k]:off[k + 1]] = m
        undecided[c] = bool((rmask[c] == -1).any())
    feasible = [bool(ch["live"][c]) and not bool(ch["infeasible"][c]) for c in range(n)]
    gub = min([state[FS_GLOBAL_UB]] + [float(ch["ub_value"][c]) for c in range(n) if feasible[c]])
    closed_lb, in_use0 = state[FS_CLOSED_LB], min(max(int(state[FS_IN_USE]), 0), cap)
    kept, n_closed = [], 0
    for c in range(n):
        if not feasible[c]:
            continue
        lb = float(ch["bound"][c])
        if undecided[c] and lb < gub - eps and (decision_bound is None or lb < decision_bound):
            kept.append(c)
        else:
            closed_lb, n_closed = min(closed_lb, lb), n_closed + 1
    for i, s in enumerate(slots):                                 # a parent none of whose C rows is live is closed at its own bound
        if 0 <= s < cap and not any(bool(ch["live"][C * i + j]) for j in range(C)):
            closed_lb, n_closed = min(closed_lb, float(pool["bound"][s])), n_closed + 1
    for s in slots:
        if 0 <= s < cap:
            pool["open"][s] = 0
    still_open = [s for s in range(in_use0) if pool["open"][s]]    # what stays open of the pool: the parents are out
    in_use, placed, dropped = in_use0, [], 0
    for r, c in enumerate(kept):                                  # ranks run in child order over all C K rows
        d = slots[r] if r < K else in_use0 + (r - K)
        if not 0 <= d < cap:
            closed_lb, dropped = min(closed_lb, float(ch["bound"][c])), dropped + 1
            continue
        pool["mask"][d], pool["alpha"][d], pool["beta"][d], pool["bound"][d], pool["open"][d] = rmask[c], ch["alpha"][c], ch["beta"][c], ch["bound"][c], 1
        for k in range(L + 1):
            pool["lb"][k][d], pool["ub"][k][d] = ch["lb"][k][c], ch["ub"][k][c]
        in_use = max(in_use, d + 1)
        placed.append(c)
    open_bounds = [float(pool["bound"][s]) for s in still_open] + [float(ch["bound"][c]) for c in placed]
    return [gub, closed_lb, min(open_bounds + [INF]), float(len(open_bounds)), float(in_use), float(len(kept) - dropped), float(n_closed + dropped),
            float(sum(bool(ch["live"][c]) and bool(ch["infeasible"][c]) for c in range(n))), float(dropped)]
