"""The host twin of a many-jobs run that learns online, for tests/test_frontier_jobs_online_cpu.py and
tests/test_gpu_frontier_jobs_online.py.

``learn_jobs_reference``: the per-entry walk of ``gnnb_frontier_learn_jobs`` and its compaction restated with
``bab_caller.resolve_online`` and the flat ReLU index; no device.

``host_loop``: ``verify_properties_online``'s loop made of public pieces -- the threshold round of ``tests.frontier_twin.twin`` with
``resolve_online`` and one ``wrong`` dict and one intercept counter per job, the round's plan from ``frontier.plan_round``, the parameters
frozen for the round, and per round ONE ``ScorerEngine.online_step`` over the learn rows of all jobs in plan-entry order, on their own
forward arguments."""
import numpy as np
import torch

from gnn_branching_amd import bab_caller, lp_producer
from gnn_branching_amd.bab_caller import gnn_improvement, resolve_online
from gnn_branching_amd.frontier import _stop_reason, plan_round
from tests.frontier_twin import EPS_BAB, INF, at_least_the_parents, ub64


# ---- the walk and the compaction, without a device ---------------------------------------------------------------------------------
def learn_jobs_reference(relu, entries, rows, wrong, thr):
    """relu: the ReLU layer sizes; entries: the plan [(segment, row0, k)]; rows: "gnn_dec" / "kw_dec" ([lay, idx] per global row), "used",
    "gnn_imp", "kw_imp" (per global row) as sequences; wrong: {segment: list of R counts}, not mutated; thr: online_threshold.

    Returns (learn_rows -- GLOBAL row numbers --, learn_kw, learn_imp: the dense lists in plan-entry order and within an entry in row
    order; learn_entry: the count per entry, then their sum; the tables afterwards as {segment: list})."""
    off = [0] + list(np.cumsum(relu))

    def flat(d):
        return int(off[d[0]] + d[1]) if 0 <= d[0] < len(relu) and 0 <= d[1] < relu[d[0]] else None
    after = {s: list(w) for s, w in wrong.items()}
    staged = []
    for seg, row0, k in entries:                              # the walk: one entry at a time, against its segment's table alone
        w, mine = after[seg], []
        for row in range(row0, row0 + k):
            gd, kd = [int(v) for v in rows["gnn_dec"][row]], [int(v) for v in rows["kw_dec"][row]]
            if not int(rows["used"][row]) or flat(gd) is None or flat(kd) is None:
                continue
            key = f"{gd[0]}-{gd[1]}"
            table = {key: w[flat(gd)]}
            dec, used, learn, improve = resolve_online(gd, float(rows["gnn_imp"][row]), kd, float(rows["kw_imp"][row]), table, thr)
            assert used and dec == kd                         # the row is consistent: used_kw is resolve_online's own choice
            w[flat(gd)] = table[key]
            if learn:
                mine.append((row, flat(kd), float(improve)))
        staged.append(mine)
    dense = [item for mine in staged for item in mine]        # the compaction: the staged slices in plan order
    counts = [len(mine) for mine in staged]
    return [r for r, _, _ in dense], [k for _, k, _ in dense], [v for _, _, v in dense], counts + [sum(counts)], after


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
class OnlineJobState:
    """One job of the host loop: its LP, its open domains, incumbent, closed bound and rounds, its intercept counter and its own table of
    wrong GNN points (the reference's wrong_pts_dc belongs to the GraphChoice it builds per property)."""

    def __init__(self, lp, root_mask, decision_bound, n_iter, lr):
        self.lp, self.db, self.rounds, self.domains, self.closed = lp, decision_bound, 0, [], INF
        self.n_iter, self.lr, self.icp, self.wrong = n_iter, lr, 0, {}
        self.fixed = {"fixed_layers": lp.layers[:-1], "prop_layers": [lp.layers[-1]]}
        root = lp.solve_many([(root_mask, None, None)], lp="dual_device", n_iter=n_iter, lr=lr)[0]
        self.gub = ub64(lp, root)
        self.keep_or_close([root])

    def keep_or_close(self, subs):
        for c in subs:
            if c is None:
                continue
            clear(c.lb, self.gub - EPS_BAB)
            if any(bool((m == -1).any()) for m in c.mask) and c.lb < self.gub - EPS_BAB:
                self.domains.append(c)
            else:
                self.closed = min(self.closed, c.lb)

    def record(self):
        from gnn_branching_amd import _lib
        from gnn_branching_amd.frontier import _start_record
        st = _start_record()
        st[_lib.FS_GLOBAL_UB], st[_lib.FS_CLOSED_LB] = self.gub, self.closed
        st[_lib.FS_LOWEST_OPEN] = min([d.lb for d in self.domains], default=INF)
        st[_lib.FS_N_OPEN] = st[_lib.FS_IN_USE] = float(len(self.domains))
        return st

    def global_lb(self):
        return min([d.lb for d in self.domains] + [self.closed, self.gub])

    def as_sub(self, d):
        lp = self.lp
        return bab_caller.Subproblem(*d.graph_bounds(lp.pre_relu_indices, len(lp.layers)), d.dual_vars, d.ub_point, d.primals, d.mask, lp.layers[-1])

    def children_of(self, pairs):
        items = []
        for d, dec in pairs:
            for c in (0, 1):
                m = [t.clone() for t in d.mask]
                m[dec[0]][dec[1]] = c
                items.append((m, d, dec[0]))
        return at_least_the_parents(self.lp.solve_many(items, lp="dual_device", n_iter=self.n_iter, lr=self.lr), [d for _, d, _ in items])


def clear(a, b):
    assert abs(a - b) > 1e-9, ("the twin's comparison is within 1e-9 of its threshold", a, b)


def bounds_of(subs):
    return [INF if c is None else c.lb for c in subs]


def host_loop(choice, lps, decision_bounds, K, segments, cap, max_rounds, threshold, online_threshold, n_iter, lr, need_two_jobs=True):
    """``verify_properties_online``'s loop on the host.  choice: a fresh online GraphChoice; lps: the LayerGraphLP of every job on its
    engine; decision_bounds: per job.  Returns "entries" (per launched round and plan entry: job, segment, round, run_round and the
    keys of the device trace), "results" per job, "steps", "rows", "rounds" (launched), "first_step" (the launched round that took
    the first step) and the final "weights".

    Asserts ITS OWN conditions: no two open bounds equal at a pick; no keep-or-close comparison, no improvement and no improve test
    within 1e-9 of its threshold; at least one step was taken and a forward ran after it; with ``need_two_jobs``, at least one step
    summed learn rows of two different jobs."""
    eng = choice._eng()
    root_mask = [torch.full((int(np.prod(lps[0].shapes[i + 1])),), -1, dtype=torch.long) for i in lps[0].pre_relu_indices]
    off = [0] + list(np.cumsum([int(m.numel()) for m in root_mask]))
    order = lp_producer._random_order(len(lps[0].pre_relu_indices), 0)
    seg_job, state, waiting = [None] * segments, [None] * segments, list(range(len(lps)))
    results, entries_out = [None] * len(lps), []
    steps = rows = run_round = 0
    first_step, forward_after_step, two_jobs = None, False, False

    def reason_of(s):
        return _stop_reason(state[s].record(), EPS_BAB, state[s].db, state[s].rounds, max_rounds)

    while True:
        for s in range(segments):
            if seg_job[s] is not None and reason_of(s) is not None:
                results[seg_job[s]] = (state[s].global_lb(), state[s].gub, state[s].rounds, None, reason_of(s))
                seg_job[s], state[s] = None, None
        for s in range(segments):
            if seg_job[s] is None and waiting:
                seg_job[s] = waiting.pop(0)
                state[s] = OnlineJobState(lps[seg_job[s]], root_mask, decision_bounds[seg_job[s]], n_iter, lr)
        if all(j is None for j in seg_job):
            break
        plan, compact, stopped = plan_round([None if seg_job[s] is None or reason_of(s) is not None else state[s].record() for s in range(segments)], K, cap)
        assert not stopped and not any(compact), "the host loop has no pool: choose a capacity no job fills"
        if not plan:
            continue
        run_round += 1
        picked_of, subs = [], []
        for s, row0, k in plan:
            job = state[s]
            job.domains.sort(key=lambda d: d.lb)
            assert len({d.lb for d in job.domains}) == len(job.domains), "two open bounds are equal at a pick"
            picked, job.domains[:] = job.domains[:k], job.domains[k:]
            picked_of.append(picked)
            subs += [job.as_sub(d) for d in picked]
        # ONE forward over the round's parents of all jobs, under the round's opening parameters
        decs = [[int(d[0]), int(d[1])] for d in bab_caller.BatchedGraphChoice.decision_many(choice, subs, state[plan[0][0]].fixed)]
        forward_after_step |= steps > 0
        outs, l_rows, l_kw, l_imp, l_jobs = [], [], [], [], []
        for (s, row0, k), picked in zip(plan, picked_of):
            job, mine = state[s], decs[row0:row0 + k]
            children = job.children_of(zip(picked, mine))
            lbs = bounds_of(children)
            imps = [gnn_improvement(lbs[2 * i], lbs[2 * i + 1], d.lb) if d.lb < 0 else 1.0 for i, d in enumerate(picked)]
            kws, selected = [[-1, -1] for _ in picked], []
            for i, d in enumerate(picked):                    # row order: the job's intercept counter is carried from parent to parent
                clear(imps[i], threshold)
                if imps[i] < threshold:                       # no table of inefficient points: every KW decision is bounded
                    (kw,), (job.icp,) = bab_caller.BatchedGraphChoice.kw_decision_many(choice, [subs[row0 + i]], job.fixed, [job.icp], order, 0)
                    kws[i] = [int(kw[0]), int(kw[1])]
                    selected.append(i)
            kw_children = job.children_of([(picked[i], kws[i]) for i in selected]) if selected else []
            kw_lbs = bounds_of(kw_children)
            final, used, kw_imps = [list(d) for d in mine], [0] * k, [-1.0] * k
            e_rows, e_kw, e_imp = [], [], []
            for j, i in enumerate(selected):                  # row order: two parents of one job that name one node both count
                kw_imps[i] = gnn_improvement(kw_lbs[2 * j], kw_lbs[2 * j + 1], picked[i].lb)
                if kws[i] == mine[i]:                         # BaBSR names the GNN's node: the same two children, the same bounds
                    assert kw_imps[i] == imps[i]
                else:
                    clear(kw_imps[i], imps[i])
                clear(kw_imps[i] - imps[i], 0.1)
                dec, u, learn, improve = resolve_online(mine[i], imps[i], kws[i], kw_imps[i], job.wrong, online_threshold)
                if learn:
                    e_rows.append(i)
                    e_kw.append(int(off[kws[i][0]] + kws[i][1]))
                    e_imp.append(float(improve))
                final[i], used[i] = [int(dec[0]), int(dec[1])], int(u)
                if u:
                    children[2 * i], children[2 * i + 1] = kw_children[2 * j], kw_children[2 * j + 1]
            job.gub = min([job.gub] + [ub64(job.lp, c) for c in children if c is not None])
            job.keep_or_close(children)                       # the commit does not depend on the parameters: first commit, then learn
            outs.append({"job": seg_job[s], "segment": s, "round": job.rounds, "run_round": run_round, "decisions": final, "gnn_decisions": mine,
                         "kw_decisions": kws, "used_kw": used, "gnn_improvement": imps, "kw_improvement": kw_imps, "selected": selected,
                         "child_bounds": bounds_of(children), "learn_rows": e_rows, "learn_kw": e_kw, "learn_improve": e_imp, "loss": [],
                         "global_lb": job.global_lb(), "global_ub": job.gub})
            job.rounds += 1
            l_rows += [row0 + i for i in e_rows]
            l_kw += e_kw
            l_imp += e_imp
            l_jobs += [seg_job[s]] * len(e_rows)
        if l_rows:                                            # ONE step over the learn rows of all jobs, in plan-entry order
            args, _ = bab_caller.collate([subs[r] for r in l_rows], state[plan[0][0]].fixed)
            loss = eng.online_step(args, l_kw, l_imp)[0].tolist()
            steps, rows, at = steps + 1, rows + len(l_rows), 0
            first_step = run_round if first_step is None else first_step
            two_jobs |= len(set(l_jobs)) >= 2
            for o in outs:
                n = len(o["learn_rows"])
                o["loss"] = loss[at:at + n]
                at += n
        entries_out.extend(outs)
    assert steps >= 1 and forward_after_step, ("the twin never decided with learned parameters: the comparison would show nothing", steps)
    if need_two_jobs:
        assert two_jobs, "no step of the twin summed learn rows of two different jobs"
    return {"entries": entries_out, "results": results, "steps": steps, "rows": rows, "rounds": run_round, "first_step": first_step,
            "weights": eng.get_weights().copy()}
