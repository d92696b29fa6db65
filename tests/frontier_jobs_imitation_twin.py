"""The host twin of a many-jobs run that learns, for tests/test_gpu_frontier_jobs_strong.py:
``tests.test_gpu_imitation.host_loop``'s pieces with one state per job, the round's plan from ``frontier.plan_round``, every
``Subproblem.prop_layer`` set to its job's, and per learning round ONE ``ScorerEngine.imitation_step`` on the ``collate`` of all picked
parents in plan row order, the audit's tables as input."""
import numpy as np
import torch

from gnn_branching_amd import _lib, bab_caller, lp_producer, nets
from gnn_branching_amd.frontier import _start_record, _stop_reason, plan_round
from tests.frontier_twin import EPS_BAB, INF, LR, N_ITER, at_least_the_parents, toy, ub64
from tests.imitation_twin import NAN
from tests.test_gpu_frontier_jobs import JOBS


def online_jobs(ids):
    """(a fresh online GraphChoice, the LayerGraphLP of each job of ``ids`` on its engine): a run that learns changes the parameters."""
    _, choice, _ = toy(online=True)
    lps = []
    for j in ids:
        seed, cls, eps, _ = JOBS[j]
        layers = nets.load_verified_net("toy_kw", 2, cls)
        x = torch.from_numpy(np.random.RandomState(seed).standard_normal((3, 32, 32)).astype(np.float32))
        lps.append(lp_producer.LayerGraphLP(layers, x - eps, x + eps, bounds="kw_device", engine=choice.model.engine()))
    return choice, lps


class JobState:
    """One job of the host loop: its LP, its open domains, incumbent, closed bound and rounds."""

    def __init__(self, lp, root_mask, decision_bound):
        self.lp, self.db, self.rounds, self.domains, self.closed = lp, decision_bound, 0, [], INF
        self.fixed = {"fixed_layers": lp.layers[:-1], "prop_layers": [lp.layers[-1]]}
        root = lp.solve_many([(root_mask, None, None)], lp="dual_device", n_iter=N_ITER, lr=LR)[0]
        self.gub = ub64(lp, root)
        self.keep_or_close([root])

    def keep_or_close(self, subs):
        for c in subs:
            if c is None:
                continue
            assert abs(c.lb - (self.gub - EPS_BAB)) > 1e-9, ("the host loop's comparison is within 1e-9 of its threshold", c.lb, self.gub - EPS_BAB)
            if any(bool((m == -1).any()) for m in c.mask) and c.lb < self.gub - EPS_BAB:
                self.domains.append(c)
            else:
                self.closed = min(self.closed, c.lb)

    def record(self):
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
        return self.lp.solve_many(items, lp="dual_device", n_iter=N_ITER, lr=LR)


def host_loop(ids, K, segments, cap, max_rounds, imitate, branching, audit, margin):
    """``verify_properties_strong``'s loop on the host.  audit: the device run's audit rows in order (per launched round, per entry, per
    parent): the tables are an input here, and in "strong" mode so are the decisions.  Returns "entries" (per launched round and entry:
    job, segment, round, run_round, decisions, child_bounds, loss, report, regret, global_lb, global_ub), "results" per job, "steps",
    "rows", "rounds" (launched) and the final "weights"."""
    choice, lps = online_jobs(ids)
    eng = choice._eng()
    root_mask = [torch.full((int(np.prod(lps[0].shapes[i + 1])),), -1, dtype=torch.long) for i in lps[0].pre_relu_indices]
    R = sum(int(m.numel()) for m in root_mask)
    tables = iter(audit)
    seg_job, state, waiting = [None] * segments, [None] * segments, list(range(len(ids)))
    results, entries_out = [None] * len(ids), []
    steps = rows = run_round = 0

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
                state[s] = JobState(lps[seg_job[s]], root_mask, JOBS[ids[seg_job[s]]][3])
        if all(j is None for j in seg_job):
            break
        plan, compact, stopped = plan_round([None if seg_job[s] is None or reason_of(s) is not None else state[s].record() for s in range(segments)], K, cap)
        assert not stopped and not any(compact), "the host loop has no pool: choose a capacity no job fills"
        if not plan:
            continue
        run_round += 1
        subs, round_entries, n_cand = [], [], 0
        for s, row0, k in plan:
            job = state[s]
            job.domains.sort(key=lambda d: d.lb)
            assert len({d.lb for d in job.domains}) == len(job.domains), "two open bounds are equal at a pick"
            picked, job.domains[:] = job.domains[:k], job.domains[k:]
            tab = [next(tables) for _ in picked]
            assert all(a["job"] == seg_job[s] and a["segment"] == s and a["round"] == job.rounds for a in tab)
            round_entries.append((s, picked, [job.as_sub(d) for d in picked], tab))
            n_cand += sum(len(a["candidates"]) for a in tab)
        all_subs = [sub for e in round_entries for sub in e[2]]
        if branching == "strong":
            decs = [list(a["strong_decision"]) for e in round_entries for a in e[3]]
        else:                                                 # one forward over the round's parents under the CURRENT parameters
            decs = [[int(d[0]), int(d[1])] for d in bab_caller.BatchedGraphChoice.decision_many(choice, all_subs, state[plan[0][0]].fixed)]
        outs, at = [], 0
        for s, picked, _, tab in round_entries:
            job, k = state[s], len(picked)
            children = at_least_the_parents(job.children_of(zip(picked, decs[at:at + k])), [d for d in picked for _ in (0, 1)])
            job.gub = min([job.gub] + [ub64(job.lp, c) for c in children if c is not None])
            job.keep_or_close(children)                       # commit first, then learn
            outs.append({"job": seg_job[s], "segment": s, "round": job.rounds, "run_round": run_round, "decisions": decs[at:at + k],
                         "child_bounds": [INF if c is None else c.lb for c in children], "loss": [], "report": [], "regret": [],
                         "global_lb": job.global_lb(), "global_ub": job.gub})
            job.rounds += 1
            at += k
        if run_round % imitate == 0 and n_cand > 0:           # ONE step over all the round's parents, in plan row order
            table = np.full((len(all_subs), R), NAN)
            i = 0
            for e in round_entries:
                for a in e[3]:
                    table[i, a["candidates"]] = a["improvements"]
                    i += 1
            args, _ = bab_caller.collate(all_subs, state[plan[0][0]].fixed)
            loss, report, regret = (v.tolist() for v in eng.imitation_step(args, table, margin))
            steps, rows, at = steps + 1, rows + len(all_subs), 0
            for o in outs:
                k = len(o["decisions"])
                o.update(loss=loss[at:at + k], report=report[at:at + k], regret=regret[at:at + k])
                at += k
        entries_out.extend(outs)
    assert next(tables, None) is None, "the device run audited parents the host loop never picked"
    return {"entries": entries_out, "results": results, "steps": steps, "rows": rows, "rounds": run_round, "weights": eng.get_weights().copy()}
