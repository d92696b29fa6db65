"""Branch-and-bound on one robustness property with the MI355X scorer and the Gurobi-free LP producer.

    python examples/bab_demo.py [--net cifar_base_kw] [--eps 0.03] [--nodes 40] [--babsr | --threshold 0.2 | --frontier 16 [--threshold 0.2 [--online 5] | --branching babsr | --branching strong [--candidates 16] [--gnn-candidates 4] | --imitate 1 [--imitate-margin 1.0] [--replay 1024 [--replay-batch 8] [--replay-steps 1]] [--candidates 16] [--gnn-candidates 4]] [--props 18 [--threshold 0.2 --online 5 | --branching strong [--candidates 16] [--gnn-candidates 4] | --imitate 1 [--imitate-margin 1.0] [--replay 1024 [--replay-batch 8] [--replay-steps 1]] [--candidates 16] [--gnn-candidates 4]]] [--witness] [--pgd 4 [--restarts 16]] [--split-depth 4]] [--bounds kw_device]

--threshold T runs the reference loop's own control flow (relu_conv_gnnkwthreshold.py:150-199): a GNN decision whose improvement of the bound is
below T makes the loop ask the BaBSR heuristic too (on the device), bound its children and keep the better pair; try --eps 0.09.

--frontier K keeps the open domains in device memory and expands the K of lowest bound per round (gnn_branching_amd/frontier.py): bounds by
gnnb_kw_bounds and 20 steps of gnnb_dual_ascent, GNN decisions, --nodes // (2 K) rounds at least one; no LP is solved.  With --threshold T
the rounds run --threshold's control flow on the device: the parents whose GNN split improves the bound by less than
T get their BaBSR split bounded too, in the same round, and the better pair is kept.  With --online N on top the
run also learns, as plnn/relu_conv_online.py does: a GNN decision that lost to BaBSR's N times makes its parent a learn row, and the round
takes one Adam step over its learn rows on the device.  With --props N it
verifies N properties in one frontier (frontier.verify_properties): the image of seed --seed + j // 9 against the j % 9-th class other than
the true one, every round's launches serving all the properties in flight; one verdict line per property.  --props N with --threshold T runs
the fall-back for every property (frontier.verify_properties_threshold): each has its own intercept counter and table of
inefficient points, and one round bounds the second pairs of all the properties' selected parents together.  --props N with --threshold T
--online M learns online over all of them (frontier.verify_properties_online): every property has its own table of
wrong GNN points, and a round takes ONE Adam step over the learn rows of all the properties in flight, which share the GNN.  --witness (with --frontier)
also returns the input point the upper bound belongs to -- the counter-example, when the verdict is one -- and prints the network's value
at it; --pgd N lowers every child's upper bound by up to N projected gradient steps on the network from its LP point;
--restarts R with --pgd N also descends from R uniform points of every child's box and keeps the least value (section 7.9; --pgd 0: the points alone).
--frontier K --branching babsr branches on the BaBSR heuristic alone, as the reference's relu_bab does: the same
rounds, bounds and pick rule with gnnb_babsr and the decision rule on the device in the GNN's place -- what the GNN's branch count is compared
with; with --props N every property has its own intercept counter (frontier.verify_properties_babsr).  (--babsr alone is the host loop.)
--frontier K --branching strong is strong branching, the strategy the GNN was trained to imitate: both children of
every candidate split of every parent are bounded on the device and the parent splits where its bound improves most; --candidates M keeps
the M undecided nodes of highest BaBSR score as candidates (without it every undecided node is one: thousands per parent on the CIFAR nets).
--gnn-candidates G shortlists the G undecided nodes of highest GNN score as well, or alone without --candidates
(frontier.Shortlist): the GNN proposes, the bounds dispose, and with --imitate the table always labels the split the GNN made.
--frontier K --imitate N (with the GNN or --branching strong) makes every N-th round a learning round: its parents'
strong-branching table stays on the device and the GNN takes one Adam step towards ranking the table's best candidate first, by
--imitate-margin M times the difference of the improvements.
--imitate N --replay C keeps the labelled states: a learning round stores its parents and their table rows in a
device-resident replay buffer of C slots and takes --replay-steps steps (default 1; 0 collects only, with a frozen GNN), each on
--replay-batch entries (default 8) drawn from everything stored so far.
--props N with --branching strong, or with --imitate N, runs both for every property in one pool (frontier.verify_properties_strong,
DESIGN.md section 7.13): the candidates of all properties' parents are bounded in the same chunks, and a learning round -- every N-th round
the run launches -- takes ONE step over the parents of all the properties in flight, which share the GNN.
--frontier K --split-depth D (one property, the GNN's branching) fills the rounds that have fewer than K parents:
each parent is split on up to D of its best-scored undecided ReLUs at once, 2^d children per parent on the round's 2K child rows.

Prints the trace of plnn/relu_conv_gnnkwthreshold.py:202 for every branch.  Needs the GPU library (no CPU fallback)."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gnn_branching_amd import lp_producer, nets                     # noqa: E402
from gnn_branching_amd.graphnet.graph_score import GraphChoice      # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "models", "cifar_trained_gnn",
                    "best_snapshot_None_0_val_acc_0.826_loss_val_0.1036_epoch_57.pt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="cifar_base_kw")
    ap.add_argument("--eps", type=float, default=0.03)
    ap.add_argument("--nodes", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--babsr", action="store_true", help="branch with the BaBSR heuristic instead of the GNN")
    ap.add_argument("--bounds", default="kw", choices=("kw", "interval", "kw_device"),
                    help="intermediate bounds: host fp64 Wong-Kolter, interval arithmetic, or Wong-Kolter on the GPU (gnnb_kw_bounds)")
    ap.add_argument("--tighten", type=int, default=0, metavar="N",
                    help="tighten the root's intermediate bounds by N steps of dual ascent per ambiguous node (gnnb_kw_tighten with --frontier or "
                         "--bounds kw_device, the host twin with --bounds kw); every child inherits them")
    ap.add_argument("--threshold", type=float, default=None, help="branching_threshold of the GNN + KW fall-back loop (the reference uses 0.2)")
    ap.add_argument("--frontier", type=int, default=None, metavar="K", help="device-resident frontier: expand the K most promising domains per round")
    ap.add_argument("--online", type=int, default=None, metavar="N", help="with --frontier K --threshold T: learn online, online_threshold N (the reference uses 5)")
    ap.add_argument("--props", type=int, default=None, metavar="N", help="with --frontier: verify N properties (seeds x wrong classes) in one frontier")
    ap.add_argument("--witness", action="store_true", help="with --frontier: return the point of the upper bound and print the network's value at it")
    ap.add_argument("--pgd", type=int, default=None, metavar="N", help="with --frontier: up to N projected gradient steps from every child's LP point")
    ap.add_argument("--restarts", type=int, default=None, metavar="R", help="with --pgd N: also descend from R uniform points of every child's box")
    ap.add_argument("--branching", default=None, choices=("gnn", "babsr", "strong"),
                    help="with --frontier K: what picks the split, the GNN (default), the BaBSR heuristic alone, or strong branching")
    ap.add_argument("--candidates", type=int, default=None, metavar="M", help="with --branching strong: bound the M undecided nodes of highest BaBSR score only")
    ap.add_argument("--gnn-candidates", type=int, default=None, metavar="G", help="with --branching strong or --imitate N: also bound the G undecided nodes of highest GNN score")
    ap.add_argument("--imitate", type=int, default=None, metavar="N", help="with --frontier K: every N-th round learns the GNN from its strong-branching table")
    ap.add_argument("--imitate-margin", type=float, default=None, metavar="M", help="with --imitate N: the margin per unit of improvement (default 1.0)")
    ap.add_argument("--replay", type=int, default=None, metavar="C", help="with --imitate N: learn from a device-resident replay buffer of C labelled states")
    ap.add_argument("--replay-batch", type=int, default=None, metavar="B", help="with --replay C: entries per step (default 8, 256 at most)")
    ap.add_argument("--replay-steps", type=int, default=None, metavar="S", help="with --replay C: steps per learning round (default 1; 0: collect only)")
    ap.add_argument("--split-depth", type=int, default=None, metavar="D",
                    help="with --frontier K: split each parent of an underfilled round on up to D ReLUs at once (1..8)")
    ap.add_argument("--repack", default=None, choices=("host", "device"),
                    help="with --frontier K and --online N (also with --props) or --imitate N (one property): where the scorer's packs are rebuilt after a learning step "
                         "(device: on the stream, the step does not wait; DESIGN.md section 7.15)")
    args = ap.parse_args()
    if args.imitate is not None and (args.frontier is None or args.imitate < 1 or args.branching == "babsr" or args.threshold is not None
                                     or args.online is not None):
        ap.error("--imitate N needs --frontier K and N >= 1, and takes no --branching babsr, --threshold or --online")
    if args.imitate_margin is not None and (args.imitate is None or not args.imitate_margin >= 0):
        ap.error("--imitate-margin M needs --imitate N, and M >= 0")
    if args.replay is not None and (args.imitate is None or not 1 <= args.replay <= 65536):
        ap.error("--replay C needs --imitate N, and 1 <= C <= 65536")
    if (args.replay_batch is not None or args.replay_steps is not None) and args.replay is None:
        ap.error("--replay-batch and --replay-steps need --replay C")
    if args.replay_batch is not None and not 1 <= args.replay_batch <= min(256, args.replay):
        ap.error("--replay-batch B: 1 <= B <= min(256, C)")
    if args.replay_steps is not None and args.replay_steps < 0:
        ap.error("--replay-steps S: S >= 0")
    imitate = args.imitate
    if args.replay is not None:                                  # the value of imitate that keeps the labelled states
        from gnn_branching_amd.frontier import Replay
        imitate = Replay(every=args.imitate, capacity=args.replay, batch=min(args.replay, 8) if args.replay_batch is None else args.replay_batch,
                         steps=1 if args.replay_steps is None else args.replay_steps)
    if args.repack is not None and (args.frontier is None or (args.props is not None and args.online is None) or
                                    (args.online is None and args.imitate is None)):
        ap.error("--repack needs --frontier K with --online N or --imitate N, and one property (no --props) unless it is --online N")
    if args.branching is not None and args.frontier is None:
        ap.error("--branching needs --frontier K (--babsr is the host loop's BaBSR)")
    if args.branching == "babsr" and (args.threshold is not None or args.online is not None):
        ap.error("--branching babsr takes no --threshold and no --online: it never asks the GNN")
    if args.branching == "strong" and (args.threshold is not None or args.online is not None):
        ap.error("--branching strong takes no --threshold and no --online: it never asks the GNN")
    if args.candidates is not None and ((args.branching != "strong" and args.imitate is None) or args.candidates < 1):
        ap.error("--candidates M needs --branching strong or --imitate N, and M >= 1")
    if args.gnn_candidates is not None and ((args.branching != "strong" and args.imitate is None) or args.gnn_candidates < 1):
        ap.error("--gnn-candidates G needs --branching strong or --imitate N, and G >= 1")
    if args.split_depth is not None and (args.frontier is None or args.props is not None or not 1 <= args.split_depth <= 8 or args.branching in ("babsr", "strong")
                                         or args.threshold is not None or args.online is not None or args.imitate is not None):
        ap.error("--split-depth D needs --frontier K and 1 <= D <= 8, and takes no --props, --branching babsr / strong, --threshold, --online or --imitate")
    branching = args.branching or "gnn"
    candidates = args.candidates
    if args.gnn_candidates is not None:                          # the value of strong_candidates that names both shortlists
        from gnn_branching_amd.frontier import Shortlist
        candidates = Shortlist(babsr=args.candidates, gnn=args.gnn_candidates)
    if args.restarts is not None and (args.pgd is None or not 0 <= args.restarts <= 4096):
        ap.error("--restarts R needs --pgd N, and 0 <= R <= 4096")
    if (args.witness or args.pgd is not None) and (args.frontier is None or (args.pgd is not None and args.pgd < 0)):
        ap.error("--witness and --pgd N need --frontier K, and N >= 0")
    upper = {"witness": [] if args.witness else None, "pgd_steps": args.pgd, "pgd_restarts": args.restarts}

    def witness_of(point, fixed, prop_layer):
        """The network's value (fp64, torch on the host) at a witness."""
        if point is None:
            return "; no upper bound point"
        with torch.no_grad():
            act = point[None].double()
            for l in list(fixed) + [prop_layer]:
                act = copy.deepcopy(l).double()(act)
        return f"; network value at the witness {float(act.reshape(())):.5f}"
    if args.props is not None and (args.frontier is None or args.props < 1):
        ap.error("--props N needs --frontier K and N >= 1")
    if args.online is not None and (args.frontier is None or args.threshold is None or args.online < 1):
        ap.error("--online N needs --frontier K --threshold T and N >= 1")

    def verdict_of(glb, gub):
        return "property holds" if glb >= 0 else ("counter-example found" if gub < 0 else "undecided within the node budget")
    if args.props is not None:
        from gnn_branching_amd.frontier import (FrontierJob, FrontierJobs, verify_properties, verify_properties_babsr, verify_properties_online,
                                                verify_properties_strong, verify_properties_threshold)
        wrong, jobs, names = [c for c in range(10) if c != 3], [], []
        for j in range(args.props):
            seed, cls = args.seed + j // 9, wrong[j % 9]
            prop = nets.load_verified_net(args.net, 3, cls)
            x = torch.from_numpy(np.random.RandomState(seed).standard_normal((3, 32, 32)).astype(np.float32))
            jobs.append(FrontierJob(x - args.eps, x + args.eps, prop[-1], 0.0))
            names.append(f"seed {seed} class 3 vs {cls}")
        lp = lp_producer.LayerGraphLP(prop, x - args.eps, x + args.eps, bounds="kw_device")
        learns = args.imitate is not None or args.online is not None
        if learns:                                               # the properties of a pool share the GNN that learns
            from gnn_branching_amd.graphnet.graph_score_online import GraphChoice as OnlineGraphChoice
        choice = (OnlineGraphChoice if learns else GraphChoice)([torch.zeros(int(np.prod(lp.shapes[i + 1]))) for i in lp.pre_relu_indices], CKPT)
        max_rounds, stats, learned = max(1, args.nodes // (2 * args.frontier)), [], {}
        if branching == "strong" or args.imitate is not None:
            margin = {} if args.imitate_margin is None else {"imitate_margin": args.imitate_margin}
            results = verify_properties_strong(choice, prop[:-1], FrontierJobs(jobs, **upper, tighten_root=args.tighten), K=args.frontier, max_rounds=max_rounds, log=lambda s: None,
                                               stats=stats, learned=learned, imitate=imitate, strong_candidates=candidates, branching=branching,
                                               **margin)
        elif branching == "babsr":
            results = verify_properties_babsr(choice, prop[:-1], FrontierJobs(jobs, **upper, tighten_root=args.tighten), K=args.frontier, max_rounds=max_rounds, log=lambda s: None)
        elif args.threshold is None:
            results = verify_properties(choice, prop[:-1], FrontierJobs(jobs, **upper, tighten_root=args.tighten), K=args.frontier, max_rounds=max_rounds, log=lambda s: None)
        elif args.online is not None:
            results = verify_properties_online(choice, prop[:-1], FrontierJobs(jobs, **upper, tighten_root=args.tighten), args.threshold, args.online,
                                               K=args.frontier, max_rounds=max_rounds, log=lambda s: None, stats=stats, learned=learned,
                                               **({} if args.repack is None else {"repack": args.repack}))
        else:
            results = verify_properties_threshold(choice, prop[:-1], FrontierJobs(jobs, **upper, tighten_root=args.tighten), args.threshold, K=args.frontier, max_rounds=max_rounds, log=lambda s: None,
                                                  stats=stats)
        for j, (name, (glb, gub, rounds, bounded, reason)) in enumerate(zip(names, results)):
            kw = ""
            if stats and "kw_bounded" in stats[j]:
                kw = f"; {stats[j]['kw_bounded']} of {stats[j]['branches']} parents bounded a KW decision, {stats[j]['kw_used']} kept it"
                if "online_rows" in stats[j]:
                    kw += f", {stats[j]['online_rows']} learn rows"
            if stats and "strong_bounded" in stats[j]:
                kw = f"; {stats[j]['branches']} branches by {branching}, {stats[j]['strong_bounded']} candidate children bounded"
            if args.witness:
                kw += witness_of(upper["witness"][j], prop[:-1], jobs[j].prop_layer)
            print(f"{name}: after {rounds} rounds ({bounded} domains bounded, stopped on: {reason}{kw}): lb {glb:.5f} ub {gub:.5f} -> {verdict_of(glb, gub)}")
        if args.online is not None:
            print(f"{learned['online_steps']} learning steps over {learned['online_rows']} learn rows in {learned['rounds']} rounds of the pool")
        if args.imitate is not None:
            print(f"{learned['imitation_steps']} imitation steps over {learned['imitation_rows']} parent rows in {learned['rounds']} rounds of the pool")
            if args.replay is not None:
                print(f"replay buffer: {learned['replay_stored']} states stored, {learned['replay_skipped']} skipped, {learned['replay_filled']} held")
        return
    layers = nets.load_verified_net(args.net, 3, 5)
    x = torch.from_numpy(np.random.RandomState(args.seed).standard_normal((3, 32, 32)).astype(np.float32))
    if args.frontier is not None:
        from gnn_branching_amd.frontier import branch_and_bound_frontier
        lp = lp_producer.LayerGraphLP(layers, x - args.eps, x + args.eps, bounds="kw_device", tighten_root=args.tighten, split_depth=args.split_depth)
        learns = args.online is not None or args.imitate is not None
        if learns:
            from gnn_branching_amd.graphnet.graph_score_online import GraphChoice as OnlineGraphChoice
        choice = (OnlineGraphChoice if learns else GraphChoice)([torch.zeros(int(np.prod(lp.shapes[i + 1]))) for i in lp.pre_relu_indices], CKPT)
        stats = {}
        if args.imitate is not None:
            upper.update(imitate=imitate, **({} if args.imitate_margin is None else {"imitate_margin": args.imitate_margin}))
        if args.repack is not None:
            upper.update(repack=args.repack)
        glb, gub, rounds, bounded, reason = branch_and_bound_frontier(lp, choice, layers, K=args.frontier, decision_bound=0.0,
                                                                      max_rounds=max(1, args.nodes // (2 * args.frontier)),
                                                                      branching_threshold=args.threshold, stats=stats, online_threshold=args.online,
                                                                      strong_candidates=candidates, branching=branching, **upper)
        verdict = "property holds" if glb >= 0 else ("counter-example found" if gub < 0 else "undecided within the node budget")
        kw = "" if args.threshold is None else f"; {stats['kw_bounded']} of {stats['branches']} parents bounded a KW decision, {stats['kw_used']} kept it"
        if args.online is not None:
            kw += f"; {stats['online_steps']} learning steps over {stats['online_rows']} learn rows"
        if args.imitate is not None:
            kw += f"; {stats['imitation_steps']} imitation steps over {stats['imitation_rows']} parent rows"
            if args.replay is not None:
                kw += f" drawn from a replay buffer ({stats['replay_stored']} states stored, {stats['replay_skipped']} skipped, {stats['replay_filled']} held)"
        if args.witness:
            kw += witness_of(upper["witness"][0], layers[:-1], layers[-1])
        by = "" if args.branching is None else f"{stats['branches']} branches by {branching}, "
        if branching == "strong":
            by += f"{stats['strong_bounded']} candidate children bounded, "
        print(f"after {rounds} rounds ({by}{bounded} domains bounded, stopped on: {reason}{kw}): lb {glb:.5f} ub {gub:.5f} -> {verdict}")
        return
    if args.tighten and args.bounds == "interval":
        ap.error("--tighten tightens Wong-Kolter bounds: it needs --bounds kw or kw_device (or --frontier)")
    lp = lp_producer.LayerGraphLP(layers, x - args.eps, x + args.eps, bounds=args.bounds, tighten_root=args.tighten)
    root_mask = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
    root = lp.solve(root_mask)
    print(f"root: lb {root.lb:.5f} ub {root.ub:.5f}, undecided ReLUs per layer {[int((m == -1).sum()) for m in root.mask]}")
    if args.threshold is not None:
        from gnn_branching_amd.plnn.kw_score_conv import choose_node_conv
        choice = GraphChoice(root.mask, CKPT)

        def kw(sub, icp, random_order, sparsest_layer):
            return choose_node_conv(sub.lower_all, sub.upper_all, sub.mask, lp.layers, lp.pre_relu_indices, icp, random_order, sparsest_layer)
        glb, gub, solves, branches, n_kw, n_used = lp_producer.branch_and_bound_threshold(
            lp, lp_producer.gnn_scorer(choice, lp), kw, layers, max_branches=args.nodes // 2, decision_bound=0.0, branching_threshold=args.threshold)
        verdict = "property holds" if glb >= 0 else ("counter-example found" if gub < 0 else "undecided within the node budget")
        print(f"after {branches} branches ({solves} LP solves; {n_kw} bounded a KW decision, {n_used} kept it): lb {glb:.5f} ub {gub:.5f} -> {verdict}")
        return
    if args.babsr:
        scorer = lp_producer.babsr_scorer(lp)
    else:
        choice = GraphChoice(root.mask, CKPT)
        scorer = lp_producer.gnn_scorer(choice, lp)
    glb, gub, visited = lp_producer.branch_and_bound(lp, scorer, layers, max_nodes=args.nodes, decision_bound=0.0)
    verdict = "property holds" if glb >= 0 else ("counter-example found" if gub < 0 else "undecided within the node budget")
    print(f"after {visited} LP solves: lb {glb:.5f} ub {gub:.5f} -> {verdict}")


if __name__ == "__main__":
    main()
