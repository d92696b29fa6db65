"""The exact anchor on the CPU (tests/exact_minimum.py, tests/golden/exact_minima.npz): every stored minimum is certified and can be
derived again; on every stored domain the host twin obeys  dual ascent <= LP optimum <= exact minimum;  the host Wong-Kolter bounds
contain the network at the minimiser and bracket the stored per-node exact extrema; the MILP gives the same minimum with Wong-Kolter
big-M constants as with interval ones; and the yardstick bites: with the split clamp's two phases exchanged the host LP bound lies more than 100 slacks above the exact
minimum of a stored child."""
import numpy as np
import pytest
import torch

from tests import exact_minimum as E

FIX = E.load()
CASES = list(FIX)
# what a default run derives again (seconds each); the others carry the `slow` mark (GNNB_RUN_SLOW=1)
QUICK = [c for c in CASES if c.startswith("kwg_single@")]
_lps, _roots = {}, {}


def lp_of(case):
    if case not in _lps:
        _lps[case] = E.case_lp(case, FIX[case])
    return _lps[case]


def root_bounds(case):
    if case not in _roots:
        lp = lp_of(case)
        _roots[case] = lp.kw_bounds(E.root_mask(lp))
    return _roots[case]


def domain(case, k):
    """(mask, parent bounds or None, split layer or None) of stored domain k."""
    e, lp = FIX[case], lp_of(case)
    mask = E.split_mask(lp, e["masks"][k])
    if int(e["parent"][k]) < 0:
        return mask, None, None
    return mask, root_bounds(case), int(e["split"][k])


def feasible(case):
    return [k for k in range(len(E.DOMAINS)) if int(FIX[case]["status"][k]) == 0]


def test_every_entry_is_certified_and_both_signs_exist():
    signs = {}
    for case, e in FIX.items():
        assert e["masks"].shape[0] == len(E.DOMAINS) and list(e["status"]) == [0] * (len(E.DOMAINS) - 1) + [2], case
        for k in feasible(case):
            assert e["m_up"][k] - e["m_lo"][k] <= E.CERT_GAP, (case, E.DOMAINS[k], e["m_lo"][k], e["m_up"][k])
            assert e["m_lo"][k] >= e["m_lo"][0] - E.slack(e["m_lo"][0]), (case, E.DOMAINS[k])      # a part of the box: no lower than the root
        assert np.isnan(e["m_lo"][-1]) and np.isnan(e["m_up"][-1])
        for lo0, lo1, hi0, hi1 in e["node_extrema"]:
            assert lo1 - lo0 <= E.CERT_GAP and hi1 - hi0 <= E.CERT_GAP and lo1 < hi0, case
        # both children of a stored split together hold the root's minimum
        for a, b in ((2, 3), (4, 5)):
            assert abs(min(e["m_up"][a], e["m_up"][b]) - e["m_up"][0]) <= 2 * E.slack(e["m_up"][0]), (case, a, b)
        signs.setdefault((e["network"], float(e["eps"])), set()).add(float(np.sign(e["m_up"][0])))
        assert np.sign(e["m_up"][0]) == np.sign(e["m_lo"][0])
    assert all(s == {-1.0, 1.0} for s in signs.values()), signs
    assert {n for n, _ in signs} == {n for n, _, _ in E.NETWORKS}


def rederive(case, k):
    e, lp = FIX[case], lp_of(case)
    info = {}
    m_lo, m_up, x = E.exact_min(lp, E.split_mask(lp, e["masks"][k]), info=info)
    print(f"{case} {E.DOMAINS[k]}: status {info['status']} binaries {info['binaries']} {info['seconds']:.1f} s m_lo {m_lo} m_up {m_up}")
    assert info["status"] == int(e["status"][k])
    if m_lo is None:
        return
    assert m_up - m_lo <= E.CERT_GAP
    # two certified brackets of one number overlap
    assert m_lo <= e["m_up"][k] + E.slack(m_lo) and e["m_lo"][k] <= m_up + E.slack(m_up), (m_lo, m_up, e["m_lo"][k], e["m_up"][k])
    assert bool((x >= lp.input_lb).all()) and bool((x <= lp.input_ub).all())


@pytest.mark.parametrize("k", range(len(E.DOMAINS)))
@pytest.mark.parametrize("case", QUICK)
def test_the_fixture_derives_again(case, k):
    rederive(case, k)


@pytest.mark.slow
@pytest.mark.parametrize("k", range(len(E.DOMAINS)))
@pytest.mark.parametrize("case", [c for c in CASES if c not in QUICK])
def test_the_fixture_derives_again_long_form(case, k):
    rederive(case, k)


@pytest.mark.parametrize("case", QUICK)
def test_node_extrema_derive_again(case):
    e, lp = FIX[case], lp_of(case)
    for node, (lo0, lo1, hi0, hi1) in zip(e["nodes"], e["node_extrema"]):
        lo, hi, st = E.exact_node_extrema(lp, int(e["node_layer"]), int(node))
        assert st == [0, 0] and abs(lo[1] - lo1) <= 2 * E.CERT_GAP and abs(hi[0] - hi0) <= 2 * E.CERT_GAP, (case, node, lo, hi)


@pytest.mark.parametrize("case", CASES)
def test_host_dual_below_lp_below_exact(case):
    """On every stored domain, in this order: dual_ascent_host (0, 20, 100 iterations) <= HiGHS LP optimum + 1e-6 <= m_up + slack; the
    infeasible domain's bounds cross."""
    e, lp = FIX[case], lp_of(case)
    for k in feasible(case):
        mask, parent, split = domain(case, k)
        bounds = lp.kw_bounds(mask, parent, split)
        sub = lp._solve_lp([m.clone() for m in mask], *bounds)
        assert sub is not None, (case, E.DOMAINS[k])
        duals = [lp.dual_ascent_host(bounds, mask, n).bound for n in (0, 20, 100)]
        print(f"{case} {E.DOMAINS[k]}: dual {duals} lp {sub.lb} exact [{e['m_lo'][k]}, {e['m_up'][k]}]")
        assert duals[0] <= duals[1] <= duals[2]
        assert duals[2] <= sub.lb + 1e-6, (case, E.DOMAINS[k], duals, sub.lb)
        assert sub.lb <= e["m_up"][k] + E.slack(e["m_up"][k]) + 1e-6, (case, E.DOMAINS[k], sub.lb, e["m_up"][k])
        if k == 0:
            assert abs(duals[1] - float(e["root20"])) <= 1e-12 * max(1.0, abs(duals[1])), (case, duals[1], e["root20"])
    mask, parent, split = domain(case, len(E.DOMAINS) - 1)
    bounds = lp.kw_bounds(mask, parent, split)
    assert lp._solve_lp([m.clone() for m in mask], *bounds) is None


@pytest.mark.parametrize("case", CASES)
def test_host_bounds_contain_the_minimiser_and_bracket_the_node_extrema(case):
    """The pre-activations at x_star lie inside the host Wong-Kolter bounds of the domain x_star minimises over (slack: the solver
    holds a split's sign constraint to its feasibility tolerance, 1e-6 at most, not exactly); the root's bounds of the stored nodes
    lie outside their exact extrema."""
    e, lp = FIX[case], lp_of(case)
    for k in feasible(case):
        mask, parent, split = domain(case, k)
        lbs, ubs = lp.kw_bounds(mask, parent, split)
        pre, out = E.pre_activations(lp, torch.from_numpy(e["x_star"][k]))
        assert abs(out - e["m_up"][k]) <= 1e-12 * max(1.0, abs(out))
        for r, i in enumerate(lp.pre_relu_indices):
            lo, up, p = lbs[i].reshape(-1), ubs[i].reshape(-1), pre[r]
            tol = 1e-6 * torch.maximum(torch.ones_like(p), p.abs())
            assert bool((p >= lo - tol).all()) and bool((p <= up + tol).all()), (case, E.DOMAINS[k], r)
        assert float(lbs[-1].reshape(-1)[0]) <= out + E.slack(out) and float(ubs[-1].reshape(-1)[0]) >= out - E.slack(out)
    lbs, ubs = root_bounds(case)
    i = lp.pre_relu_indices[int(e["node_layer"])]
    for node, (lo0, lo1, hi0, hi1) in zip(e["nodes"], e["node_extrema"]):
        lo, up = float(lbs[i].reshape(-1)[node]), float(ubs[i].reshape(-1)[node])
        assert lo <= lo1 + E.slack(lo1) and up >= hi0 - E.slack(hi0), (case, int(node), lo, up, lo1, hi0)


def kw_constants_agree(case):
    e, lp = FIX[case], lp_of(case)
    info = {}
    m_lo, m_up, _ = E.exact_min(lp, E.root_mask(lp), big_m="kw", info=info)
    print(f"{case}: Wong-Kolter constants: {info['binaries']} binaries, {info['seconds']:.1f} s, m_up {m_up}; interval constants m_up {e['m_up'][0]}")
    assert info["status"] == 0 and m_up - m_lo <= E.CERT_GAP
    assert abs(m_up - e["m_up"][0]) <= 1e-9, (case, m_up, e["m_up"][0])


@pytest.mark.parametrize("case", [c for c in CASES if c.startswith(("kwg_single@", "kwg_mlp@0.01"))])
def test_milp_with_wong_kolter_constants_gives_the_same_minimum(case):
    kw_constants_agree(case)


@pytest.mark.slow
@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith(("kwg_single@", "kwg_mlp@0.01"))])
def test_milp_with_wong_kolter_constants_gives_the_same_minimum_long_form(case):
    kw_constants_agree(case)


def test_the_yardstick_sees_an_exchanged_split_clamp():
    """The mutant: ``kw_bounds`` with the split clamp's two phases exchanged (a node split passing gets its upper bound clamped to 0, one
    split blocked its lower bound), everything else untouched.  The host bound on the mutant's intermediate bounds -- the HiGHS LP of
    ``_solve_lp``, the middle of the chain test_host_dual_below_lp_below_exact asserts -- exceeds m_up by more than 100 slacks on at
    least one stored child (the children of the fixture were chosen with their two bounds far apart), where the unmutated LP bound of
    the same child is at or below m_up: ``sub.lb <= m_up + slack`` catches the mutant.  A mutant LP that is infeasible throws a feasible
    child away and counts as caught too.

    Extras.  The 20-step ascent on the same mutated bounds is printed, not asserted: it reads a split's phase from the mask, so the
    clamp only moves the intermediate bounds of the layers above, and its bound stayed below m_up on all 40 stored children (closest:
    21.9 slacks below, kwg_deep8@0.002:3:5 first_blocked).  Containment sees the mutant as well: on at least one stored child the split
    node's pre-activation at x_star lies outside the mutant's bounds by more than 100 slacks.  And with the phases exchanged all the way
    through (the clamp and the reading of the mask) the ascent's bound exceeds m_up by more than 100 slacks on at least one child."""
    caught, outside, above = [], [], []
    for case, e in FIX.items():
        lp = lp_of(case)
        root = E.flat_mask(E.root_mask(lp))
        for k in (2, 3, 4, 5):
            mask, parent, split = domain(case, k)
            flat = int(np.nonzero(e["masks"][k] != root)[0][0])
            m_up, sl = float(e["m_up"][k]), E.slack(e["m_up"][k])
            good_lp = lp._solve_lp([m.clone() for m in mask], *lp.kw_bounds(mask, parent, split))
            clamp_only, bad_bounds = E.mutated_bound(lp, mask, parent, split)
            bad_lp = lp._solve_lp([m.clone() for m in mask], *bad_bounds)
            bad = float("inf") if bad_lp is None else bad_lp.lb
            through = E.exchanged_phase_bound(lp, mask, parent, split)
            pre, _ = E.pre_activations(lp, torch.from_numpy(e["x_star"][k]))
            p = float(torch.cat(pre)[flat])
            i = lp.pre_relu_indices[split]
            node = int(flat) - sum(int(np.prod(lp.shapes[j + 1])) for j in lp.pre_relu_indices[:split])
            lo, up = float(bad_bounds[0][i].reshape(-1)[node]), float(bad_bounds[1][i].reshape(-1)[node])
            out = max(lo - p, p - up) / E.slack(p)
            print(f"{case} {E.DOMAINS[k]}: exact {m_up:.9f}; LP {good_lp.lb:.9f}, on the exchanged clamp {bad:.9f} = {(bad - m_up) / sl:.1f} slacks above; "
                  f"20-step ascent on it {(clamp_only - m_up) / sl:.1f} slacks above; split node at x_star {p:.3e} outside [{lo:.3e}, {up:.3e}] by "
                  f"{out:.1f} slacks; phases exchanged throughout {(through - m_up) / sl:.1f} slacks above")
            assert good_lp is not None and good_lp.lb <= m_up + sl + 1e-6, (case, E.DOMAINS[k], good_lp.lb, m_up)
            if bad > m_up + 100 * sl:
                caught.append((case, E.DOMAINS[k], bad))
            if out > 100:
                outside.append((case, E.DOMAINS[k], out))
            if (through - m_up) / sl > 100:
                above.append((case, E.DOMAINS[k]))
    print(f"the LP on the exchanged clamp is more than 100 slacks above the exact minimum on {len(caught)} of {4 * len(FIX)} stored children")
    assert any(b != float("inf") for _, _, b in caught), "no stored child exposes the exchanged clamp by its LP bound"
    assert outside, "no stored child exposes the exchanged clamp by containment"
    assert above, "no stored child exposes the exchanged phases by its bound"
    assert E.lp_producer._clamp_by_mask.__name__ == "_clamp_by_mask"      # the mutation is gone


@pytest.mark.parametrize("case", QUICK)
def test_the_host_loop_decides_within_its_stored_branch_count(case):
    e, lp = FIX[case], lp_of(case)
    for db, n in zip((float(e["m_lo"][0] - e["d"]), 0.0), e["n_host"]):
        branches, reason, glb, gub = E.host_loop(lp, db)
        assert (branches if reason == "decision" else -1) == int(n), (case, db, branches, reason)
        if glb >= db:                                           # the host loop's verdicts are held to the truth as well
            assert e["m_up"][0] >= db - E.slack(db), (case, db, glb)
        if gub < db:
            assert e["m_lo"][0] < db, (case, db, gub)
