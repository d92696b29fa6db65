"""-m gpu: frontier runs that learn with repack="device" (DESIGN.md section 7.15): the learning step is only issued, its status word and
what a traced round shows of it are read with the next round's state record.  toy_kw with the settings of tests/test_gpu_imitation.py's
frontier case (and tests/test_gpu_frontier_online.py's for the online form); the host twins run on an engine in repack mode 1."""
import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib
from tests import frontier_twin
from tests import test_gpu_frontier_online as tfo
from tests import test_gpu_imitation as tgi
from tests.test_online_gradients import bits

pytestmark = pytest.mark.gpu
ROUNDS = 4


@pytest.fixture()
def twins_on_device_mode(monkeypatch):
    """The host twins make their own GraphChoice through tests.frontier_twin.toy: every online one gets an engine in repack mode 1."""
    toy = frontier_twin.toy

    def toy_mode_1(*a, **kw):
        lp, choice, mask = toy(*a, **kw)
        if kw.get("online"):
            choice._eng().set_repack("device")
        return lp, choice, mask
    monkeypatch.setattr(frontier_twin, "toy", toy_mode_1)
    monkeypatch.setattr(tfo, "toy", toy_mode_1)


# ---- 1. equivalence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_the_device_mode_run_equals_the_host_loop_on_a_mode_1_engine(K, twins_on_device_mode):
    from gnn_branching_amd.engine import state_blob
    from tests.frontier_twin import masked
    branching = "gnn"
    (glb, gub, rounds, bounded, reason), trace, audit, stats, choice = tgi.frontier_run(K, 1, branching, rounds=ROUNDS, repack="device")
    assert choice._eng().repack_mode == "host"              # the run puts the engine's mode back
    rows, tables = iter(audit), []
    for t in trace:
        tables.append([next(rows) for _ in t["slots"]])
    host = tgi.host_loop(K, ROUNDS, 1, branching, tables, tgi.FR_MARGIN[branching])
    first = next((r for r, l in enumerate(host["loss"]) if l), None)
    assert first is not None and first + 1 < len(host["decisions"]), "the host loop never decided after a step"
    assert any(v > 0 for l in host["loss"] for v in l), "no step of the host loop carried a gradient"
    assert len(trace) == len(host["decisions"]) >= 2
    assert [t["decisions"] for t in trace] == host["decisions"]
    assert [masked(t["child_bounds"], t["infeasible"], t["live"]) for t in trace] == host["child_bounds"]
    for r, t in enumerate(trace):
        assert "imitation_loss" in t, r                      # (every round learns; the last round's entries came at the end of the run)
        assert t["global_lb"] == host["global_lb"][r] and abs(t["global_ub"] - host["global_ub"][r]) <= 1e-9 * max(1.0, abs(host["global_ub"][r]))
        np.testing.assert_array_equal(bits(t["imitation_loss"]), bits(host["loss"][r]))
        assert t["imitation_report"] == host["report"][r] and tgi.same_or_nan(t["imitation_regret"], host["regret"][r])
    assert glb == host["global_lb"][-1]
    assert stats["imitation_steps"] == host["steps"] == len(trace) and stats["imitation_rows"] == host["rows"]
    got_w = choice._eng().get_weights()
    np.testing.assert_array_equal(bits(got_w), bits(host["weights"]))
    assert (bits(host["weights"]) != bits(host["weights_start"])).any()
    np.testing.assert_array_equal(bits(state_blob(choice.model.state_dict())), bits(got_w))


# ---- 2. a learning round under the sync-debug mode --------------------------------------------------------------------------------------
def test_a_device_mode_learning_round_waits_for_nothing_but_its_reads():
    """One learning round under torch.cuda.set_sync_debug_mode("error") with the exemptions the strong-branching test has -- the read of
    cand0[K] and the read of the state record; the status word of the step is not read in its round."""
    from gnn_branching_amd.frontier import FrontierRun
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in the installed torch")
    lp, choice, _ = toy(online=True)
    run = FrontierRun(lp, choice, lp.layers, K=2, n_iter=N_ITER, lr=LR, eps=EPS_BAB, imitate=1, strong_candidates=tgi.FR_CANDIDATES, strong_chunk=3,
                      branching="gnn", repack="device")
    try:
        st = run.root()
        if not tfo.sync_mode_is_live(run):
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a synchronising copy in the installed torch")
        before = torch.cuda.get_sync_debug_mode()
        w0 = run.eng.get_weights().copy()
        reads, read_candidates = [], run.read_candidates

        def exempt_read(n):
            with pytest.raises(RuntimeError):
                read_candidates(n)
            torch.cuda.set_sync_debug_mode(before)
            try:
                reads.append(read_candidates(n))
            finally:
                torch.cuda.set_sync_debug_mode("error")
            return reads[-1]
        run.read_candidates = exempt_read
        try:
            torch.cuda.set_sync_debug_mode("error")
            run.launch_round(1, int(st[_lib.FS_IN_USE]))
            with pytest.raises(RuntimeError):
                run.read_state()                              # the state record: a synchronising copy
            torch.cuda.set_sync_debug_mode(before)
            st = run.pool.state.cpu().tolist()                # ... exempted by hand
            assert run.imitate_pending and run.learning and run.pending_step is None
            torch.cuda.set_sync_debug_mode("error")
            run._settle_step()                                # nothing is pending in the first round: no read
            run._imitate()                                    # the step and the pack build are issued; nothing is read back
            assert run.pending_step is not None and run.pending_step["round"] == 1
            torch.cuda.set_sync_debug_mode(before)
        finally:
            torch.cuda.set_sync_debug_mode(before)
        assert reads == [tgi.FR_CANDIDATES] and run.imitation_steps == 1 and not run.imitate_pending
        run.check_status()                                    # the end of the run: the step's status word is read now
        assert run.pending_step is None
        assert (bits(run.eng.get_weights()) != bits(w0)).any()
    finally:
        run.close()


# ---- 3. a refusal is raised one round late and names its round ---------------------------------------------------------------------------
def test_a_refused_row_raises_with_the_next_state_record_and_names_the_round_that_learnt():
    from gnn_branching_amd.frontier import FrontierRun
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy
    lp, choice, _ = toy(online=True)
    run = FrontierRun(lp, choice, lp.layers, K=1, n_iter=N_ITER, lr=LR, eps=EPS_BAB, imitate=1, strong_candidates=tgi.FR_CANDIDATES, branching="gnn",
                      repack="device")
    try:
        st = run.root()
        run.launch_round(1, int(st[_lib.FS_IN_USE]))
        decided = (run.P.amb[0] == 0).nonzero().view(-1)
        assert decided.numel() > 0, "toy_kw's root has no decided node: the test cannot name one"
        run.im_table[0, int(decided[0])] = 0.5                # the table names a decided node: the step refuses the row
        st = run.read_state()                                 # round 1's step is issued; nothing is raised in its round
        assert run.pending_step["round"] == 1 and run.imitation_steps == 1
        run.launch_round(1, int(st[_lib.FS_IN_USE]))
        with pytest.raises(RuntimeError, match=r"gnnb_imitation_step_rows refused a row \(status bit 3\).*learning step of round 1$"):
            run.read_state()
        assert run.round == 2 and run.pending_step is None
    finally:
        run.close()


# ---- 4. the online form -----------------------------------------------------------------------------------------------------------------
def test_the_online_run_in_device_mode_equals_its_twin(twins_on_device_mode):
    from gnn_branching_amd.frontier import branch_and_bound_frontier
    from tests.frontier_twin import EPS_BAB, LR, N_ITER, toy, twin
    K, rounds = 4, tfo.ROUNDS_K4
    want = twin(K, rounds, 1.0, online_threshold=1)
    lp, choice, _ = toy(online=True)
    trace, stats = [], {}
    res = branch_and_bound_frontier(lp, choice, lp.layers, K=K, n_iter=N_ITER, lr=LR, eps=EPS_BAB, max_rounds=rounds, log=lambda s: None, trace=trace,
                                    branching_threshold=1.0, stats=stats, online_threshold=1, repack="device")
    assert choice._eng().repack_mode == "host"
    tfo.assert_same_run(want, (res, trace, stats, choice))


# ---- 5. a bad argument ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["gpu", "", None, 1])
def test_a_bad_repack_raises_before_a_device_is_touched(bad):
    from gnn_branching_amd.frontier import FrontierRun, branch_and_bound_frontier

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the run touched its arguments ({name}) before it checked repack")
    with pytest.raises(ValueError, match="^repack = "):
        branch_and_bound_frontier(Untouchable(), Untouchable(), [], repack=bad)
    with pytest.raises(ValueError, match="^repack = "):      # the run class behind it
        FrontierRun(Untouchable(), Untouchable(), [], K=4, repack=bad)
