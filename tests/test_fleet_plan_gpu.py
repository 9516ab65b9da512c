"""Planned fleet calls (mpc_episodes_fleet_run_planned, k_episodes_run with
FleetPlanObs of csrc/mpc_episodes_fleet.h, through DeviceFleet(predict="plan"))
pinned to the host model, bit for bit.

The pattern is test_fleet_predict_gpu.py's: every comparison is
robots_model.compare on the whole state tensor, every log ring and the progress
records, plus, after every run(), read_blocked(), the neighbour table, both
sides of the pose board and both sides of the plan board with `==`, against
tests/fleet_plan_model.py's PlanFleet.  Every case first asserts its
preconditions on that model (tests/fleet_plan_cases.py) — the margin between
any state and any PLANNED rim above ranking.MARGIN, the margins at the reach
and the cap (fleet_plan_bench.model), and what the case is about — before any
kernel is looked at.  The model also scores every step under each wrong rule
(standing circles, the constant displacement, the plan one layer early, a2 held
for j >= 3, the multipliers j - 1 and j - 3, ot published by robots that
stand): the ring matrix asserts that each would have given other counts and
other winners."""
import math

import numpy as np
import pytest

import fleet_model as FM
import fleet_plan_bench as PB
import fleet_plan_cases as PC
import robots_cases as RC
from diplomjourney_amd.abi import MPC_MAX_STEPS
from diplomjourney_amd.device_episodes import fleet_reach
from diplomjourney_amd.episode_config import tree_episode_config
from fleet_cases import FOLLOW_CLEARANCE, RING_CLEARANCE, SPLIT, follow, long_crowd, ring, robot

pytestmark = pytest.mark.gpu

DEVICE = True        # the model's reciprocal estimates: the GPU's


# ----------------------------------------------------------------------------
# 1. the matrix: six robots on a ring
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("L", (0.5, 0.45))
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_ring_matrix(engine, integ, n_steps, L):
    """Ten planned fleet calls as run(1) x 3 + run(2) + run(5) — odd and even
    call0, both boards' parity across entry calls — and as one run(10): the
    same bits, the model's."""
    cfgs = ring(L)
    F, got, per = PB.check(engine, cfgs, n_steps, integ, RING_CLEARANCE, SPLIT,
                           precondition=PC.ring_plans, name=f"ring {integ} N={n_steps} L={L}")
    one, per1 = PB.device_run(engine, cfgs, n_steps, integ, RING_CLEARANCE, None, (), (10,), 16)
    assert one == got
    PB.against(F, cfgs, 16, (10,), one, per1, "ring, one run(10)")
    assert (per1[0].blocked == sum(p.blocked for p in per)).all()
    assert (per1[0].board, per1[0].plan) == (per[-1].board, per[-1].plan)


# ----------------------------------------------------------------------------
# 2. a turning leader
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_turning_leader(engine, integ):
    """The leader's heading is off its target line: its plan is an arc, and the
    second robot's candidates are cut by the rim.  The planned run differs from
    the constant displacement's and from the standing circles'."""
    cfgs, clearance, n_calls = PC.turning()
    reach = fleet_reach(cfgs, 3, clearance, predict=True)
    PB.check(engine, cfgs, 3, integ, clearance, (3, n_calls - 3), reach=reach,
             precondition=lambda F: PC.turns(F, cfgs, integ, clearance, reach, n_calls, DEVICE),
             name=f"turning {integ}")


# ----------------------------------------------------------------------------
# 3. call 0 is the fleet call
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_call_0_is_the_fleet_call(engine, integ):
    """run(1) after reset() with predict="plan" and with predict=False (the
    same explicit reach): the same state, log, progress, blocked counts,
    neighbours and pose board; the plan board's side 0 is (x, y, x, y) of the
    pose board's side 0, bit for bit, and side 1 the robots' plans."""
    cfgs = ring()
    reach = fleet_reach(cfgs, 3, RING_CLEARANCE, predict=True)
    a, pa = PB.device_run(engine, cfgs, 3, integ, RING_CLEARANCE, reach, (), (1,), 16)
    b, pb = PB.device_run(engine, cfgs, 3, integ, RING_CLEARANCE, reach, (), (1,), 16,
                          predict=False)
    assert a == b
    assert (pa[0].blocked == pb[0].blocked).all()
    assert (pa[0].neighbours == pb[0].neighbours).all() and pa[0].board == pb[0].board
    board = np.frombuffer(pa[0].board, dtype=np.uint64).reshape(2, 6, 2)
    plan = np.frombuffer(pa[0].plan, dtype=np.uint64).reshape(2, 6, 4)
    assert (plan[0, :, 0:2] == board[0]).all() and (plan[0, :, 2:4] == board[0]).all()
    moved = np.frombuffer(pa[0].plan, dtype=np.float64).reshape(2, 6, 4)[1]
    assert (moved[:, 0:2] != moved[:, 2:4]).any(axis=1).all()
    assert (plan[1, :, 0:2] != board[1]).any(axis=1).all()


# ----------------------------------------------------------------------------
# 4. parked neighbours
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_parked_neighbours_equal_the_fleet_call(engine, integ):
    """One moving robot among parked ones and a static circle: every plan entry
    a block reads is a position twice, so eight run(1) equal predict=False bit
    for bit."""
    cfgs, static, cl = PC.PARKED, PC.PARKED_STATIC, PC.PARKED_CLEARANCE
    reach = fleet_reach(cfgs, 3, cl, predict=True)
    F = PB.model(cfgs, 3, integ, cl, reach, static, 8)
    PC.parked_stand(F)
    a, pa = PB.device_run(engine, cfgs, 3, integ, cl, reach, static, (1,) * 8, 16)
    b, pb = PB.device_run(engine, cfgs, 3, integ, cl, reach, static, (1,) * 8, 16, predict=False)
    assert a == b
    for x, y in zip(pa, pb):
        assert (x.blocked == y.blocked).all() and (x.neighbours == y.neighbours).all()
        assert x.board == y.board
    PB.against(F, cfgs, 16, (1,) * 8, a, pa, f"parked {integ}")


# ----------------------------------------------------------------------------
# 5. a finishing neighbour
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_finishing_neighbour(engine, integ):
    """Robot 0 returns the layers 1 and 2 of its plan (m = 1, 2) and arrives:
    its entry is (ot[2], ot[2]) after the call that returned layer 1 and its
    position twice from the call it arrives in (the one that returns layer 2),
    on both sides one call later; robot 1 reads every one of them and is then
    blocked by its standing circle.  The plan board is compared after every
    run(1)."""
    cfgs, clearance, n_calls = PC.finishing()
    PB.check(engine, cfgs, 3, integ, clearance, (1,) * n_calls, precondition=PC.finishes,
             name=f"finishing {integ}")


# ----------------------------------------------------------------------------
# 6. a stale neighbour
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_stale_neighbour_stands(engine, integ):
    """fleet_cases.follow(): the follower's call 0 is all blocked, as under
    standing circles; it publishes its position twice and the leader reads it."""
    PB.check(engine, follow(), 3, integ, FOLLOW_CLEARANCE, (1, 2, 7), precondition=PC.stale_stands,
             name=f"stale {integ}")


# ----------------------------------------------------------------------------
# 7. flagged candidates
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_flagged_candidates_meet_the_planned_circle(engine, integ, n_steps):
    """A flagged candidate (|beta| = 1.2 > kTanMax: its states are the
    recompute's) is blocked by the neighbour's planned step-j circle, j >= 2,
    and by neither the standing circle nor the constant-displacement one: the
    safe recompute tests each state against its own step's world table."""
    cfgs, clearance = PC.flagged_plan_fleet(integ, n_steps, device=DEVICE)
    PB.check(engine, cfgs, n_steps, integ, clearance, (2, 2), cap=8, precondition=PC.flagged,
             name=f"flagged {integ} N={n_steps}")


# ----------------------------------------------------------------------------
# 8. the longest horizon: the tables' second pass
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_longest_horizon_fills_the_tables_in_two_passes(engine, integ):
    """n_steps = MPC_MAX_STEPS and a full table: 32 x 16 = 512 entries, formed
    by 256 threads in two passes; some candidate is blocked only by entries of
    steps 17..32, the extrapolated centres."""
    PB.check(engine, long_crowd(), MPC_MAX_STEPS, integ, 0.0113, (1, 2), cap=4,
             precondition=PC.second_pass, name=f"long horizon {integ}")


# ----------------------------------------------------------------------------
# 9. reach
# ----------------------------------------------------------------------------
def test_reach_beyond_two_horizons_changes_nothing(engine):
    """Two fast robots head-on.  reach=None (two horizons' travel plus
    clearance) and twice that: the same bytes.  On the model alone: with the
    unpredicted fleet_reach some neighbour that blocks a candidate is out of
    reach."""
    cfgs = [robot((0.0, 0.0), (0.9, 0.0), v=1.0), robot((0.9, 0.004), (0.0, 0.004), v=1.0)]
    reach = fleet_reach(cfgs, 3, FOLLOW_CLEARANCE, predict=True)
    F = PB.model(cfgs, 3, "qk21", FOLLOW_CLEARANCE, None, (), 10)
    F2 = PB.model(cfgs, 3, "qk21", FOLLOW_CLEARANCE, 2 * reach, (), 10)
    short = fleet_reach(cfgs, 3, FOLLOW_CLEARANCE)
    blockers = [math.sqrt(FM.d2_row(F.boards[c], r)[q])
                for r, M in enumerate(F.models) for c in range(M.calls)
                for i, q in enumerate(F.picks[c][r][1]) if M.hits[c][:, i, :].any()]
    assert blockers and max(blockers) >= short, (max(blockers, default=None), short)
    a, pa = PB.device_run(engine, cfgs, 3, "qk21", FOLLOW_CLEARANCE, None, (), (10,), 16)
    b, pb = PB.device_run(engine, cfgs, 3, "qk21", FOLLOW_CLEARANCE, 2 * reach, (), (10,), 16)
    assert a == b and (pa[0].board, pa[0].plan) == (pb[0].board, pb[0].plan)
    assert (pa[0].blocked == pb[0].blocked).all()
    PB.against(F, cfgs, 16, (10,), a, pa, "reach")
    PB.against(F2, cfgs, 16, (10,), b, pb, "twice the reach")


# ----------------------------------------------------------------------------
# 10. the driver
# ----------------------------------------------------------------------------
def test_run_tree_fleet_plans(engine):
    """run_tree_fleet(predict="plan") with the crossing, every heading turned
    (fleet_plan_cases.CROSSING_TURNED: headed straight at their targets the
    robots' plans are their displacements' lines): the model's records, stop
    names and stats over host calls of eight fleet calls; it differs from
    predict=True and from predict=False."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import run_math_model as rmm
    mmt.reset_state()
    kw, starts = PC.CROSSING_RUN, PC.CROSSING_TURNED
    cfgs = [tree_episode_config(s, kw["max_calls"]) for s in starts]
    F = PB.model(cfgs, 3, "qk21", kw["clearance"], None, kw["obstacles"], kw["max_calls"])
    PC.crossing_differs(F, cfgs, DEVICE)
    stats = {}
    got = rmm.run_tree_fleet(starts, engine=engine, stats=stats, chunk=8, predict="plan", **kw)
    for r, (records, stop) in enumerate(got):
        assert stop == rmm._stop_name(F.models[r].stop), r
        assert records == [[q[k] for k in ("x", "y", "phi", "v", "beta")] for q in F.recs[r]], r
    assert stats["steps"] == max(M.calls for M in F.models)
    assert stats["candidates"] == sum(M.candidates for M in F.models)
    assert stats["blocked"] == sum(sum(M.blocked_steps) for M in F.models)
    moved = rmm.run_tree_fleet(starts, engine=engine, chunk=8, predict=True, **kw)
    standing = rmm.run_tree_fleet(starts, engine=engine, chunk=8, **kw)
    assert moved != got and standing != got
