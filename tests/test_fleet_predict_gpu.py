"""Predicted fleet calls (mpc_episodes_fleet_run_predicted, k_episodes_run with
FleetMotionObs of csrc/mpc_episodes_fleet.h, through DeviceFleet(predict=True))
pinned to the host model, bit for bit.

The pattern is test_fleet_gpu.py's: every comparison is robots_model.compare on
the whole state tensor, every log ring and the progress records, plus, after
every run(), read_blocked(), the neighbour table, both sides of the pose board
and both sides of the motion board with `==`, against
tests/fleet_model.py's Fleet(predict=True).  Every case first asserts its preconditions on
that model — the margin between any state and any MOVING rim above
ranking.MARGIN, the margins at the reach and the cap, and what the case is
about — before any kernel is looked at.  The model also scores every step
under each wrong multiplier of the displacement (0, j - 1, j + 1, N, 1): the
ring matrix asserts that each of them would have given other counts and other
winners."""
import functools
import math

import numpy as np
import pytest

import fleet_model as FM
import robots_bench as RB
import robots_cases as RC
from diplomjourney_amd.abi import MPC_EP_ARRIVED, MPC_MAX_OBSTACLES, MPC_MAX_STEPS
from diplomjourney_amd.device_episodes import fleet_reach
from diplomjourney_amd.episode_config import tree_episode_config
from fleet_cases import (CROSSING, FLAG_CLEARANCE, FOLLOW_CLEARANCE, RING_CLEARANCE, SPLIT,
                         flagged_fleet, follow, long_crowd, parked, ring, robot)
from robots_bench import fleet_against as against

pytestmark = pytest.mark.gpu

DEVICE = True        # the model's reciprocal estimates: the GPU's
# the bench with the predicted entry (a call may still say predict=False)
device_run = functools.partial(RB.fleet_device_run, predict=True)
model = functools.partial(RB.fleet_model, predict=True)
check = functools.partial(RB.fleet_check, predict=True, name="predicted fleet")


def winners(F):
    """Per robot, per step: the model's winner."""
    return [[rec["index"] for rec in rr] for rr in F.recs]


# ----------------------------------------------------------------------------
# 1. the matrix: six robots on a ring
# ----------------------------------------------------------------------------
def ring_predicts(F):
    """The case tells the prediction from every wrong one: a rim cuts through
    a step's candidates, and under each wrong multiplier of the displacement
    some step's blocked count and some step's winner are others."""
    assert any(p[0] >= 1 for p in F.picks[0]), F.picks[0]
    assert any(0 < n < 451 for M in F.models for n in M.blocked_steps)
    won = winners(F)
    for name in FM.WRONG:
        counts = sum(w[0] != n for M in F.models for w, n in zip(M.wrong[name], M.blocked_steps))
        wins = sum(w[1] != i for M, ww in zip(F.models, won) for w, i in zip(M.wrong[name], ww))
        assert counts >= 1 and wins >= 1, (name, counts, wins)


@pytest.mark.parametrize("L", (0.5, 0.45))
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_ring_matrix(engine, integ, n_steps, L):
    """Ten predicted fleet calls as run(1) x 3 + run(2) + run(5) — odd and
    even call0, both boards' parity across entry calls — and as one run(10):
    the same bits, the model's."""
    cfgs = ring(L)
    F, got, per = check(engine, cfgs, n_steps, integ, RING_CLEARANCE, SPLIT,
                        precondition=ring_predicts, name=f"ring {integ} N={n_steps} L={L}")
    one, per1 = device_run(engine, cfgs, n_steps, integ, RING_CLEARANCE, None, (), (10,), 16)
    assert one == got
    against(F, cfgs, 16, (10,), one, per1, "ring, one run(10)")
    assert (per1[0].blocked == sum(p.blocked for p in per)).all()
    assert (per1[0].board, per1[0].motion) == (per[-1].board, per[-1].motion)


# ----------------------------------------------------------------------------
# 2. follow
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_follower_runs_behind_the_leader(engine, integ):
    """A follower behind a leader.  Standing circles stop it as stuck after two
    all-blocked calls (the leader's circle covers its whole horizon); under
    the prediction only call 0 is blocked and it runs all ten calls."""
    cfgs = follow()
    reach = fleet_reach(cfgs, 3, FOLLOW_CLEARANCE, predict=True)
    S = FM.Fleet(cfgs, 3, integ, FOLLOW_CLEARANCE, reach).run(10, device=DEVICE)
    assert S.models[0].calls == 2 and S.models[0].stop and S.models[0].blocked_steps == [451, 451]

    def follows(F):
        M = F.models[0]
        assert M.calls == 10 and not M.stop
        assert M.blocked_steps[0] == 451 and all(n < 451 for n in M.blocked_steps[1:])

    check(engine, cfgs, 3, integ, FOLLOW_CLEARANCE, (3, 7), precondition=follows,
          name=f"follow {integ}")


# ----------------------------------------------------------------------------
# 3. call 0 is the fleet call
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_call_0_is_the_fleet_call(engine, integ):
    """run(1) after reset() with predict=True and with predict=False (the same
    explicit reach): the same state, log, progress, blocked counts, neighbours
    and pose board; the motion board's side 0 zeroed, its side 1 the
    displacements."""
    cfgs = ring()
    reach = fleet_reach(cfgs, 3, RING_CLEARANCE, predict=True)
    a, pa = device_run(engine, cfgs, 3, integ, RING_CLEARANCE, reach, (), (1,), 16)
    b, pb = device_run(engine, cfgs, 3, integ, RING_CLEARANCE, reach, (), (1,), 16,
                       predict=False)
    assert a == b
    assert (pa[0].blocked == pb[0].blocked).all()
    assert (pa[0].neighbours == pb[0].neighbours).all() and pa[0].board == pb[0].board
    board = np.frombuffer(pa[0].board, dtype=np.float64).reshape(2, 6, 2)
    motion = np.frombuffer(pa[0].motion, dtype=np.float64).reshape(2, 6, 2)
    assert (motion[0] == 0.0).all() and (motion[1] == board[1] - board[0]).all()
    assert (motion[1] != 0.0).any(axis=1).all()


# ----------------------------------------------------------------------------
# 4. parked neighbours
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_parked_neighbours_equal_the_fleet_call(engine, integ):
    """One moving robot among parked ones and a static circle: every motion
    entry a block reads is zero, so eight run(1) equal predict=False bit for
    bit (the robot steers around what is in its way: circles are tested)."""
    cfgs = [robot((0.0, 0.0), (0.6, 0.0)), parked((0.3, 0.03)), parked((0.18, -0.05)),
            parked((0.45, 0.04))]
    static = ((0.1, 0.06, 0.0313),)
    reach = fleet_reach(cfgs, 3, 0.0413, predict=True)
    F = model(cfgs, 3, integ, 0.0413, reach, static, 8)
    assert sum(F.models[0].blocked_steps) > 0 and F.models[0].calls == 8
    assert all(m == (0.0, 0.0) for mot in F.motions for m in mot[1:])
    a, pa = device_run(engine, cfgs, 3, integ, 0.0413, reach, static, (1,) * 8, 16)
    b, pb = device_run(engine, cfgs, 3, integ, 0.0413, reach, static, (1,) * 8, 16,
                       predict=False)
    assert a == b
    for x, y in zip(pa, pb):
        assert (x.blocked == y.blocked).all() and (x.neighbours == y.neighbours).all()
        assert x.board == y.board
    against(F, cfgs, 16, (1,) * 8, a, pa, f"parked {integ}")


# ----------------------------------------------------------------------------
# 5. ended robots publish zero
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_ended_robots_publish_zero(engine, integ):
    """test_fleet_gpu's four robots: from the call in which robot 2 arrives its
    motion entry is (0, 0), on both sides one call later, and robot 3 is blocked
    by its standing circle; robot 0, never started, publishes zero throughout.
    The motion board is compared after every run(1)."""
    cfgs = [parked((0.3, 0.03)), robot((0.0, 0.0), (0.6, 0.0)),
            robot((0.0, 0.4), (0.07, 0.4)), robot((-0.3, 0.42), (0.6, 0.4))]

    def stay(F):
        M0, M1, M2, M3 = F.models
        assert M0.calls == 0 and M0.stop == MPC_EP_ARRIVED
        assert M2.stop & MPC_EP_ARRIVED and 2 <= M2.calls and F.calls >= M2.calls + 3
        assert all(mot[0] == (0.0, 0.0) for mot in F.motions)
        assert all(F.motions[c][2] != (0.0, 0.0) for c in range(1, M2.calls))
        assert all(F.motions[c][2] == (0.0, 0.0) for c in range(M2.calls, F.calls + 1))
        assert F.boards[M2.calls][2] != F.boards[M2.calls - 1][2]     # (it moved in that call)
        assert sum(M3.blocked_steps[M2.calls:]) > 0, "robot 2 blocks nothing once it has arrived"
        both = np.frombuffer(F.motion(M2.calls + 1), dtype=np.float64).reshape(2, 4, 2)
        assert (both[:, 2] == 0.0).all()

    check(engine, cfgs, 3, integ, 0.0413, (1,) * 12, precondition=stay, name=f"ended {integ}")


# ----------------------------------------------------------------------------
# 6. flagged candidates
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_flagged_candidates_meet_the_moved_circle(engine, integ, n_steps):
    """A flagged candidate (|beta| = 1.2 > kTanMax: its states are the
    recompute's) is blocked by the moving neighbour's step-j circle, j >= 2,
    and by neither the standing circle nor the one of step j - 1: the safe
    recompute tests each state against its own step's world table."""
    cfgs, k = flagged_fleet(integ, n_steps, device=DEVICE)

    def flagged(F):
        M = F.models[0]
        found = []
        for c in range(1, M.calls):
            if 2 not in (F.picks[c][0] or (0, []))[1]:
                continue
            i = len(F.static) + F.picks[c][0][1].index(2)
            for kk in np.flatnonzero(np.abs(M.betas[c]) > RC.K_TAN_MAX):
                late = M.hits[c][1:, i, kk].any()
                if late and not M.wrong["0"][c][2][kk] and not M.wrong["j-1"][c][2][kk]:
                    found.append((c, int(kk)))
        assert found, "no flagged candidate is blocked by a moved circle alone"
        assert F.motions[found[0][0]][2] != (0.0, 0.0)
        assert not any(m.all() for m, _ in M.masks)

    check(engine, cfgs, n_steps, integ, FLAG_CLEARANCE, (2, 2), cap=8, precondition=flagged,
          name=f"flagged {integ} N={n_steps}")


# ----------------------------------------------------------------------------
# 7. the longest horizon: the tables' second pass
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_longest_horizon_fills_the_tables_in_two_passes(engine, integ):
    """n_steps = MPC_MAX_STEPS and a full table: 32 x 16 = 512 entries, formed
    by 256 threads in two passes.  Some candidate is blocked only by entries
    of the second pass ((j - 1) * 16 + i >= 256: steps 17..32)."""
    cfgs = long_crowd()
    n = MPC_MAX_STEPS

    def second_pass(F):
        assert all(p is not None and len(p[1]) == MPC_MAX_OBSTACLES for row in F.picks for p in row)
        late = [(r, c, int(k)) for r, M in enumerate(F.models) for c in range(1, M.calls)
                for k in np.flatnonzero(M.hits[c][16:].any(axis=(0, 1))
                                        & ~M.hits[c][:16].any(axis=(0, 1)))]
        assert late, "no candidate is blocked by the second pass's entries alone"
        assert any(m != (0.0, 0.0) for m in F.motions[1])

    check(engine, cfgs, n, integ, 0.0113, (1, 2), cap=4, precondition=second_pass,
          name=f"long horizon {integ}")


# ----------------------------------------------------------------------------
# 8. reach
# ----------------------------------------------------------------------------
def test_reach_beyond_two_horizons_changes_nothing(engine):
    """Two fast robots head-on.  reach=None (two horizons' travel plus
    clearance) and twice that: the same bytes.  On the model alone: with the unpredicted fleet_reach some
    neighbour that blocks a candidate is out of reach."""
    cfgs = [robot((0.0, 0.0), (0.9, 0.0), v=1.0), robot((0.9, 0.004), (0.0, 0.004), v=1.0)]
    reach = fleet_reach(cfgs, 3, FOLLOW_CLEARANCE, predict=True)
    F = model(cfgs, 3, "qk21", FOLLOW_CLEARANCE, None, (), 10)
    F2 = model(cfgs, 3, "qk21", FOLLOW_CLEARANCE, 2 * reach, (), 10)
    short = fleet_reach(cfgs, 3, FOLLOW_CLEARANCE)
    blockers = [math.sqrt(FM.d2_row(F.boards[c], r)[q])
                for r, M in enumerate(F.models) for c in range(M.calls)
                for i, q in enumerate(F.picks[c][r][1]) if M.hits[c][:, i, :].any()]
    assert blockers and max(blockers) >= short, (max(blockers, default=None), short)
    a, pa = device_run(engine, cfgs, 3, "qk21", FOLLOW_CLEARANCE, None, (), (10,), 16)
    b, pb = device_run(engine, cfgs, 3, "qk21", FOLLOW_CLEARANCE, 2 * reach, (), (10,), 16)
    assert a == b and (pa[0].board, pa[0].motion) == (pb[0].board, pb[0].motion)
    assert (pa[0].blocked == pb[0].blocked).all()
    against(F, cfgs, 16, (10,), a, pa, "reach")
    against(F2, cfgs, 16, (10,), b, pb, "twice the reach")


# ----------------------------------------------------------------------------
# 9. the driver
# ----------------------------------------------------------------------------
def test_run_tree_fleet_predicts(engine):
    """run_tree_fleet(predict=True) with test_fleet_gpu's crossing: the model's
    records, stop names and stats over host calls of eight fleet calls; it
    differs from predict=False, which is what it was."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import run_math_model as rmm
    mmt.reset_state()
    cfgs = [tree_episode_config(s, 24) for s in CROSSING]
    F = model(cfgs, 3, "qk21", 0.0513, None, (), 24)
    assert sum(sum(M.blocked_steps) for M in F.models) > 0 and all(M.stop for M in F.models)
    stats = {}
    got = rmm.run_tree_fleet(CROSSING, 0.0513, max_calls=24, engine=engine, stats=stats, chunk=8,
                             predict=True)
    for r, (records, stop) in enumerate(got):
        assert stop == rmm._stop_name(F.models[r].stop), r
        assert records == [[q[k] for k in ("x", "y", "phi", "v", "beta")] for q in F.recs[r]], r
    assert stats["steps"] == max(M.calls for M in F.models)
    assert stats["candidates"] == sum(M.candidates for M in F.models)
    assert stats["blocked"] == sum(sum(M.blocked_steps) for M in F.models)
    S = model(cfgs, 3, "qk21", 0.0513, None, (), 24, predict=False)
    standing = rmm.run_tree_fleet(CROSSING, 0.0513, max_calls=24, engine=engine, chunk=8)
    for r, (records, stop) in enumerate(standing):
        assert stop == rmm._stop_name(S.models[r].stop), r
        assert records == [[q[k] for k in ("x", "y", "phi", "v", "beta")] for q in S.recs[r]], r
    assert standing != got
