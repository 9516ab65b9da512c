"""Robots as each other's keep-out circles (mpc_episodes_fleet_begin / _run,
k_episodes_run with the fleet hook of csrc/mpc_episodes_fleet.h, through
DeviceFleet) pinned to the host model, bit for bit.

Every comparison is robots_model.compare on the whole state tensor, every log
ring and the progress records — `==` on the bits — plus, after every run(),
read_blocked(), the neighbour table and both sides of the pose board against
tests/fleet_model.py: R ObstacleRobotModels in lockstep, each call's circles
chosen by the header's rule from the host build of the device's own distance
function.  Every case first asserts its preconditions on that model — the
margin between any state and any rim above ranking.MARGIN, the margin between
any distance and the reach, the gap at a capped selection's boundary — before
any kernel is looked at; the exact-tie case says where it does not.  The
robots have the reference's 11 x 41 grid unless a case says otherwise."""
import numpy as np
import pytest

import fleet_model as FM
import robots_bench as RB
import robots_cases as RC
import robots_model as RM
import robots_obstacle_cases as OC
import robots_obstacle_model as OM
from diplomjourney_amd.abi import MPC_EP_ARRIVED
from diplomjourney_amd.device_episodes import DeviceEpisodes, DeviceFleet, fleet_reach
from diplomjourney_amd.episode_config import tree_episode_config
from fleet_cases import (CROSSING, CROWD_STATIC, LATTICE, NEAR, RING_CLEARANCE, SPLIT, cloud_20,
                         cloud_520, crowd, parked, ring, robot)
from ranking import MARGIN
from robots_bench import (fleet_against as against, fleet_check as check,
                          fleet_device_run as device_run, fleet_model as model)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------
# 1. the matrix: six robots on a ring
# ----------------------------------------------------------------------------
def ring_interacts(F):
    assert any(p[0] >= 1 for p in F.picks[0]), F.picks[0]
    assert sum(sum(M.blocked_steps) for M in F.models) > 0
    assert any(f >= 0 and M.masks[s][0][f] for M in F.models for s, f in enumerate(M.free))
    if F.models[0].n_steps == 3:     # (the longer horizon's steps are all blocked or free)
        assert any(0 < n < 451 for M in F.models for n in M.blocked_steps)


@pytest.mark.parametrize("L", (0.5, 0.45))
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_ring_matrix(engine, integ, n_steps, L):
    """Ten fleet calls as run(1) x 3 + run(2) + run(5) — odd and even call0,
    the board's parity across entry calls — and as one run(10): the same bits,
    the model's."""
    cfgs = ring(L)
    F, got, per = check(engine, cfgs, n_steps, integ, RING_CLEARANCE, SPLIT,
                        precondition=ring_interacts, name=f"ring {integ} N={n_steps} L={L}")
    one, per1 = device_run(engine, cfgs, n_steps, integ, RING_CLEARANCE, None, (), (10,), 16)
    assert one == got
    against(F, cfgs, 16, (10,), one, per1, "ring, one run(10)")
    assert (per1[0].blocked == sum(p.blocked for p in per)).all()


def test_reach_beyond_the_horizon_changes_nothing(engine):
    """reach=None (the horizon's length plus clearance) and twice that: the
    same logs — a robot farther away cannot matter."""
    cfgs = ring()
    reach = fleet_reach(cfgs, 3, RING_CLEARANCE)
    F = model(cfgs, 3, "qk21", RING_CLEARANCE, None, (), 10)
    F2 = model(cfgs, 3, "qk21", RING_CLEARANCE, 2 * reach, (), 10)
    assert any(a != b for a, b in zip(F.picks, F2.picks)), "the wider reach sees nobody new"
    a, _ = device_run(engine, cfgs, 3, "qk21", RING_CLEARANCE, None, (), (10,), 16)
    b, _ = device_run(engine, cfgs, 3, "qk21", RING_CLEARANCE, 2 * reach, (), (10,), 16)
    assert a == b
    assert not RM.compare(dict(cfgs=cfgs, cap=16, launches=(10,)), *b, F2.models, F2.recs)


# ----------------------------------------------------------------------------
# 2. head-on
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_two_robots_swap_places(engine, integ):
    """Two robots drive at each other: a call has blocked candidates and a
    winner that is not the winner without neighbours (asserted on the model
    first: the test cannot pass vacuously)."""
    cfgs = [robot((0.0, 0.0), (0.6, 0.0)), robot((0.6, 0.0), (0.0, 0.0))]

    def met(F):
        assert any(n > 0 and f != rec["index"]
                   for M, rr in zip(F.models, F.recs)
                   for n, f, rec in zip(M.blocked_steps, M.free, rr))

    check(engine, cfgs, 3, integ, 0.1013, (3, 4, 7), precondition=met, name=f"head-on {integ}")


# ----------------------------------------------------------------------------
# 3. the crowd and the cap
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_crowd_above_the_cap(engine, integ):
    """Twenty robots inside one reach and three static circles: K = 13 of the
    19 others are chosen, per robot, and the table is full."""
    cfgs = cloud_20()

    def capped(F):
        assert F.keep == 13
        assert all(p[0] == 19 and len(p[1]) == 13 for p in F.picks[0])
        assert len({tuple(sorted(p[1])) for p in F.picks[0]}) > 1
        assert sum(sum(M.blocked_steps) for M in F.models) > 0

    check(engine, cfgs, 3, integ, 0.0113, (1, 2), reach=0.5, static=CROWD_STATIC,
          precondition=capped, name=f"crowd {integ}")


def test_crowd_across_the_scan_chunks(engine):
    """520 robots scattered over a square, in no order: the board is scanned
    256 entries at a time (two full chunks and one of 8), every robot has more
    than 16 others within reach, and its 16 nearest come from all three
    chunks — the kept list is merged with every chunk's."""
    cfgs = cloud_520()

    def spread(F):
        assert F.keep == 16 and all(p[0] > 16 and len(p[1]) == 16 for p in F.picks[0])
        chunks = [{q // 256 for q in p[1]} for p in F.picks[0]]
        assert sum(c == {0, 1} for c in chunks) > 100 and any(2 in c for c in chunks)
        assert sum(sum(M.blocked_steps) for M in F.models) > 0

    check(engine, cfgs, 3, "rect+cum", 0.0113, (1, 1), reach=0.3, cap=4, precondition=spread,
          name="520 robots")


def test_ties_at_the_cap_and_the_reach(engine):
    """Exactly representable positions: at call 0 robot 0's 13th and 14th
    nearest are equally far (the lower index is chosen), and robot 19 stands
    at exactly d2 == reach * reach from robot 0 (strict <: not a neighbour).
    The margins at the reach and at the cap are what this case has none of;
    the margin between states and rims is asserted as everywhere."""
    cfgs = crowd(LATTICE)

    def tied(F):
        d2 = FM.d2_row(LATTICE, 0)
        within, chosen = F.picks[0][0]
        order = sorted(range(1, 19), key=lambda q: (d2[q], q))
        assert d2[19] == 0.25 * 0.25 and within == 18 and 19 not in chosen
        assert d2[order[12]] == d2[order[13]] and chosen == order[:13]
        assert F.edge == 0.0 and F.gap == 0.0

    check(engine, cfgs, 3, "qk21", 0.0113, (1, 1), reach=0.25, static=CROWD_STATIC,
          precondition=tied, ties=True, name="lattice")


# ----------------------------------------------------------------------------
# 4. ended robots stay
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_ended_robots_stay_obstacles(engine, integ):
    """Robot 0 starts on its target (no step, ever) beside robot 1's way, which
    steers around it; robot 2 arrives after two calls in the way of robot 3,
    which stops in front of it.  Both keep blocking, and their board entries
    are carried to the other side on every call (the board is compared after
    every run(1))."""
    cfgs = [parked((0.3, 0.03)), robot((0.0, 0.0), (0.6, 0.0)),
            robot((0.0, 0.4), (0.07, 0.4)), robot((-0.3, 0.42), (0.6, 0.4))]

    def stay(F):
        M0, M1, M2, M3 = F.models
        assert M0.calls == 0 and M0.stop == MPC_EP_ARRIVED
        assert M2.stop & MPC_EP_ARRIVED and F.calls >= M2.calls + 3
        assert all(b[0] == (0.3, 0.03) for b in F.boards)
        assert 0 < sum(M1.blocked_steps) and M1.blocked_steps[-1] == 0 and M1.calls == F.calls
        assert sum(M3.blocked_steps[M2.calls:]) > 0, "robot 2 blocks nothing once it has arrived"
        assert all(F.boards[c][2] == F.boards[-1][2] for c in range(M2.calls, F.calls + 1))
        assert all(p[0] is None for p in F.picks) and F.picks[-1][2] is None

    check(engine, cfgs, 3, integ, 0.0413, (1,) * 12, precondition=stay, name=f"ended {integ}")


# ----------------------------------------------------------------------------
# 5. equivalences with what exists
# ----------------------------------------------------------------------------
def stepwise(eps, n):
    """run(1) n times -> (state, log, progress) bytes and the blocked counts."""
    blocked = RB.run_launches(eps, (1,) * n, lambda e: e.read_blocked())
    return RB.snapshot(eps), np.array(blocked)


@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
@pytest.mark.parametrize("what", ("reach 0", "16 static circles", "one robot", "nobody near"))
def test_equals_the_episodes_without_neighbours(engine, integ, what):
    """reach = 0, a full static table (K = 0) and a single robot equal
    DeviceEpisodes(obstacles=static).run(1) repeated, bit for bit and count for
    count; no static circle and nobody within reach equals the plain
    mpc_episodes_run stepwise."""
    cfgs, static, reach = ring(), (NEAR,), None
    if what == "reach 0":
        reach = 0.0
    elif what == "16 static circles":
        static = (NEAR,) + tuple(OC.FILLERS[:15])
    elif what == "one robot":
        cfgs = cfgs[:1]
    else:
        cfgs, static = ring(radius=5.0), ()     # (5 apart and more)
    # (the model's margins first: the static circles alone, and the fleet as it is run)
    assert min(M.margin for M in OM.run(cfgs, 3, integ, 8, list(static), device=True)[0]) > MARGIN
    model(cfgs, 3, integ, RING_CLEARANCE, reach, static, 8)
    fleet = DeviceFleet(engine, cfgs, RING_CLEARANCE, 3, integ, log_capacity=16, obstacles=static,
                        reach=reach)
    base = DeviceEpisodes(engine, cfgs, 3, integ, log_capacity=16, obstacles=static)
    assert (base._obstacle_args() is None) == (what == "nobody near")
    got, blocked = stepwise(fleet, 8)
    want, counts = stepwise(base, 8)
    assert got == want
    assert (blocked == counts).all() and (what == "nobody near") == (blocked.sum() == 0)
    assert all(not chosen and (within == 0 or what == "16 static circles")
               for within, chosen in fleet.read_neighbours())


# ----------------------------------------------------------------------------
# 6. flagged candidates
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_flagged_candidates_are_tested_by_their_safe_states(engine, integ, n_steps):
    """Robots of robots_cases' case B (the 3 x 7 grid with |beta| = 1.2 >
    kTanMax; a start heading above kFastMax) with a parked robot on a flagged
    candidate's final state and one on a first-layer state: the recompute
    resets the flag and tests the step_safe states against the world table,
    the neighbour's circle in it."""
    base = RC.case_b(integ, n_steps, 0.5)
    sets = ([base["cfgs"][i] for i in (0, 3, 10)], [base["cfgs"][i] for i in (21, 25, 38)])
    s1 = RC.first_step(sets[0][0], n_steps, integ)[2]
    s2 = RC.first_step(sets[1][0], n_steps, integ)[2]
    B = RC.first_step(sets[0][0], n_steps, integ)[1]
    k1, k2 = 0 * 7 + 0, 2 * 7 + 4
    assert abs(B[k1 % 7]) > RC.K_TAN_MAX
    park = lambda at: parked(at, lambda s, t, heading: RC.base_cfg(
        start=(s[0], s[1], heading, 0.5, 0.0), target=t))
    cfgs = sets[0] + sets[1] + [park((float(s1[-1, 0, k1]), float(s1[-1, 1, k1]))),
                                park((float(s2[0, 0, k2]), float(s2[0, 1, k2])))]

    def flagged(F):
        assert F.models[6].calls == 0 and F.models[7].calls == 0
        assert all(6 in F.picks[0][r][1] and 7 in F.picks[0][r][1] for r in range(6))
        assert all(F.models[r].masks[0][0][k1] for r in range(3))
        assert all(F.models[r].masks[0][1 if n_steps > 1 else 0][k2] for r in range(3, 6))
        assert not any(M.masks[0][0].all() for M in F.models[:6])

    check(engine, cfgs, n_steps, integ, 0.0083, (2, 4), cap=8, precondition=flagged,
          name=f"flagged {integ} N={n_steps}")


# ----------------------------------------------------------------------------
# 7. the frame moves with the robot
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ,L", (("rect+cum", 0.5), ("rect+cum", 0.45), ("qk21", 0.5)))
def test_the_frame_moves_with_the_robot(engine, integ, L):
    """Three robots of robots_obstacle_cases' case C (the 9 x 61 grid, started
    around one point and headed past it, 40 calls over runs of 5, 7 and 28)
    with a parked robot in the middle instead of the static circle (all eight
    would jam each other within six calls): rect+cum's frame table is formed
    from each call's pose."""
    base = OC.case_c(integ, L)
    mid = RC.base_cfg(start=(*OC.C_CENTRE, 0.0, 0.5, 0.0), target=OC.C_CENTRE, L=L, eps=OC.C_EPS)
    cfgs = [base["cfgs"][j] for j in (1, 4, 6)] + [mid]

    def around(F):
        assert F.models[3].calls == 0
        assert all(any(p[r] and 3 in p[r][1] for p in F.picks) for r in range(3))
        late = [r for r, M in enumerate(F.models[:3])
                if any(f >= 0 and M.masks[s][0][f] for s, f in enumerate(M.free) if s >= 2)]
        assert late == [0, 1, 2], late
        assert max(M.calls for M in F.models) >= 8     # (a pose per call: eight frames at least)

    check(engine, cfgs, 3, integ, OC.C_RADIUS, OC.C_LAUNCHES, cap=8, precondition=around,
          name=f"frame {integ} L={L}")


# ----------------------------------------------------------------------------
# 8. the driver
# ----------------------------------------------------------------------------
def test_run_tree_fleet_equals_the_model(engine):
    """run_tree_fleet with four starts that cross in the middle of a square:
    the model's records and stop names, several host calls of eight fleet
    calls; with a clearance nothing is ever within, run_tree_batched."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import run_math_model as rmm
    mmt.reset_state()
    cfgs = [tree_episode_config(s, 24) for s in CROSSING]
    F = model(cfgs, 3, "qk21", 0.0513, None, (), 24)
    assert sum(sum(M.blocked_steps) for M in F.models) > 0 and all(M.stop for M in F.models)
    stats = {}
    got = rmm.run_tree_fleet(CROSSING, 0.0513, max_calls=24, engine=engine, stats=stats, chunk=8)
    for r, (records, stop) in enumerate(got):
        assert stop == rmm._stop_name(F.models[r].stop), r
        assert records == [[q[k] for k in ("x", "y", "phi", "v", "beta")] for q in F.recs[r]], r
    assert stats["steps"] == max(M.calls for M in F.models)
    assert stats["candidates"] == sum(M.candidates for M in F.models)
    assert stats["blocked"] == sum(sum(M.blocked_steps) for M in F.models)
    lone = model(cfgs, 3, "qk21", 1e-9, None, (), 24)      # (its margins; nothing is blocked)
    assert sum(sum(M.blocked_steps) for M in lone.models) == 0
    alone = rmm.run_tree_fleet(CROSSING, 1e-9, max_calls=24, engine=engine, chunk=8)
    assert alone == rmm.run_tree_batched(CROSSING, max_calls=24, engine=engine, obstacles=())
    assert alone != got
