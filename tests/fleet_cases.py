"""The scenes of the fleet tests (tests/test_fleet_gpu.py,
tests/test_fleet_predict_gpu.py) and of their CPU preconditions
(tests/test_fleet_cpu.py, tests/test_fleet_predict_cpu.py): the robots'
configurations, clearances, static circles and launch splits, and the argument
list of the two fleet entries for the tests of what they reject.  Nothing here
needs a GPU unless it is asked for the device's estimates.  Test
infrastructure only."""
import ctypes
import math

import numpy as np

import fleet_model as FM
import robots_cases as RC
import robots_obstacle_cases as OC
from diplomjourney_amd import abi
from diplomjourney_amd.episode_config import reference_episode_config


def robot(start, target, L=0.5, heading=None, v=0.5):
    """A robot of the reference's configuration (11 x 41 grid, delta_t = 0.05,
    arrival within sqrt(0.001)), no operator events, run_math_model.py's stuck
    rule; headed at its target unless told otherwise."""
    if heading is None:
        heading = math.atan2(target[1] - start[1], target[0] - start[0])
    c = reference_episode_config(start=(start[0], start[1], heading, v, 0.0), target=target,
                                 enumerate=True)
    c.L = L
    c.p_turn_right = c.p_turn_left = c.p_new_target = 0
    c.stop_rule = 1
    return c


def parked(at, make=robot):
    """A robot that starts on its target: stopped at reset, an obstacle for good."""
    return make(at, at, heading=0.0)


# ----------------------------------------------------------------------------
# six robots on a ring
# ----------------------------------------------------------------------------
RING_CLEARANCE = 0.0213
SPLIT = (1, 1, 1, 2, 5)
RING_JITTER = (0.0, 0.05, -0.07, 0.11, 0.02, -0.04)


def ring(L=0.5, radius=0.17):
    """Six robots on a ring, each with its target diametrically opposite: they
    meet in the middle after six calls (0.025 per call).  The ring is a little
    irregular (radius + 0.012 j, the angles jittered), so that the robots do
    not all do the same and a rim cuts through a step's candidates."""
    out = []
    for j in range(6):
        a = 0.2 + 2 * math.pi * j / 6 + RING_JITTER[j]
        p = ((radius + 0.012 * j) * math.cos(a), (radius + 0.012 * j) * math.sin(a))
        out.append(robot(p, (-p[0], -p[1]), L))
    return out


NEAR = (0.05, 0.02, 0.0313)        # a static circle the ring's robots meet


# ----------------------------------------------------------------------------
# a follower behind a leader
# ----------------------------------------------------------------------------
FOLLOW_CLEARANCE = 0.0513


def follow():
    return [robot((0.0, 0.0), (0.8, 0.0)), robot((0.09, 0.004), (0.8, 0.01))]


# ----------------------------------------------------------------------------
# crowds
# ----------------------------------------------------------------------------
CROWD_STATIC = ((0.16, 0.05, 0.0213), OC.FILLERS[0], OC.FILLERS[1])
LATTICE = [(i / 32.0, j / 32.0) for j in range(4) for i in range(5)][:19] + [(8 / 32.0, 0.0)]


def crowd(points):
    """Every robot headed the same way at a far target of its own."""
    return [robot(p, (p[0] + 3.0, p[1] + 1.0)) for p in points]


def _cloud(seed, count, draw, inside=lambda p: True):
    """`count` points drawn by draw(rng), nobody nearer than 0.03 to another."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < count:
        p = draw(rng)
        if inside(p) and all(np.hypot(*(p - q)) > 0.03 for q in pts):
            pts.append(p)
    return pts


def _disc(seed, count):
    """A cloud of radius 0.12."""
    return _cloud(seed, count, lambda rng: rng.uniform(-0.12, 0.12, 2),
                  lambda p: np.hypot(*p) < 0.12)


def cloud_20():
    """Twenty robots inside one reach."""
    return crowd([(float(p[0]), float(p[1])) for p in _disc(20261021, 20)])


def cloud_520():
    """520 robots scattered over a square, in no order."""
    return crowd([(float(p[0]), float(p[1]))
                  for p in _cloud(20261022, 520, lambda rng: rng.uniform(0.0, 1.0, 2))])


def long_crowd():
    """18 robots with case B's 3 x 7 grid in one cloud, headed one way."""
    out = []
    for p in _disc(20261024, 18):
        x, y = float(p[0]), float(p[1])
        out.append(RC.base_cfg(start=(x, y, math.atan2(1.0, 3.0), 0.5, 0.0),
                               target=(x + 3.0, y + 1.0), ratio_v=1.0, delta_beta=0.4,
                               ratio_beta=3.0, beta_bound=1.3))
    return out


# ----------------------------------------------------------------------------
# a moving neighbour on a flagged candidate
# ----------------------------------------------------------------------------
FLAG_CLEARANCE = 0.0083


def flagged_fleet(integ, n_steps, device=True):
    """Two robots of robots_cases' case B (one of each set) and a moving
    neighbour (the reference's robot, 0.025 a call) started where its circle
    at step N of fleet call 1 lies on a flagged candidate's state after step N
    of robot 0: the robots' lone runs give that state and the neighbour's
    first displacement; the fleet's model then says whether it came so."""
    base = RC.case_b(integ, n_steps, 0.5)
    a, a2 = base["cfgs"][0], base["cfgs"][21]
    lone = FM.Fleet([a], n_steps, integ, FLAG_CLEARANCE, 0.0, predict=True).run(2, device=device)
    M = lone.models[0]
    k = int(np.flatnonzero(np.abs(M.betas[1]) > RC.K_TAN_MAX)[0])
    at = (float(M.states[1][n_steps - 1, 0, k]), float(M.states[1][n_steps - 1, 1, k]))
    u = (math.cos(2.3), math.sin(2.3))
    q = FM.Fleet([robot((0.0, 0.0), (3 * u[0], 3 * u[1]))], n_steps, integ, FLAG_CLEARANCE, 0.0,
                 predict=True).run(1, device=device)
    d = q.motions[1][0]
    p0 = (at[0] - (n_steps + 1) * d[0], at[1] - (n_steps + 1) * d[1])
    return [a, a2, robot(p0, (p0[0] + 3 * u[0], p0[1] + 3 * u[1]))], k


# ----------------------------------------------------------------------------
# four starts that cross in the middle of a square (run_tree_fleet)
# ----------------------------------------------------------------------------
CROSSING = [(0.0, 0.0, math.pi / 4, 0.3, 0.3), (0.3, 0.0, 3 * math.pi / 4, 0.0, 0.3),
            (0.3, 0.3, -3 * math.pi / 4, 0.0, 0.0), (0.0, 0.3, -math.pi / 4, 0.3, 0.0)]


# ----------------------------------------------------------------------------
# the entries' arguments, for what they reject before any HIP call
# ----------------------------------------------------------------------------
FAKE = ctypes.c_void_p(0x1000)     # (a HIP call on it would fail)


def circles(*rows):
    return abi.make_obstacles(rows)[0]


def fleet_args(obs=None, n=0, state=FAKE, board=FAKE, call0=0, clearance=0.1, reach=0.3,
               n_robots=1, n_steps=3, integ=0, n_calls=1, log=None, cap=0):
    """(state, board) and what follows them in mpc_episodes_fleet_run; the
    predicted entry takes its motion board between the two."""
    return (state, board), (call0, obs, n, clearance, reach, n_robots, n_steps, integ, n_calls,
                            log, cap, None, None, None, None)


def fleet_run(L, *a, **kw):
    head, rest = fleet_args(*a, **kw)
    return L.mpc_episodes_fleet_run(*head, *rest)


def fleet_run_predicted(L, *a, motion=FAKE, **kw):
    head, rest = fleet_args(*a, **kw)
    return L.mpc_episodes_fleet_run_predicted(*head, motion, *rest)
