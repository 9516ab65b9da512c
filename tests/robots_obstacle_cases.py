"""The cases of the batched robots' keep-out-circle test
(tests/test_robots_obstacles_gpu.py) and of its CPU preconditions
(tests/test_robots_obstacles_cpu.py): robots_cases' robots, and per case the
circles (ONE table for all robots of a launch).  A case is a robots_cases
case plus `circles` (those that may block) and `fillers` (far ones that block
nothing and fill the table up to the instantiation's count: 4 or 16 circles
share one model run).  Circles are placed once, from the host replica with the
host's 1.0 / q, and are the same numbers in a GPU run.  Radii sit off the
grid's lattice: velocity steps of 0.05 and h = 0.1 put states 0.005 apart
along a ray, so a radius such as 0.02 has a state exactly on the rim.  Test
infrastructure only."""
import functools
import math

import numpy as np

import robots_cases as RC
import robots_obstacle_model as OM
from episode_obstacle_cases import FAR
from ranking import MARGIN

NEVER = (5.0, 5.0, 0.5)       # circle (c) of ranking.circles: never reached
# episode_obstacle_cases' far circles and two more (a case of one circle fills 15 slots)
FILLERS = FAR + tuple((6.0 + 0.7 * i, -5.0, 0.3) for i in range(2))


def table(case, count):
    """The `count` circles of a launch: the case's, then far fillers."""
    circ = list(case["circles"])
    assert len(circ) <= count <= len(circ) + len(case["fillers"])
    return circ + list(case["fillers"][:count - len(circ)])


def _case(base, name, circles, fillers=FILLERS, **fields):
    return dict(base, name=name, circles=tuple(circles), fillers=tuple(fillers), **fields)


# ----------------------------------------------------------------------------
# 1. every unblocked candidate wins once
# ----------------------------------------------------------------------------
# (mode, N, L, count): all five modes at the unrolled horizon with every
# instantiation; rect+cum (the frame table) at a horizon below 3, the generic
# one and the divided wheelbase; qk21 at the generic horizon and the divided
# wheelbase.  4 and 16 circles of one shape are neighbours: one model run.
MATRIX_A = tuple(
    [(m, 3, 0.5, n) for m in RC.MODES for n in (1, 4, 16)]
    + [("rect+cum", N, L, n) for N, L in ((1, 0.5), (4, 0.5), (3, 0.3), (4, 0.3)) for n in (4, 16)]
    + [("qk21", 4, 0.3, 4)])


@functools.lru_cache(maxsize=None)
def case_a(integ, n_steps, L, one):
    """robots_cases.case_a's 549 robots (robot c's target: candidate c's final
    state) under (a) a circle on the first step's final state of the middle
    candidate, r = 0.0213 N / 3, (b) one on the first-layer state of a fast,
    steered candidate, r = 0.0083, (c) one never reached.  one: (a) alone (the
    one-circle instantiation)."""
    base = RC.case_a(integ, n_steps, L)
    V, B, states, _ = RC.first_step(RC.base_cfg(L=L), n_steps, integ)
    ka = (len(V) // 2) * len(B) + len(B) // 2
    kb = (len(V) - 1) * len(B) + 5 * len(B) // 6
    circ = [(float(states[-1, 0, ka]), float(states[-1, 1, ka]), 0.0213 * n_steps / 3),
            (float(states[0, 0, kb]), float(states[0, 1, kb]), 0.0083), NEVER]
    return _case(base, f"{base['name']} circles {'a' if one else 'abc'}",
                 circ[:1] if one else circ, () if one else FILLERS)


def check_case_a(case, models, first):
    """Before any kernel is looked at: the margin; some but not all candidates
    blocked at the first step (every robot starts from one pose: one mask);
    for N >= 2 a candidate blocked by a state before the last alone; every
    unblocked robot's first winner is its own candidate, every blocked
    robot's an unblocked one; no step of the run is all-blocked."""
    assert min(M.margin for M in models) > MARGIN, min(M.margin for M in models)
    mask, early = models[0].masks[0]
    assert all((M.masks[0][0] == mask).all() for M in models)
    assert 0 < mask.sum() < 549, int(mask.sum())
    if case["n_steps"] >= 2:
        final = OM.ranking.blocked(_first_states(case)[-1:], case["circles"])[0]
        assert (mask & ~final).any(), "no candidate is blocked by a state before the last alone"
        assert (early <= mask).all()
    for c, (costs, row) in enumerate(first):
        assert row.index >= 0 and not mask[row.index], c
        if not mask[c]:
            others = np.delete(costs, c)
            assert row.index == c and (others > costs[c]).all(), c
    assert all(n < s[0] * s[1] for M in models for n, s in zip(M.blocked_steps, M.sizes))
    return mask


def _first_states(case):
    L = case["cfgs"][0].L
    return RC.first_step(RC.base_cfg(L=L), case["n_steps"], case["integ"])[2]


# ----------------------------------------------------------------------------
# 2. flagged candidates
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_b(integ, n_steps):
    """robots_cases.case_b's two sets (|beta| = 1.2 > kTanMax on the 3 x 7
    grid; a start heading above kFastMax) under a circle on the final state of
    a flagged candidate of the first set (the slowest with beta = -1.2) and
    one on the first-layer state of a candidate of the second set (the fastest
    with beta = 0.4, flagged by the direct heading forms): the safe
    recurrence's states are what blocks them."""
    base = RC.case_b(integ, n_steps, 0.5)
    cfg = [RC._clone(base["cfgs"][0]), RC._clone(base["cfgs"][21])]
    s1 = RC.first_step(cfg[0], n_steps, integ)[2]
    s2 = RC.first_step(cfg[1], n_steps, integ)[2]
    V, B = RC.first_step(cfg[0], n_steps, integ)[:2]
    k1, k2 = 0 * 7 + 0, 2 * 7 + 4
    assert len(V) * len(B) == 21 and abs(B[k1 % 7]) > RC.K_TAN_MAX      # k1 is flagged in every mode
    circ = [(float(s1[-1, 0, k1]), float(s1[-1, 1, k1]), 0.0113),
            (float(s2[0, 0, k2]), float(s2[0, 1, k2]), 0.0067), NEVER]
    return _case(base, f"{base['name']} circles", circ, flagged_at=(k1, 21 + k2))


def check_case_b(case, models, recs):
    """The margin; the flagged candidate under the first circle is blocked at
    the first step of every robot of its set, through the safe recurrence's
    states (the replica's states of a flagged candidate are those); the second
    circle blocks its candidate in the second set, by a first-layer state; no
    first step is all-blocked; flagged candidates still win steps."""
    assert min(M.margin for M in models) > MARGIN, min(M.margin for M in models)
    k1, k2 = case["flagged_at"]
    assert all(models[r].masks[0][0][k1] for r in case["sets"][0])
    assert all(models[r].masks[0][1 if case["n_steps"] > 1 else 0][k2 - 21]
               for r in case["sets"][1])
    assert not any(M.masks[0][0].all() for M in models)
    assert sum(len(f) for f in RC.flagged_winners(case, recs)) >= 1
    assert sum(sum(M.blocked_steps) for M in models) > 42


# ----------------------------------------------------------------------------
# 3. the frame moves with the robot
# ----------------------------------------------------------------------------
C_RADIUS = 0.1213
C_CENTRE = (0.3, -0.2)
C_LAUNCHES = (5, 7, 28)
C_OFF = (0.0, 0.2, 0.3, 0.5, -0.2, -0.3, 0.4, 0.1)     # start heading off the line, per robot
C_EPS = 0.0225                # on target within 0.15: the 9 x 61 grid stops a robot 0.11 - 0.15 short


@functools.lru_cache(maxsize=None)
def case_c(integ, L):
    """Eight robots around ONE circle: robot j starts 0.5 from its centre in
    direction j, headed at it or up to 0.5 rad off, and has its target 0.5
    beyond it (1.0 ahead on the straight line, the circle of radius 0.1213
    half way).  Some stop in front of it, some drive around and arrive (the
    CPU run of OM.run decided which headings are here).  40 steps over
    launches of 5, 7 and 28 with the same table: the robot drives around, and from the second step of
    a launch on a rect+cum table formed once per launch would be in the wrong
    frame."""
    cfgs = []
    for j in range(8):
        a = 0.3 + j * math.pi / 4
        ux, uy = math.cos(a), math.sin(a)
        cfgs.append(RC.base_cfg(start=(C_CENTRE[0] - 0.5 * ux, C_CENTRE[1] - 0.5 * uy,
                                       a + C_OFF[j], 0.45, 0.0),
                                target=(C_CENTRE[0] + 0.5 * ux, C_CENTRE[1] + 0.5 * uy), L=L,
                                eps=C_EPS))
    base = dict(name=f"C {integ} L={L}", cfgs=cfgs, n_steps=3, integ=integ, launches=C_LAUNCHES,
                cap=8)
    return _case(base, base["name"], [(*C_CENTRE, C_RADIUS)])


def check_case_c(case, models, recs):
    """The margin; every robot has a step of index >= 2 whose winner without
    circles is blocked; a robot arrives; no logged pose lies inside the circle."""
    assert min(M.margin for M in models) > MARGIN, min(M.margin for M in models)
    for r, M in enumerate(models):
        assert any(f >= 0 and M.masks[s][0][f] for s, f in enumerate(M.free) if s >= 2), r
        for q in recs[r]:
            assert math.hypot(q["x"] - C_CENTRE[0], q["y"] - C_CENTRE[1]) > C_RADIUS, (r, q["step"])
    assert any(M.stop & RC.RM.MPC_EP_ARRIVED for M in models), [M.stop for M in models]


# ----------------------------------------------------------------------------
# 4. edges, one robot each
# ----------------------------------------------------------------------------
FAR_TARGET = (2.7, 3.0)


def _one(name, cfg, circles, integ, n_steps=3, launches=(6,), cap=8, **fields):
    base = dict(name=f"{name} {integ}", cfgs=[cfg], n_steps=n_steps, integ=integ,
                launches=launches, cap=cap)
    return _case(base, base["name"], circles, **fields)


def case_all_blocked(integ):
    """Every candidate blocked (r = 10 around the start)."""
    return _one("all blocked", RC.base_cfg(target=FAR_TARGET),
                [(RC.START[0], RC.START[1], 10.0)], integ)


def case_start_inside(integ):
    """The start inside a small circle (the start pose is not tested) that
    the fast candidates leave with their first step."""
    return _one("start inside", RC.base_cfg(target=FAR_TARGET),
                [(RC.START[0], RC.START[1], 0.0513)], integ)


def case_clamped(integ):
    """The 64 x 64 clamped grid of 4096 candidates (eight passes of both pair
    slots) with a circle across its middle."""
    cfg = RC.base_cfg(target=FAR_TARGET, ratio_v=40.0, ratio_beta=40.0, delta_v=0.005,
                      delta_beta=0.01)
    h = RC.START[2]
    return _one("clamped grid", cfg, [(RC.START[0] + 0.15 * math.cos(h),
                                       RC.START[1] + 0.15 * math.sin(h), 0.0313)], integ,
                launches=(3,))


def case_single(integ):
    """A grid of one candidate, which the circle blocks from its second step on."""
    cfg = RC.base_cfg(target=FAR_TARGET, ratio_v=0.0, ratio_beta=0.0)
    h = RC.START[2]
    return _one("one candidate", cfg, [(RC.START[0] + 0.3 * math.cos(h),
                                        RC.START[1] + 0.3 * math.sin(h), 0.0913)], integ)


def case_schedule(integ):
    """robots_cases.case_e's operator schedule with one circle on its path."""
    base = RC.case_e(integ)
    return _case(base, f"{base['name']} circle", [(0.13, 0.05, 0.0263)])


# ----------------------------------------------------------------------------
_RUNS = {}       # the last two model runs


def model_run(case, device):
    """OM.run of the case's robots and circles over all of its launches, the
    last two kept (robots_cases.model_run): runs that differ in their fillers'
    number alone share one.  A caller changes nothing in what it gets."""
    key = (tuple(bytes(c) for c in case["cfgs"]), case["n_steps"], case["integ"],
           sum(case["launches"]), case["circles"], case["fillers"], bool(device))
    if key not in _RUNS:
        while len(_RUNS) >= 2:
            del _RUNS[next(iter(_RUNS))]
        _RUNS[key] = OM.run(case["cfgs"], *key[1:6], device=bool(device))
    return _RUNS[key]
