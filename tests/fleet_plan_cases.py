"""The scenes of the planned fleet call's tests (tests/test_fleet_plan_cpu.py,
tests/test_fleet_plan_gpu.py) that fleet_cases does not have, each with the
precondition it must meet on the host model alone, and the argument list of
mpc_episodes_fleet_run_planned.  Test infrastructure only."""
import numpy as np

import fleet_plan_model as PM
import robots_cases as RC
from diplomjourney_amd.abi import MPC_EP_ARRIVED, MPC_MAX_OBSTACLES
from fleet_cases import CROSSING, FAKE, fleet_args, parked, robot


def fleet_run_planned(L, *a, plan=FAKE, **kw):
    head, rest = fleet_args(*a, **kw)
    return L.mpc_episodes_fleet_run_planned(*head, plan, *rest)


def records(F):
    """Per robot, per step: what the log keeps of the step."""
    return [[(q["index"], q["x"], q["y"], q["phi"], q["status"]) for q in rr] for rr in F.recs]


# ----------------------------------------------------------------------------
# the ring: every wrong rule gives other counts and other winners
# ----------------------------------------------------------------------------
def ring_plans(F):
    """A rim cuts through a step's candidates, and under each wrong rule some
    step's blocked count and some step's winner are others."""
    assert any(p[0] >= 1 for p in F.picks[0]), F.picks[0]
    assert any(0 < n < 451 for M in F.models for n in M.blocked_steps)
    for name, (counts, wins) in F.separated().items():
        assert counts >= 1 and wins >= 1, (name, counts, wins)


# ----------------------------------------------------------------------------
# a stale neighbour
# ----------------------------------------------------------------------------
def stale_stands(F):
    """fleet_cases.follow(): in call 0 everybody stands, the leader's circle
    covers the follower's whole horizon, and its step is stale: it publishes
    its position twice, and the leader reads that entry in call 1.  From call 1
    on the leader's circle follows its plan and the follower runs."""
    M = F.models[0]
    assert M.blocked_steps[0] == 451 and M.layers[0] == (0, True)
    assert F.plans[1][0] == PM.stand(F.boards[1][0]) and F.boards[1][0] == F.boards[0][0]
    assert F.plans[1][1] != PM.stand(F.boards[1][1])
    assert F.picks[1][1] == (1, [0]), "nobody reads the stale robot's entry"
    assert M.calls == 10 and not M.stop and all(n < 451 for n in M.blocked_steps[1:])


# ----------------------------------------------------------------------------
# the longest horizon
# ----------------------------------------------------------------------------
def second_pass(F):
    """A full table in every call, and some candidate blocked by entries of
    steps 17..32 alone: the second pass over the table, and the extrapolation."""
    assert all(p is not None and len(p[1]) == MPC_MAX_OBSTACLES for row in F.picks for p in row)
    late = [(r, c, int(k)) for r, M in enumerate(F.models) for c in range(1, M.calls)
            for k in np.flatnonzero(M.hits[c][16:].any(axis=(0, 1))
                                    & ~M.hits[c][:16].any(axis=(0, 1)))]
    assert late, "no candidate is blocked by the second pass's entries alone"
    assert any(p != PM.stand(q) for p, q in zip(F.plans[1], F.boards[1]))
    for name in ("standing", "hold", "j-1", "j-3"):
        assert F.separated()[name][0] >= 1, name


# ----------------------------------------------------------------------------
# parked neighbours
# ----------------------------------------------------------------------------
PARKED = [robot((0.0, 0.0), (0.6, 0.0)), parked((0.3, 0.03)), parked((0.18, -0.05)),
          parked((0.45, 0.04))]
PARKED_STATIC = ((0.1, 0.06, 0.0313),)
PARKED_CLEARANCE = 0.0413


def parked_stand(F):
    """One moving robot among parked ones: every entry a block reads is a
    position twice, and circles are tested (the robot steers around them)."""
    assert sum(F.models[0].blocked_steps) > 0 and F.models[0].calls == 8
    assert all(plans[q] == PM.stand(pos[q]) for plans, pos in zip(F.plans, F.boards)
               for q in (1, 2, 3))
    assert any(plans[0] != PM.stand(pos[0]) for plans, pos in zip(F.plans, F.boards))


# ----------------------------------------------------------------------------
# a turning leader
# ----------------------------------------------------------------------------
def turning():
    """Robot 0 drives along the x axis; the leader starts beside it, headed the
    same way, with its target far off to the other side: a short wheelbase
    (L = 0.25) lets it turn hard, across robot 0's way.  -> (cfgs, clearance,
    fleet calls)."""
    return ([robot((0.0, 0.0), (0.8, 0.0)),
             robot((0.0, 0.08), (0.3, -0.8), L=0.25, heading=0.0)], 0.0513, 6)


def turns(F, cfgs, integ, clearance, reach, n_calls, device):
    """The leader's plan is an arc (its published points and its position are
    not on one line), a rim cuts through robot 0's candidates, and the run is
    neither the constant displacement's nor the standing circles'."""
    import robots_bench as RB
    lead = [(p[1], q[1]) for p, q in zip(F.plans[1:], F.boards[1:]) if p[1] != PM.stand(q[1])]
    assert lead and any(abs((a[0] - p[0]) * (a[3] - p[1]) - (a[1] - p[1]) * (a[2] - p[0])) > 1e-6
                        for a, p in lead), "the leader's plan is a straight line"
    assert any(0 < n < 451 for n in F.models[0].blocked_steps)
    for predict in (True, False):
        other = RB.fleet_model(cfgs, 3, integ, clearance, reach, (), n_calls, predict=predict,
                               device=device)
        assert records(other) != records(F), f"the run is predict={predict}'s"
    sep = F.separated()
    assert sep["moved"][0] >= 1 and sep["standing"][0] >= 1, sep


# ----------------------------------------------------------------------------
# a finishing neighbour
# ----------------------------------------------------------------------------
def finishing():
    """Robot 0 (robots_cases' wide velocity grid, arrival within 0.01) probes
    its target in call 0, returns layer 1 in call 1 — short of the target: it
    slows down — and layer 2 in call 2, where it arrives.  Robot 1 comes up
    behind it and reads its entries.  -> (cfgs, clearance, fleet calls)."""
    fin = RC.base_cfg(start=(0.0, 0.4, 0.0, 0.5, 0.0), target=(0.12, 0.4), eps=1e-4)
    return [fin, robot((-0.3, 0.42), (0.6, 0.4))], 0.0413, 10


def finishes(F):
    M, other = F.models
    assert [k for k, _ in M.layers] == [0, 1, 2] and not any(s for _, s in M.layers)
    assert M.stop & MPC_EP_ARRIVED and F.calls >= M.calls + 3
    # call 0: the next two layers; call 1 (m = 1, layer 1 returned): layer 2 twice
    assert F.plans[1][0] == (*M.ots[0][1], *M.ots[0][2]) and M.ots[0][1] != M.ots[0][2]
    assert F.plans[2][0] == (*M.ots[1][2], *M.ots[1][2]) != PM.stand(F.boards[2][0])
    # call 2 (m = 2): it arrives on layer 2 and stands there from then on
    assert F.boards[3][0] == M.ots[2][2] and F.boards[3][0] != F.boards[2][0]
    assert all(F.plans[c][0] == PM.stand(F.boards[3][0]) for c in range(3, F.calls + 1))
    both = np.frombuffer(F.plan(4), dtype=np.float64).reshape(2, 2, 4)
    assert (both[:, 0] == np.array(PM.stand(F.boards[3][0]))).all()
    # somebody reads every one of these entries, and meets the standing circle
    assert all(F.picks[c][1] is not None and 0 in F.picks[c][1][1] for c in range(0, 5))
    assert sum(other.blocked_steps[M.calls:]) > 0, "the arrived robot blocks nothing"


# ----------------------------------------------------------------------------
# a turning neighbour on a flagged candidate
# ----------------------------------------------------------------------------
FLAG_CLEARANCE = 0.0083


def flagged_plan_fleet(integ, n_steps, device=True):
    """Two robots of robots_cases' case B (one of each set) and a TURNING
    neighbour (L = 0.25, its target 1.2 rad off its heading) started where, in
    fleet call 1, its planned circle of step N covers a flagged candidate's
    state after step N of robot 0 and the constant displacement's circle of
    step N does not: the robots' lone runs give that state, the neighbour's
    first plan entry and its first displacement; the state is put inside the
    planned rim by half the two centres' distance, on the far side of the
    displaced centre.  -> (cfgs, clearance)."""
    base = RC.case_b(integ, n_steps, 0.5)
    a, a2 = base["cfgs"][0], base["cfgs"][21]
    lone = PM.PlanFleet([a], n_steps, integ, FLAG_CLEARANCE, 0.0).run(2, device=device)
    M = lone.models[0]
    k = int(np.flatnonzero(np.abs(M.betas[1]) > RC.K_TAN_MAX)[0])
    at = np.array([M.states[1][n_steps - 1, 0, k], M.states[1][n_steps - 1, 1, k]])

    def neighbour(p0):
        t = (p0[0] + 3 * np.cos(2.3 - 1.2), p0[1] + 3 * np.sin(2.3 - 1.2))
        return robot((float(p0[0]), float(p0[1])), (float(t[0]), float(t[1])), L=0.25, heading=2.3)

    q = PM.PlanFleet([neighbour((0.0, 0.0))], n_steps, integ, FLAG_CLEARANCE, 0.0).run(
        1, device=device)
    x1, y1, x2, y2 = q.plans[1][0]
    planned = np.array([x2 + (n_steps - 2) * (x2 - x1), y2 + (n_steps - 2) * (y2 - y1)])
    moved = np.array(q.boards[1][0]) + n_steps * np.array(q.motions[1][0])
    apart = float(np.hypot(*(planned - moved)))
    assert apart > 1e-4, "the neighbour's plan is its displacement's line"
    p0 = at - (planned - moved) / apart * (FLAG_CLEARANCE - 0.5 * apart) - planned
    return [a, a2, neighbour(p0)], FLAG_CLEARANCE


def flagged(F):
    """Some flagged candidate of robot 0 is blocked by the neighbour's planned
    circle of a step j >= 2 and by neither its standing circle nor its
    constant-displacement one."""
    M = F.models[0]
    found = []
    for c in range(1, M.calls):
        if 2 not in (F.picks[c][0] or (0, []))[1]:
            continue
        i = len(F.static) + F.picks[c][0][1].index(2)
        for kk in np.flatnonzero(np.abs(M.betas[c]) > RC.K_TAN_MAX):
            late = M.hits[c][1:, i, kk].any()
            if late and not M.wrong["standing"][c][2][kk] and not M.wrong["moved"][c][2][kk]:
                found.append((c, int(kk)))
    assert found, "no flagged candidate is blocked by a planned circle alone"
    assert F.plans[found[0][0]][2] != PM.stand(F.boards[found[0][0]][2])
    assert not any(m.all() for m, _ in M.masks)


# ----------------------------------------------------------------------------
# the driver: fleet_cases.CROSSING with every heading turned
# ----------------------------------------------------------------------------
# Headed at their targets the four robots drive straight, and a straight plan is
# the constant displacement's line: the planned run IS predict=True's (the model
# says so for every clearance).  Started 0.8 rad off their target lines they
# turn all the way to the middle, and the planned run is neither of the others.
CROSSING_TURNED = [(x, y, phi + 0.8, xt, yt) for x, y, phi, xt, yt in CROSSING]
CROSSING_RUN = dict(clearance=0.1513, max_calls=24, obstacles=())


def crossing_differs(F, cfgs, device):
    """Circles block candidates, everybody ends, and the records are neither
    predict=True's nor predict=False's."""
    import robots_bench as RB
    assert sum(sum(M.blocked_steps) for M in F.models) > 0 and all(M.stop for M in F.models)
    for predict in (True, False):
        other = RB.fleet_model(cfgs, 3, "qk21", CROSSING_RUN["clearance"], None, (),
                               CROSSING_RUN["max_calls"], predict=predict, device=device)
        assert records(other) != records(F), f"the run is predict={predict}'s"
