"""The planned fleet call (mpc_episodes_fleet_run_planned) without a GPU: the
plan board's size, what the entry rejects before any HIP call, each against
mpc_episodes_fleet_run_predicted's order, DeviceFleet's ValueError, the model's
per-step mask (PlanRobotModel, tests/fleet_plan_model.py) against an
independent brute force, and the preconditions of tests/test_fleet_plan_gpu.py's
scenes on the models alone (the host's reciprocal estimates)."""
import math

import numpy as np
import pytest

import fleet_plan_bench as PB
import fleet_plan_cases as PC
import fleet_plan_model as PM
import robots_cases as RC
import robots_model as RM
from diplomjourney_amd import abi, native
from diplomjourney_amd.abi import MPC_MAX_STEPS
from diplomjourney_amd.device_episodes import DeviceFleet, fleet_reach
from fleet_cases import (FAKE, FOLLOW_CLEARANCE, RING_CLEARANCE, circles as _circles,
                         fleet_run_predicted as _predicted, follow, long_crowd, ring)
from fleet_plan_cases import fleet_run_planned as _run


def test_plan_bytes():
    """Two sides of n entries {x1, y1, x2, y2}, 32 B each."""
    L = native.lib()
    sizes = [L.mpc_episodes_fleet_plan_bytes(n) for n in (-1, 0, 1, 6, 549, 65535)]
    assert sizes == [0, 0, 64, 384, 2 * 549 * 32, 2 * 65535 * 32]


def test_rejections_before_any_hip_call():
    """plan NULL is MPC_ERR_ARG whatever else is wrong or right (an unsupported
    mode, n_calls == 0 included), as motion NULL is for the predicted entry;
    with a plan board every rejection is the predicted entry's, status for
    status — call0 < 0 and a bad clearance among the fleet's own arguments,
    mpc_episodes_run's after them; n_calls == 0 launches nothing.  (Every
    pointer is a fake: a HIP call on one would fail.)"""
    L = native.lib()
    ok = _circles((0.0, 0.0, 1.0))
    for kw in (dict(), dict(integ=7), dict(n_calls=0), dict(state=None), dict(n_steps=0),
               dict(board=None), dict(clearance=0.0), dict(call0=-1)):
        assert _run(L, ok, 1, plan=None, **kw) == abi.MPC_ERR_ARG, kw
        assert _run(L, plan=None, **kw) == abi.MPC_ERR_ARG, kw
        assert _predicted(L, ok, 1, motion=None, **kw) == abi.MPC_ERR_ARG, kw
    fleet = (dict(call0=-1), dict(call0=-2 ** 40), dict(clearance=0.0), dict(clearance=-0.1),
             dict(clearance=math.nan), dict(clearance=math.inf), dict(reach=-1e-300),
             dict(reach=math.nan), dict(reach=math.inf), dict(n_calls=-1), dict(board=None))
    for kw in fleet:
        for more in (dict(), dict(integ=7), dict(n_calls=0) if "n_calls" not in kw else dict(),
                     dict(state=None)):
            assert (_run(L, ok, 1, **kw, **more) == abi.MPC_ERR_ARG
                    == _predicted(L, ok, 1, **kw, **more)), (kw, more)
    assert _run(L, ok, -1) == abi.MPC_ERR_ARG
    assert _run(L, _circles(*[(0.0, 0.0, 1.0)] * 17), 17) == abi.MPC_ERR_ARG
    assert _run(L, None, 1) == abi.MPC_ERR_ARG
    assert _run(L, _circles((1.0, 1.0, 0.5), (0.0, 0.0, math.nan)), 2) == abi.MPC_ERR_ARG
    for obs, n in ((ok, 1), (None, 0)):
        for kw in (dict(state=None), dict(n_robots=0), dict(n_robots=65536), dict(n_steps=0),
                   dict(n_steps=abi.MPC_MAX_STEPS + 1), dict(cap=-1), dict(log=FAKE, cap=0),
                   dict(integ=7), dict(n_calls=0), dict(n_steps=0, integ=7)):
            want = _predicted(L, obs, n, **kw)
            assert _run(L, obs, n, **kw) == want, kw
            assert want == (abi.MPC_OK if kw == dict(n_calls=0) else
                            abi.MPC_ERR_UNSUPPORTED if kw == dict(integ=7) else abi.MPC_ERR_ARG), kw
    assert _run(L, reach=0.0, n_calls=0, call0=2 ** 40 + 1) == abi.MPC_OK


def test_device_fleet_refuses_other_predictions():
    """predict is False, True or "plan": anything else is a ValueError, raised
    before the device is touched."""
    for bad in ("plans", "Plan", "", None, 2, "true"):
        with pytest.raises(ValueError):
            DeviceFleet(None, [], 0.1, predict=bad)


def _brute(states, static, entries, r, n_steps):
    """Candidate by candidate, step by step, circle by circle, in Python floats."""
    out = []
    for k in range(states.shape[2]):
        hit = False
        for j in range(1, n_steps + 1):
            x, y = float(states[j - 1, 0, k]), float(states[j - 1, 1, k])
            circ = list(static)
            for x1, y1, x2, y2 in entries:
                if j == 1:
                    circ.append((x1, y1, r))
                elif j == 2:
                    circ.append((x2, y2, r))
                else:
                    circ.append((x2 + float(j - 2) * (x2 - x1), y2 + float(j - 2) * (y2 - y1), r))
            for cx, cy, cr in circ:
                hit = hit or (x - cx) * (x - cx) + (y - cy) * (y - cy) < cr * cr
        out.append(hit)
    return np.array(out)


def test_per_step_mask_against_brute_force():
    """PlanRobotModel.score on the first step of robots_cases' base robot: its
    mask, its count and its `early` mask against the loops above, with one
    neighbour whose extrapolated circle lies on a candidate's last state and one
    whose a2 lies on a candidate's second; the rules that read the same board
    otherwise (hold, j - 1, j - 3) give other masks."""
    cfg = RC.base_cfg()
    for integ, n_steps in (("qk21", 3), ("rect+cum", 4)):
        V, B, states, costs = RC.first_step(cfg, n_steps, integ)
        k = states.shape[2] // 2
        last = (float(states[-1, 0, k]), float(states[-1, 1, k]))
        mid = (float(states[1, 0, k]), float(states[1, 1, k]))
        d = (0.004, -0.003)
        static = [(last[0] + 0.5, last[1], 0.01)]
        a2 = (last[0] - (n_steps - 2) * d[0], last[1] - (n_steps - 2) * d[1])
        entries = [(a2[0] - d[0], a2[1] - d[1], a2[0], a2[1]),
                   (mid[0] - 0.002, mid[1] - 0.001, mid[0], mid[1])]
        M = PM.PlanRobotModel(cfg, n_steps, integ, static)
        M.near = dict(pos=[(0.0, 0.0)] * 2, mot=[(0.0, 0.0)] * 2, plan=entries, early=entries,
                      ot=entries, r=0.0047)
        v, b = RM.enumerate_controls(V, B, n_steps)
        scored = M.score(states, np.array(costs, dtype=np.float64), v, b)
        mask = M.masks[0][0]
        assert mask[k] and 0 < mask.sum() < len(mask)
        assert (mask == _brute(states, static, entries, 0.0047, n_steps)).all()
        assert M.blocked_steps == [int(mask.sum())]
        assert (np.isinf(scored) == (mask | np.isinf(costs))).all()
        assert (M.hits[0].any(axis=(0, 1)) == mask).all()
        assert (M.masks[0][1] == M.hits[0][:-1].any(axis=(0, 1))).all()
        for name in ("standing", "moved", "hold", "j-1", "j-3"):
            assert (M.wrong[name][0][2] != mask).any(), name
        for name in ("early", "ot"):        # (the same entries here: the same mask)
            assert (M.wrong[name][0][2] == mask).all(), name


def test_the_plan_board_of_the_model():
    """PlanFleet.plan(c): side c & 1 what call c - 1 published, the other side
    what it read; side 0 before call 0 the start positions twice."""
    cfgs = follow()
    F = PB.model(cfgs, 3, "rect+cum", FOLLOW_CLEARANCE, None, (), 3, device=False)
    assert F.plans[0] == [PM.stand(p) for p in F.boards[0]] and F.motion(2) is None
    for c in (1, 2, 3):
        sides = np.frombuffer(F.plan(c), dtype=np.float64).reshape(2, 2, 4)
        assert sides[c & 1].tolist() == [list(e) for e in F.plans[c]]
        assert sides[(c - 1) & 1].tolist() == [list(e) for e in F.plans[c - 1]]
    # a robot that goes on after a step with a winner: layers 1 and 2 of its ot
    M = F.models[1]
    assert F.plans[1][1] == (*M.ots[0][1], *M.ots[0][2]) and M.layers[0] == (0, False)
    assert F.boards[1][1] == M.ots[0][0]


@pytest.mark.parametrize("integ,n_steps,L", (("qk21", 3, 0.5), ("rect+cum", 4, 0.45)))
def test_ring_precondition_on_the_model(integ, n_steps, L):
    F = PB.model(ring(L), n_steps, integ, RING_CLEARANCE, None, (), 10, device=False)
    PC.ring_plans(F)


@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_scene_preconditions_on_the_models(integ):
    """The turning leader, the parked neighbours, the finishing neighbour, the
    stale neighbour and the flagged candidates."""
    cfgs, clearance, n_calls = PC.turning()
    reach = fleet_reach(cfgs, 3, clearance, predict=True)
    F = PB.model(cfgs, 3, integ, clearance, reach, (), n_calls, device=False)
    PC.turns(F, cfgs, integ, clearance, reach, n_calls, False)
    reach = fleet_reach(PC.PARKED, 3, PC.PARKED_CLEARANCE, predict=True)
    PC.parked_stand(PB.model(PC.PARKED, 3, integ, PC.PARKED_CLEARANCE, reach, PC.PARKED_STATIC, 8,
                             device=False))
    cfgs, clearance, n_calls = PC.finishing()
    PC.finishes(PB.model(cfgs, 3, integ, clearance, None, (), n_calls, device=False))
    PC.stale_stands(PB.model(follow(), 3, integ, FOLLOW_CLEARANCE, None, (), 10, device=False))
    for n_steps in (3, 4):
        cfgs, clearance = PC.flagged_plan_fleet(integ, n_steps, device=False)
        PC.flagged(PB.model(cfgs, n_steps, integ, clearance, None, (), 4, device=False))


def test_longest_horizon_precondition_on_the_model():
    PC.second_pass(PB.model(long_crowd(), MPC_MAX_STEPS, "qk21", 0.0113, None, (), 3,
                            device=False))


def test_crossing_precondition_on_the_model():
    from diplomjourney_amd.episode_config import tree_episode_config
    kw = PC.CROSSING_RUN
    cfgs = [tree_episode_config(s, kw["max_calls"]) for s in PC.CROSSING_TURNED]
    F = PB.model(cfgs, 3, "qk21", kw["clearance"], None, kw["obstacles"], kw["max_calls"],
                 device=False)
    PC.crossing_differs(F, cfgs, False)
