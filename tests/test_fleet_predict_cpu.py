"""The predicted fleet call (mpc_episodes_fleet_run_predicted) without a GPU:
what the entry rejects before any HIP call, the motion board's size, the
model's per-step mask (MotionRobotModel, tests/fleet_model.py) against an independent
brute force, the host build of the device's centre function against numpy,
fleet_reach(predict=True) against its formula, and the follow case's
precondition on the models alone."""
import math

import numpy as np

import fleet_model as FM
import robots_cases as RC
import robots_model as RM
from diplomjourney_amd import abi, native
from diplomjourney_amd.device_episodes import fleet_reach
from fleet_cases import (FAKE, FOLLOW_CLEARANCE, circles as _circles, fleet_run as _plain,
                         fleet_run_predicted as _run, follow)


def test_rejections_before_any_hip_call():
    """motion NULL is MPC_ERR_ARG whatever else is wrong or right (an
    unsupported mode, n_calls == 0 included); with a motion board every
    rejection is mpc_episodes_fleet_run's, status for status, the fleet's own
    arguments first and mpc_episodes_run's after them; n_calls == 0 launches
    nothing.  (Every pointer is a fake: a HIP call on one would fail.)"""
    L = native.lib()
    ok = _circles((0.0, 0.0, 1.0))
    for kw in (dict(), dict(integ=7), dict(n_calls=0), dict(state=None), dict(n_steps=0),
               dict(board=None), dict(clearance=0.0)):
        assert _run(L, ok, 1, motion=None, **kw) == abi.MPC_ERR_ARG, kw
        assert _run(L, motion=None, **kw) == abi.MPC_ERR_ARG, kw
    fleet = (dict(clearance=0.0), dict(clearance=-0.1), dict(clearance=math.nan),
             dict(clearance=math.inf), dict(reach=-1e-300), dict(reach=math.nan),
             dict(reach=math.inf), dict(call0=-1), dict(n_calls=-1), dict(board=None))
    for kw in fleet:
        for more in (dict(), dict(integ=7), dict(n_calls=0) if "n_calls" not in kw else dict()):
            assert _run(L, ok, 1, **kw, **more) == abi.MPC_ERR_ARG == _plain(L, ok, 1, **kw, **more)
    assert _run(L, ok, -1) == abi.MPC_ERR_ARG
    assert _run(L, _circles(*[(0.0, 0.0, 1.0)] * 17), 17) == abi.MPC_ERR_ARG
    assert _run(L, None, 1) == abi.MPC_ERR_ARG
    assert _run(L, _circles((1.0, 1.0, 0.5), (0.0, 0.0, math.nan)), 2) == abi.MPC_ERR_ARG
    for obs, n in ((ok, 1), (None, 0)):
        for kw in (dict(state=None), dict(n_robots=0), dict(n_robots=65536), dict(n_steps=0),
                   dict(n_steps=abi.MPC_MAX_STEPS + 1), dict(cap=-1), dict(log=FAKE, cap=0),
                   dict(integ=7), dict(n_calls=0), dict(n_steps=0, integ=7)):
            want = _plain(L, obs, n, **kw)
            assert _run(L, obs, n, **kw) == want, kw
            assert want == (abi.MPC_OK if kw == dict(n_calls=0) else
                            abi.MPC_ERR_UNSUPPORTED if kw == dict(integ=7) else abi.MPC_ERR_ARG), kw
    assert _run(L, reach=0.0, n_calls=0, call0=2 ** 40 + 1) == abi.MPC_OK


def test_motion_bytes():
    """Two sides of n entries {dx, dy}, 16 B each: the pose board's size."""
    L = native.lib()
    sizes = [L.mpc_episodes_fleet_motion_bytes(n) for n in (-1, 0, 1, 6, 549, 65535)]
    assert sizes == [0, 0, 32, 192, 2 * 549 * 16, 2 * 65535 * 16]
    assert sizes == [L.mpc_episodes_fleet_board_bytes(n) for n in (-1, 0, 1, 6, 549, 65535)]


def test_centre_is_numpys():
    """fleet_predict's host build == x + j * dx as numpy evaluates it: the
    product rounded, then the sum; j = 0 and d = 0 give x back."""
    rng = np.random.default_rng(20261023)
    x = np.concatenate([rng.uniform(-3, 3, 500), [0.1, 1e300, -1e-300, 0.3]])
    d = np.concatenate([rng.uniform(-0.05, 0.05, 500), [0.2, 1e299, 1e-308, 0.1]])
    fused = 0
    for j in (0, 1, 2, 3, 4, 31, 32):
        got = FM.centres(x, d, j)
        assert (got == x + np.float64(j) * d).all(), j
        exact = np.array([float(np.longdouble(a) + np.longdouble(j) * np.longdouble(b))
                          for a, b in zip(x, d)])
        fused += int((got != exact).sum())
    assert fused > 0, "no input tells two roundings from one"
    assert (FM.centres(x, d, 0) == x).all() and (FM.centres(x, np.zeros(len(x)), 7) == x).all()


def _brute(states, static, moving, n_steps):
    """Candidate by candidate, step by step, circle by circle, in Python floats."""
    out = []
    for k in range(states.shape[2]):
        hit = False
        for j in range(1, n_steps + 1):
            x, y = float(states[j - 1, 0, k]), float(states[j - 1, 1, k])
            circ = list(static) + [(cx + float(j) * dx, cy + float(j) * dy, r)
                                   for cx, cy, dx, dy, r in moving]
            for cx, cy, r in circ:
                hit = hit or (x - cx) * (x - cx) + (y - cy) * (y - cy) < r * r
        out.append(hit)
    return np.array(out)


def test_per_step_mask_against_brute_force():
    """MotionRobotModel.score on the first step of robots_cases' base robot:
    its mask, its count, its `early` mask and every wrong multiplier's mask
    against the loops above; the moving circles are placed so that the true
    multiplier and every wrong one give different masks."""
    cfg = RC.base_cfg()
    for integ, n_steps in (("qk21", 3), ("rect+cum", 4)):
        V, B, states, costs = RC.first_step(cfg, n_steps, integ)
        k = states.shape[2] // 2
        last = (float(states[-1, 0, k]), float(states[-1, 1, k]))
        mid = (float(states[1, 0, k]), float(states[1, 1, k]))
        d = (0.004, -0.003)
        static = [(last[0] + 0.5, last[1], 0.01)]
        moving = [(last[0] - n_steps * d[0], last[1] - n_steps * d[1], d[0], d[1], 0.0051),
                  (mid[0] - 2 * 0.002, mid[1] - 2 * 0.001, 0.002, 0.001, 0.0043)]
        M = FM.MotionRobotModel(cfg, n_steps, integ, static)
        M.moving = moving
        v, b = RM.enumerate_controls(V, B, n_steps)
        scored = M.score(states, np.array(costs, dtype=np.float64), v, b)
        mask = M.masks[0][0]
        assert mask[k] and 0 < mask.sum() < len(mask)
        assert (mask == _brute(states, static, moving, n_steps)).all()
        assert M.blocked_steps == [int(mask.sum())]
        assert (np.isinf(scored) == (mask | np.isinf(costs))).all()
        assert (M.hits[0].any(axis=(0, 1)) == mask).all()
        assert (M.masks[0][1] == M.hits[0][:-1].any(axis=(0, 1))).all()
        for name, mult in FM.WRONG.items():
            count, _, wm = M.wrong[name][0]
            want = np.zeros(len(mask), dtype=bool)
            for j in range(1, n_steps + 1):      # (step j alone, the circle moved mult times)
                x, y = states[j - 1, 0, :], states[j - 1, 1, :]
                for cx, cy, dx, dy, r in moving:
                    m = mult(j, n_steps)
                    want |= (x - (cx + m * dx)) ** 2 + (y - (cy + m * dy)) ** 2 < r * r
            assert (wm == want).all() and count == want.sum(), name
            assert (wm != mask).any(), name


def test_predicted_reach_is_its_formula():
    """fleet_reach(predict=True): the far term doubled; the default unchanged."""
    slow = RC.base_cfg()
    fast = RC.base_cfg(v_max=1.5, delta_t=0.2)
    assert fleet_reach([slow], 3, 0.07, predict=True) == 2 * (3 * 0.1 * 1.0) * (1.0 + 2.0 ** -40) + 0.07
    assert fleet_reach([slow, fast], 4, 0.0, predict=True) == 2 * (4 * 0.2 * 1.5) * (1.0 + 2.0 ** -40)
    assert fleet_reach([slow], 3, 0.07) == fleet_reach([slow], 3, 0.07, predict=False)
    assert fleet_reach([slow], 3, 0.07) == 3 * 0.1 * 1.0 * (1.0 + 2.0 ** -40) + 0.07


def test_follow_precondition_on_the_models():
    """A follower behind a leader: the standing circle covers the follower's
    whole horizon, so the standing model's follower has every candidate
    blocked in calls 0 and 1 and is stopped as stuck after two calls; under
    the prediction only call 0 is blocked (nobody has moved yet) and the
    follower runs all ten calls.  The motion list is what the boards say."""
    cfgs = follow()
    reach = fleet_reach(cfgs, 3, FOLLOW_CLEARANCE, predict=True)
    S = FM.Fleet(cfgs, 3, "rect+cum", FOLLOW_CLEARANCE, reach).run(10, device=False)
    assert S.models[0].calls == 2 and S.models[0].stop and S.models[0].blocked_steps == [451, 451]
    P = FM.Fleet(cfgs, 3, "rect+cum", FOLLOW_CLEARANCE, reach, predict=True).run(10,
                                                                                 device=False)
    M = P.models[0]
    assert M.calls == 10 and not M.stop and M.blocked_steps[0] == 451
    assert all(n < 451 for n in M.blocked_steps[1:])
    assert P.motions[0] == [(0.0, 0.0)] * 2
    for c in range(1, 11):
        for r in range(2):
            assert P.motions[c][r] == (P.boards[c][r][0] - P.boards[c - 1][r][0],
                                       P.boards[c][r][1] - P.boards[c - 1][r][1])
    assert P.motions[1][0] == (0.0, 0.0) and P.motions[2][0] != (0.0, 0.0)
    assert len(P.motion(0)) == len(P.motion(10)) == 64 and P.motion(0) == bytes(64)
    assert np.frombuffer(P.motion(3), dtype=np.float64).reshape(2, 2, 2)[1].tolist() == [
        list(m) for m in P.motions[3]]
