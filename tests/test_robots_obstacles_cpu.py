"""Keep-out circles in the batched robots' episodes, without a GPU: what
mpc_episodes_run_obstacles rejects before any HIP call, the Python layer's
checks, the preconditions of every case of tests/test_robots_obstacles_gpu.py
on the IEEE replica (host 1.0 / q: margins, the masks' sizes, who wins), and
the model's blocked counts against a direct recount."""
import ctypes
import math

import numpy as np
import pytest

import harness
import ranking
import robots_cases as RC
import robots_model as RM
import robots_obstacle_cases as OC
import robots_obstacle_model as OM
from diplomjourney_amd import abi, native


def _circles(*rows):
    return abi.make_obstacles(rows)[0]


def test_rejections_before_any_hip_call():
    """The circles are checked first, with mpc_rollout_partials_obstacles'
    rejections; with valid circles the base entry's rejections, status for
    status; max_calls == 0 launches nothing."""
    L = native.lib()
    fake = ctypes.c_void_p(0x1000)
    ok = _circles((0.0, 0.0, 1.0))

    def run(obs, n, state=fake, n_robots=1, n_steps=3, integ=0, max_calls=1, log=None, cap=0):
        return L.mpc_episodes_run_obstacles(state, obs, n, n_robots, n_steps, integ, max_calls,
                                            log, cap, None, None, None)

    assert run(ok, -1) == abi.MPC_ERR_ARG
    assert run(_circles(*[(0.0, 0.0, 1.0)] * 17), 17) == abi.MPC_ERR_ARG
    assert run(None, 1) == abi.MPC_ERR_ARG
    for bad in ((math.nan, 0.0, 1.0), (0.0, math.inf, 1.0), (0.0, -math.inf, 1.0), (0.0, 0.0, 0.0),
                (0.0, 0.0, -1.0), (0.0, 0.0, math.nan), (0.0, 0.0, math.inf)):
        assert run(_circles((1.0, 1.0, 0.5), bad), 2) == abi.MPC_ERR_ARG, bad
    # the circles come first: a bad circle with an unsupported mode is an argument error
    assert run(_circles((0.0, 0.0, 0.0)), 1, integ=7) == abi.MPC_ERR_ARG
    # with valid circles (and with none): mpc_episodes_run's rejections
    for obs, n in ((ok, 1), (None, 0)):
        for kw in (dict(state=None), dict(n_robots=0), dict(n_robots=65536), dict(n_steps=0),
                   dict(n_steps=abi.MPC_MAX_STEPS + 1), dict(max_calls=-1), dict(cap=-1),
                   dict(log=fake, cap=0), dict(integ=7), dict(max_calls=0)):
            base = L.mpc_episodes_run(
                kw.get("state", fake), kw.get("n_robots", 1), kw.get("n_steps", 3),
                kw.get("integ", 0), kw.get("max_calls", 1), kw.get("log"), kw.get("cap", 0), None,
                None)
            assert run(obs, n, **kw) == base, kw
            assert base == (abi.MPC_OK if kw == dict(max_calls=0) else
                            abi.MPC_ERR_UNSUPPORTED if "integ" in kw else abi.MPC_ERR_ARG), kw
    # an argument error outranks the unsupported mode, as in the base entry
    assert run(ok, 1, n_steps=0, integ=7) == abi.MPC_ERR_ARG
    assert run(ok, 1, max_calls=0) == abi.MPC_OK


def test_python_layer_refuses_more_than_sixteen_circles():
    """DeviceEpisodes.set_obstacles: ValueError before anything is allocated
    for them (no device needed: the method reads no state)."""
    from diplomjourney_amd.device_episodes import DeviceEpisodes
    eps = DeviceEpisodes.__new__(DeviceEpisodes)
    with pytest.raises(ValueError):
        eps.set_obstacles([(0.0, 0.0, 1.0)] * (abi.MPC_MAX_OBSTACLES + 1))
    with pytest.raises(ValueError):
        eps.set_obstacles([(0.0, 0.0)])
    eps.set_obstacles([(0.0, 0.0, 1.0)] * abi.MPC_MAX_OBSTACLES)
    assert eps._n_obs == 16
    eps.set_obstacles(())
    assert eps._n_obs == 0 and eps._obstacle_args() is None


def test_radius_on_the_lattice_has_no_margin():
    """Why the radii are what they are: with the base configuration a radius
    of 0.02 around a candidate's final state has another state on its rim."""
    V, B, states, _ = RC.first_step(RC.base_cfg(), 3, "rect+cum")
    ka = (len(V) // 2) * len(B) + len(B) // 2
    centre = (float(states[-1, 0, ka]), float(states[-1, 1, ka]))
    assert ranking.blocked(states, [(*centre, 0.02)])[1] < ranking.MARGIN
    assert ranking.blocked(states, [(*centre, 0.0213)])[1] > ranking.MARGIN


# the shapes of MATRIX_A, one model run each (4 and 16 circles share one)
SHAPES = sorted({(m, N, L, n == 1) for m, N, L, n in OC.MATRIX_A})
TABLE = {("rect+cum", 3, 0.5): 314, ("qk21", 3, 0.5): 314, ("rect+cum", 4, 0.3): 232}


@pytest.mark.parametrize("integ,n_steps,L,one", SHAPES)
def test_case_a_preconditions(integ, n_steps, L, one):
    """OC.check_case_a on the IEEE replica, over all six steps; the blocked
    candidates of the first step where the issue tabulated them; the fillers
    change no mask (OM asserts it per step); the counts against a recount."""
    case = OC.case_a(integ, n_steps, L, one)
    models, recs, first = OC.model_run(case, device=False)
    mask = OC.check_case_a(case, models, first)
    if not one and (integ, n_steps, L) in TABLE:
        assert int(mask.sum()) == TABLE[(integ, n_steps, L)]
    assert [rr[0]["index"] for c, rr in enumerate(recs) if not mask[c]] == list(
        np.flatnonzero(~mask))
    assert OC.table(case, 1 if one else 16)[:len(case["circles"])] == list(case["circles"])
    for M in models[::61]:
        assert M.blocked_steps == [int(m.sum()) for m, _ in M.masks]


@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_case_b_preconditions(integ, n_steps):
    case = OC.case_b(integ, n_steps)
    models, recs, _ = OC.model_run(case, device=False)
    OC.check_case_b(case, models, recs)


@pytest.mark.parametrize("integ,L", (("rect+cum", 0.5), ("rect+cum", 0.45), ("qk21", 0.5)))
def test_case_c_preconditions(integ, L):
    case = OC.case_c(integ, L)
    models, recs, _ = OC.model_run(case, device=False)
    OC.check_case_c(case, models, recs)
    assert sum(case["launches"]) == 40 and max(M.calls for M in models) > 5
    want = OM.launch_counts(models, case["launches"])
    assert sum(int(w.sum()) for w in want) == sum(sum(M.blocked_steps) for M in models)
    assert all((w >= 0).all() for w in want) and int(want[1].sum()) > 0


@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_edge_preconditions(integ):
    for make in (OC.case_all_blocked, OC.case_start_inside, OC.case_clamped, OC.case_single,
                 OC.case_schedule):
        case = make(integ)
        models, recs, _ = OC.model_run(case, device=False)
        assert models[0].margin > OC.MARGIN, (case["name"], models[0].margin)
    M = OC.model_run(OC.case_all_blocked(integ), False)[0][0]
    assert M.blocked_steps == [549, 549] and M.candidates == 1098 and M.stop & abi.MPC_EP_BREAK
    M = OC.model_run(OC.case_single(integ), False)[0][0]
    assert M.blocked_steps == [0, 0, 1, 1]
    M = OC.model_run(OC.case_clamped(integ), False)[0][0]
    assert M.sizes[0] == (64, 64) and 0 < M.blocked_steps[0] < 4096
    M = OC.model_run(OC.case_schedule(integ), False)[0][0]
    assert sum(M.blocked_steps) > 0 and M.calls == 10
    M = OC.model_run(OC.case_start_inside(integ), False)[0][0]
    assert 0 < M.blocked_steps[0] < 549


def test_model_counts_against_a_direct_recount():
    """The model's blocked count of a step against a loop over candidates,
    steps and circles with the header's formula, and no circles against the
    plain model: the same records."""
    case = OC.case_c("qk21", 0.5)
    cfg = case["cfgs"][1]
    M = OM.ObstacleRobotModel(cfg, 3, "qk21", case["circles"])
    P = RM.RobotModel(cfg, 3, "qk21")
    Z = OM.ObstacleRobotModel(cfg, 3, "qk21", ())
    with harness.estimates_installed(np.zeros(0), False):
        for _ in range(8):
            V, B, _g = M.grids()
            v, b = RM.enumerate_controls(V, B, 3)
            states, _c = harness.replica_rollout(_problem(M), v, b, "qk21", device_consts=True)
            n = 0
            for c in range(states.shape[2]):
                inside = False
                for s in range(3):
                    for cx, cy, r in case["circles"]:
                        dx, dy = states[s, 0, c] - cx, states[s, 1, c] - cy
                        inside |= dx * dx + dy * dy < r * r
                n += int(inside)
            M.mpc_step()
            assert M.blocked_steps[-1] == n
            assert Z.mpc_step() == P.mpc_step()
    assert sum(M.blocked_steps) > 0 and Z.blocked_steps == [0] * 8


def _problem(M):
    """The step's problem without advancing the model: begin_step on a copy."""
    import copy
    return copy.deepcopy(M).begin_step()[0]
