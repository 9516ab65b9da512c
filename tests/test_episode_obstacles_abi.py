"""Keep-out circles in the device-resident episode steps, without a GPU: the
three entries' declarations and argument checks (fake device pointers: every
call returns before any HIP call), the frame function of rect+cum on the host,
and the preconditions of the GPU cases (tests/test_episode_obstacles_gpu.py)
on the IEEE replica."""
import ctypes
import math

import numpy as np
import pytest

import episode_obstacle_cases as EC
import harness
import obstacle_cases
import ranking as R
from diplomjourney_amd import abi, native

ENTRIES = ("mpc_episode_partials_obstacles", "mpc_episode_step_obstacles",
           "mpc_episode_chain_step_obstacles")
_P = ctypes.c_void_p


def test_exports_declared_and_present():
    header = open(native.HEADER).read()
    so = ctypes.CDLL(native.LIB_PATH)
    for name in ENTRIES:
        assert name in native.EXPORTS and name in native.PROTOTYPES
        assert name + "(" in header
        getattr(so, name)
    # the base entry's arguments + (circles, count) + n_blocked_out
    for name in ENTRIES:
        base = native.PROTOTYPES[name.replace("_obstacles", "")][1]
        assert len(native.PROTOTYPES[name][1]) == len(base) + 3


def _circles(rows):
    return abi.make_obstacles(rows)


def _calls():
    """{entry: (obstacle call, base call)}(**overrides) over fake pointers; every
    default is an acceptable argument, so a call without a fault would launch."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    cfg = reference_episode_config()
    f, g = _P(0x1000), _P(0x2000)
    base = dict(cfg=cfg, state=f, v=f, b=g, n=1024, ns=10, base=0,
                integ=abi.INTEGRATORS["rect+cum"], ws=f, wsb=1 << 24, out=f, log=f, cap=8,
                epoch=3, mode=1, ws_prev=f, v_prev=None, b_prev=None, advance=None, nb=None)

    def ref(c):
        return ctypes.byref(c) if c is not None else None

    def partials(a, obs):
        head = (a["state"],) + obs
        tail = (a["v"], a["b"], a["n"], a["ns"], a["integ"], a["ws"], a["wsb"])
        if obs:
            return L.mpc_episode_partials_obstacles(*head, *tail, a["nb"], None)
        return L.mpc_episode_partials(*head, *tail, None)

    def step(a, obs):
        head = (a["state"],) + obs
        tail = (a["v"], a["b"], a["n"], a["ns"], a["base"], a["integ"], a["ws"], a["wsb"], a["out"],
                ref(a["advance"]), a["log"], a["cap"])
        if obs:
            return L.mpc_episode_step_obstacles(*head, *tail, a["nb"], None)
        return L.mpc_episode_step(*head, *tail, None)

    def chain(a, obs):
        head = (ref(a["cfg"]), a["state"]) + obs
        tail = (a["mode"], a["epoch"], a["v"], a["b"], a["n"], a["ns"], a["base"], a["integ"],
                a["ws"], a["ws_prev"], a["wsb"], a["v_prev"], a["b_prev"], a["out"], None, 0,
                a["log"], a["cap"])
        if obs:
            return L.mpc_episode_chain_step_obstacles(*head, *tail, a["nb"], None)
        return L.mpc_episode_chain_step(*head, *tail, None)

    def entry(fn):
        return lambda obs, **kw: fn({**base, **kw}, obs)

    return {"partials": entry(partials), "step": entry(step), "chain_step": entry(chain)}


def test_obstacle_rejections_without_gpu():
    """Every obstacle rejection is MPC_ERR_ARG with otherwise acceptable
    arguments (fake pointers: a call that got past the check would fault or
    report a HIP error), also when the base arguments are wrong as well."""
    bad = obstacle_cases.rejected_circles()
    assert len(bad) == 17
    for name, call in _calls().items():
        for what, obs in bad.items():
            assert call(obs) == abi.MPC_ERR_ARG, (name, what)
            assert call(obs, integ=7, wsb=8) == abi.MPC_ERR_ARG, (name, what)


def test_base_rejections_match_the_base_entries_without_gpu():
    """With valid circles (and with none) every rejection is the base entry's
    own: the same status for the same wrong call."""
    f, odd = _P(0x1000), _P(0x2008)
    cum = abi.INTEGRATORS["rect+cum"]
    from diplomjourney_amd.episode import reference_episode_config
    bad_cfg = reference_episode_config()
    bad_cfg.stop_rule = 2
    common = [dict(state=None), dict(v=None), dict(b=None), dict(n=0), dict(ns=0), dict(ns=33),
              dict(integ=7), dict(integ=cum | 0x800), dict(ws=None), dict(wsb=8),
              dict(ns=0, integ=7), dict(integ=7, wsb=8)]
    rows = {
        "partials": common + [dict(integ=cum | abi.MPC_LAYOUT_TILED)],
        "step": common,
        "chain_step": common + [
            dict(epoch=0), dict(mode=2), dict(mode=0), dict(integ=1), dict(b=odd), dict(cap=-1),
            dict(base=-1), dict(cfg=bad_cfg), dict(cfg=None), dict(n=1023),
            dict(v_prev=f, b_prev=None), dict(v_prev=f, b_prev=None, wsb=8),
            dict(v_prev=f, b_prev=odd), dict(b=odd, wsb=8)],
    }
    circles = _circles([(1.0, 2.0, 0.5), (-3.0, 0.5, 0.25)])
    statuses = set()
    for name, call in _calls().items():
        for kw in rows[name]:
            want = call((), **kw)
            assert want != abi.MPC_OK, (name, kw)
            shown = {k: getattr(v, "value", v) for k, v in kw.items() if k != "cfg"}
            assert call(circles, **kw) == want, (name, shown)
            assert call((None, 0), **kw) == want, (name, shown)
            statuses.add(want)
    assert statuses == {abi.MPC_ERR_ARG, abi.MPC_ERR_UNSUPPORTED, abi.MPC_ERR_WORKSPACE}


# ----------------------------------------------------------------------------
# the frame function on the host
# ----------------------------------------------------------------------------
def _frame_lib():
    L = harness.host_lib("frame_harness")
    L.frame_consts.argtypes = [ctypes.POINTER(abi.MpcProblem), _P]
    L.frame_circles.argtypes = [ctypes.POINTER(abi.MpcProblem), _P, ctypes.c_int, _P]
    L.frame_cum_pose.argtypes = [ctypes.POINTER(abi.MpcProblem), _P, ctypes.c_int, _P]
    L.frame_tables.argtypes = [ctypes.POINTER(abi.MpcProblem), _P, ctypes.c_int, _P, _P]
    return L


def _tables(lib, p, circles):
    """The library's own builder (world_obstacles / frame_obstacles,
    csrc/mpc_host_consts.h) on the rows (x, y, r): the world and the rect+cum
    loop table, all 16 entries (cx, cy, r2) of each."""
    obs, n = abi.make_obstacles([tuple(c) for c in circles])
    world, loop = np.full((16, 3), np.nan), np.full((16, 3), np.nan)
    lib.frame_tables(ctypes.byref(p), obs, n, world.ctypes.data_as(_P), loop.ctypes.data_as(_P))
    return world, loop


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("L", R.WHEELBASES)
def test_frame_circle_on_the_host(L):
    """frame_circle (csrc/mpc_device.h), the table the rect+cum kernels form
    from the episode's pose: its numbers are the frame formula's, the tables
    the library's builder makes (frame_obstacles, the one-shot entries' `loop`
    table) are that formula on the bits, padding included, and a point of the
    sums frame is inside the transformed circle exactly when its cum_pose is
    inside the world circle."""
    lib = _frame_lib()
    rng = np.random.default_rng(20261020)
    headings = (0.7, 2.3, -2.4, -0.6, 3.9, 5.8, 0.0, math.pi / 2)   # every quadrant
    n_in = n_out = 0
    for k, phi in enumerate(headings):
        pose = (float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), phi)
        p = R.problem(L, pose)
        K = np.zeros(7)
        lib.frame_consts(ctypes.byref(p), K.ctypes.data_as(_P))
        x0, y0, s0, c0, inv_L, pow2 = (float(q) for q in K[:6])
        assert bool(pow2) == (L == 0.5) and (inv_L == 2.0 if pow2 else inv_L == 0.0)
        world = np.column_stack([pose[0] + rng.uniform(-1, 1, 16), pose[1] + rng.uniform(-1, 1, 16),
                                 rng.uniform(0.02, 0.6, 16)])
        got = np.zeros((16, 3))
        lib.frame_circles(ctypes.byref(p), world.ctypes.data_as(_P), 16, got.ctypes.data_as(_P))
        # the frame formula, operation for operation
        sc = inv_L if pow2 else 1.0
        wants = []
        for (wx, wy, wr), g in zip(world.tolist(), got.tolist()):
            dx, dy, r = wx - x0, wy - y0, wr * sc
            want = [(c0 * dx + s0 * dy) * sc, (c0 * dy - s0 * dx) * sc, r * r]
            assert g == want, (k, g, want)
            wants.append(want)
        # the tables the entries launch with: that formula, the world circles
        # as given and r2 = -1 past the count, on the bits
        for n in (0, 1, 4, 5, 16):
            tw, tl = _tables(lib, p, world[:n])
            pad = [[0.0, 0.0, -1.0]] * (16 - n)
            want_w = [[wx, wy, wr * wr] for wx, wy, wr in world[:n].tolist()] + pad
            assert (_bits(tw) == _bits(want_w)).all(), (k, n)
            assert (_bits(tl) == _bits(wants[:n] + pad)).all(), (k, n)
        # points of the sums frame around every circle: near its rim and anywhere
        for (wx, wy, wr), (cx, cy, r2) in zip(world.tolist(), got.tolist()):
            m = 400
            rad = math.sqrt(r2) * np.concatenate([rng.uniform(0.0, 2.0, m // 2),
                                                  1.0 + rng.uniform(-1e-6, 1e-6, m // 2)])
            ang = rng.uniform(0, 2 * math.pi, m)
            ab = np.ascontiguousarray(np.column_stack([cx + rad * np.cos(ang),
                                                       cy + rad * np.sin(ang)]))
            xy = np.zeros_like(ab)
            lib.frame_cum_pose(ctypes.byref(p), ab.ctypes.data_as(_P), m, xy.ctypes.data_as(_P))
            d = np.hypot(xy[:, 0] - wx, xy[:, 1] - wy)
            clear = np.abs(d - wr) >= 1e-9
            inside_world = (xy[:, 0] - wx) ** 2 + (xy[:, 1] - wy) ** 2 < wr * wr
            da, db = ab[:, 0] - cx, ab[:, 1] - cy
            inside_frame = db * db + da * da < r2
            assert (inside_world == inside_frame)[clear].all(), k
            n_in += int((inside_world & clear).sum())
            n_out += int((~inside_world & clear).sum())
    assert n_in > 1000 and n_out > 1000


def test_frame_radius_is_the_scaled_radius_squared():
    """frame_obstacles forms r2 as r^2 * sc^2 (frame_circle), the one-shot
    entries formed (r * sc)^2 before they shared it: the same bits for every
    radius whose squares are normal numbers (include/mpc_rollout.h), with the
    scale of a power-of-two wheelbase (1/L) and without one."""
    lib = _frame_lib()
    rng = np.random.default_rng(20261020)
    radii = np.concatenate([np.logspace(-140, 140, 60), rng.uniform(0.02, 0.6, 16)])
    for L in R.WHEELBASES + (0.3, 4.0):      # 0.45, 0.3: no scale; 0.5, 4.0: 2 and 1/4
        p = R.problem(L, (0.4, -1.3, 0.7))
        K = np.zeros(7)
        lib.frame_consts(ctypes.byref(p), K.ctypes.data_as(_P))
        pow2 = bool(K[5])
        assert pow2 == (L in (0.5, 4.0))
        sc = float(K[4]) if pow2 else 1.0
        assert sc == (1.0 / L if pow2 else 1.0)
        for at in range(0, len(radii), 16):
            rs = radii[at:at + 16]
            _, loop = _tables(lib, p, [(0.1 * i, -0.2 * i, r) for i, r in enumerate(rs.tolist())])
            want = [(r * sc) * (r * sc) for r in rs.tolist()]
            assert (_bits(loop[:len(rs), 2]) == _bits(want)).all(), (L, at)


# ----------------------------------------------------------------------------
# the GPU cases' preconditions, on the IEEE replica
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,L,n_steps,n", EC.FIRST_STEP)
def test_first_step_preconditions(mode, L, n_steps, n):
    inp, st, costs = EC.first_step(mode, L, n_steps, n, device=False)
    assert R.check_preconditions(inp, costs) == n - 3
    for k, (circ, mask) in EC.masked(st, costs, n_steps, EC.counts_of(n)).items():
        assert len(circ) == k
        # something is left to rank, and an irregular candidate is among the blocked or the free
        assert (np.isfinite(costs) & ~mask).sum() > 100


@pytest.mark.parametrize("L,n_steps", EC.SECOND_STEP)
def test_second_step_preconditions(L, n_steps):
    """The chained cases, with step A's winner from the IEEE replica (the GPU
    cases rebuild step B's problem from step A's log record and assert the same)."""
    traj_a, pose = EC.batch_a_winner(L, n_steps, device=False)
    inp = R.controls(n_steps)
    st, costs = harness.replica_rollout(R.problem_after(pose, L), inp.v, inp.b, "rect+cum",
                                        device_consts=True)
    assert R.check_preconditions(inp, costs) == inp.n - 3
    for k, (circ, mask) in EC.masked(st, costs, n_steps, (4, 16)).items():
        EC.a_unblocked(traj_a, circ)


def test_grid_shape_preconditions():
    """The chained case at ranking.BIG_N candidates (4 circles, the first 8 ranked)."""
    va, ba = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[0])
    traj_a, pose = EC.batch_a_winner(0.5, R.BIG_STEPS, device=False, batch=(va, ba))
    v, b = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[1])
    st, costs = harness.replica_rollout(R.problem_after(pose, 0.5), v, b, "rect+cum",
                                        device_consts=True)
    circ, mask = EC.masked(st, costs, R.BIG_STEPS, (4,), EC.big_circles(st, costs))[4]
    EC.a_unblocked(traj_a, circ)
    free = costs[np.isfinite(costs) & ~mask]
    assert len(free) >= 8 and len(np.unique(np.sort(free)[:9])) == 9   # no tie among the ranked
