"""The fleet call (mpc_episodes_fleet_begin / _run) without a GPU: what the
entries reject before any HIP call, the board's size, the model's neighbour
selection (tests/fleet_model.py) against an independent sort on exact
arithmetic, and DeviceFleet's default reach against its formula."""
import math
import random
from fractions import Fraction

import numpy as np

import fleet_model as FM
import robots_cases as RC
from diplomjourney_amd import abi, native
from diplomjourney_amd.device_episodes import fleet_reach
from fleet_cases import FAKE, LATTICE as lattice, circles as _circles, fleet_run as _run


def test_rejections_before_any_hip_call():
    """The fleet's own arguments first (the circle checks of
    mpc_rollout_partials_obstacles, clearance, reach, call0, n_calls, the
    board), each MPC_ERR_ARG whatever else is wrong; with valid fleet
    arguments mpc_episodes_run's rejections, status for status; n_calls == 0
    launches nothing."""
    L = native.lib()
    ok = _circles((0.0, 0.0, 1.0))
    assert _run(L, ok, -1) == abi.MPC_ERR_ARG
    assert _run(L, _circles(*[(0.0, 0.0, 1.0)] * 17), 17) == abi.MPC_ERR_ARG
    assert _run(L, None, 1) == abi.MPC_ERR_ARG
    for bad in ((math.nan, 0.0, 1.0), (0.0, math.inf, 1.0), (0.0, -math.inf, 1.0), (0.0, 0.0, 0.0),
                (0.0, 0.0, -1.0), (0.0, 0.0, math.nan), (0.0, 0.0, math.inf)):
        assert _run(L, _circles((1.0, 1.0, 0.5), bad), 2) == abi.MPC_ERR_ARG, bad
    for kw in (dict(clearance=0.0), dict(clearance=-0.1), dict(clearance=math.nan),
               dict(clearance=math.inf), dict(reach=-1e-300), dict(reach=math.nan),
               dict(reach=math.inf), dict(reach=-math.inf), dict(call0=-1), dict(n_calls=-1),
               dict(board=None)):
        assert _run(L, ok, 1, **kw) == abi.MPC_ERR_ARG, kw
        assert _run(L, **kw) == abi.MPC_ERR_ARG, kw
        # a fleet argument error outranks the unsupported mode and n_calls == 0
        assert _run(L, ok, 1, integ=7, **kw) == abi.MPC_ERR_ARG, kw
        if "n_calls" not in kw:
            assert _run(L, ok, 1, n_calls=0, **kw) == abi.MPC_ERR_ARG, kw
    assert _run(L, _circles((0.0, 0.0, 0.0)), 1, integ=7) == abi.MPC_ERR_ARG
    # reach = 0 and a large call0 are valid
    assert _run(L, reach=0.0, n_calls=0, call0=2 ** 40 + 1) == abi.MPC_OK
    # with valid fleet arguments: mpc_episodes_run's rejections, in its order
    for obs, n in ((ok, 1), (None, 0)):
        for kw in (dict(state=None), dict(n_robots=0), dict(n_robots=65536), dict(n_steps=0),
                   dict(n_steps=abi.MPC_MAX_STEPS + 1), dict(cap=-1), dict(log=FAKE, cap=0),
                   dict(integ=7), dict(n_calls=0)):
            base = L.mpc_episodes_run(
                kw.get("state", FAKE), kw.get("n_robots", 1), kw.get("n_steps", 3),
                kw.get("integ", 0), kw.get("n_calls", 1), kw.get("log"), kw.get("cap", 0), None,
                None)
            assert _run(L, obs, n, **kw) == base, kw
            assert base == (abi.MPC_OK if kw == dict(n_calls=0) else
                            abi.MPC_ERR_UNSUPPORTED if "integ" in kw else abi.MPC_ERR_ARG), kw
    assert _run(L, ok, 1, n_steps=0, integ=7) == abi.MPC_ERR_ARG


def test_begin_rejections_and_board_bytes():
    L = native.lib()
    assert L.mpc_episodes_fleet_begin(None, 1, FAKE, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_fleet_begin(FAKE, 1, None, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_fleet_begin(FAKE, 0, FAKE, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_fleet_begin(FAKE, 65536, FAKE, None) == abi.MPC_ERR_ARG
    # two sides of n positions, 16 B per robot per side
    assert [L.mpc_episodes_fleet_board_bytes(n) for n in (-1, 0, 1, 6, 549, 65535)] == [
        0, 0, 32, 192, 2 * 549 * 16, 2 * 65535 * 16]


def _exact_d2(pr, pq):
    """fma(dy, dy, dx * dx) with dx, dy the rounded differences: the product
    rounded once, the fused step once, on exact rationals."""
    dx, dy = pq[0] - pr[0], pq[1] - pr[1]            # (float subtraction: one rounding each)
    xx = float(Fraction(dx) * Fraction(dx))          # dx * dx, rounded
    return float(Fraction(dy) * Fraction(dy) + Fraction(xx))


def _independent(pos, r, reach, keep):
    rows = sorted((_exact_d2(pos[r], pos[q]), q) for q in range(len(pos)) if q != r)
    near = [(d, q) for d, q in rows if d < reach * reach]
    return len(near), [q for _, q in near[:keep]]


def test_selection_against_an_independent_sort():
    """fleet_model.select on the host build's d2 against a sort of exactly
    rounded d2: random clouds (more and fewer than the cap within reach, every
    cap 0..16), and a lattice of exactly representable positions where d2 ties
    at the cap's boundary (the lower index wins) and one robot sits at exactly
    d2 == reach * reach (strict <: not a neighbour)."""
    rng = random.Random(20261021)
    for n, spread, reach in ((1, 1.0, 0.5), (2, 0.1, 0.5), (7, 1.0, 0.4), (20, 0.2, 0.5),
                             (40, 1.0, 0.3), (300, 1.0, 0.25)):
        pos = [(rng.uniform(-spread, spread), rng.uniform(-spread, spread)) for _ in range(n)]
        for r in range(0, n, max(1, n // 7)):
            d2 = FM.d2_row(pos, r)
            assert [float(v) for v in d2] == [_exact_d2(pos[r], p) for p in pos]
            for keep in (0, 1, 13, 16):
                within, chosen, _, _ = FM.select(d2, r, reach, keep)
                assert (within, chosen) == _independent(pos, r, reach, keep), (n, r, keep)
    d2 = FM.d2_row(lattice, 0)
    assert d2[19] == 0.25 * 0.25
    within, chosen, edge, gap = FM.select(d2, 0, 0.25, 13)
    assert within == 18 and 19 not in chosen and edge == 0.0 and gap == 0.0
    assert (within, chosen) == _independent(lattice, 0, 0.25, 13)
    order = sorted(range(1, 19), key=lambda q: (d2[q], q))
    assert d2[order[12]] == d2[order[13]] and order[12] < order[13] and chosen[-1] == order[12]
    # reach 0: nobody, whatever the cap
    assert FM.select(d2, 0, 0.0, 16)[:2] == (0, [])


def test_default_reach_is_its_formula():
    """fleet_reach: max over the cfgs of n_steps * delta_t * max(|v_max|,
    |v_min|), times (1 + 2**-40), plus clearance — and the farthest step-end
    state of a first step is inside it."""
    slow = RC.base_cfg()
    fast = RC.base_cfg(v_max=1.5, delta_t=0.2)
    back = RC.base_cfg(v_max=0.5, v_min=-2.0)
    assert fleet_reach([slow], 3, 0.07) == 3 * 0.1 * 1.0 * (1.0 + 2.0 ** -40) + 0.07
    assert fleet_reach([slow, fast, slow], 4, 0.0) == 4 * 0.2 * 1.5 * (1.0 + 2.0 ** -40)
    assert fleet_reach([back, slow], 2, 0.01) == 2 * 0.1 * 2.0 * (1.0 + 2.0 ** -40) + 0.01
    for integ in ("qk21", "rect+cum"):
        _, _, states, _ = RC.first_step(slow, 3, integ)
        far = np.nanmax(np.hypot(states[:, 0, :] - RC.START[0], states[:, 1, :] - RC.START[1]))
        assert far <= fleet_reach([slow], 3, 0.0)
