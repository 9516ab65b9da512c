"""Keep-out circles in the full tree, without a GPU: the three entries'
declarations and table checks (fake device pointers: every call returns before
any HIP call), the model of tests/fulltree_obstacle_cases.py against a plain
triple-loop scan, the shard counts, and the scenes' own stated conditions on
the IEEE replica (tests/test_fulltree_obstacles_gpu.py runs them on the device)."""
import ctypes
import math

import numpy as np
import pytest

import fulltree_cases as F
import fulltree_obstacle_cases as FO
import obstacle_cases
from diplomjourney_amd import abi, native

ENTRIES = ("mpc_fulltree_argmin_obstacles", "mpc_fulltree_argmin_batched_obstacles",
           "mpc_fulltree_episodes_run_obstacles")
_P = ctypes.c_void_p


def test_exports_declared_and_present():
    header = open(native.HEADER).read()
    so = ctypes.CDLL(native.LIB_PATH)
    for name in ENTRIES:
        assert name in native.EXPORTS and name in native.PROTOTYPES
        assert name + "(" in header
        getattr(so, name)
        # the plain twin's arguments + (circles, count) + n_blocked_out
        base = native.PROTOTYPES[name.replace("_obstacles", "")][1]
        assert len(native.PROTOTYPES[name][1]) == len(base) + 3
    assert "the full tree take no obstacles" not in " ".join(header.split())


def _calls():
    """{entry: call(circles, count, **overrides)} over fake pointers; every
    default is an acceptable argument, so a call without a fault would launch."""
    L = native.lib()
    p = F.problem("move")
    f, g = _P(0x1000), _P(0x2000)
    rect = abi.INTEGRATORS["rect"]

    def one(obs, n, integ=rect, wsb=1 << 24):
        return L.mpc_fulltree_argmin_obstacles(ctypes.byref(p), obs, n, f, 3, g, 3, math.inf,
                                               integ, 0, 1, f, wsb, None, f, None)

    def batched(obs, n, integ=rect, wsb=1 << 24):
        return L.mpc_fulltree_argmin_batched_obstacles(f, obs, n, g, 4, 0.5, 0.1, 0.15, f, 3, g,
                                                       3, integ, f, wsb, None, f, None)

    def episodes(obs, n, integ=rect, wsb=0, max_calls=2):
        return L.mpc_fulltree_episodes_run_obstacles(f, obs, n, 4, f, 3, g, 3, 0.5, 0.05, 1e-3,
                                                     integ, max_calls, None, 0, None, None, None)

    return {"argmin": one, "batched": batched, "episodes": episodes}


def test_table_faults_without_gpu():
    """Every table fault is MPC_ERR_ARG with otherwise acceptable arguments
    (fake pointers: a call that got past the check would fault or report a HIP
    error), also when other arguments are wrong as well."""
    bad = obstacle_cases.rejected_circles()
    assert len(bad) == 17
    for name, call in _calls().items():
        for what, (obs, n) in bad.items():
            assert call(obs, n) == abi.MPC_ERR_ARG, (name, what)
            assert call(obs, n, integ=7, wsb=8) == abi.MPC_ERR_ARG, (name, what)


def test_other_rejections_are_the_plain_entries():
    """With a valid table the plain entry's checks answer, in its order."""
    ok = abi.make_obstacles([(1.0, 2.0, 0.5)])
    calls = _calls()
    cum = abi.INTEGRATORS["rect+cum"]
    assert calls["argmin"](*ok, integ=cum) == abi.MPC_ERR_UNSUPPORTED
    assert calls["batched"](*ok, integ=cum) == abi.MPC_ERR_UNSUPPORTED
    assert calls["argmin"](*ok, wsb=8) == abi.MPC_ERR_WORKSPACE
    assert calls["batched"](*ok, wsb=8) == abi.MPC_ERR_WORKSPACE
    assert calls["episodes"](*ok, integ=cum) == abi.MPC_ERR_UNSUPPORTED
    assert calls["episodes"](*ok, max_calls=-1) == abi.MPC_ERR_ARG


@pytest.mark.parametrize("scene", ["pair", "graze", "start_inside", "nan"])
@pytest.mark.parametrize("s1", [5, 9])
def test_model_equals_the_plain_scan(s1, scene):
    """model() + expected_records() + shard_counts() against the triple loop,
    every shard of every split of the sweep."""
    c, circles = FO.scene_case(scene, s1, "rect")
    m = FO.model(c, circles)
    for n in F.sweep(s1):
        leaf, cost, _ = F.expected_records(m.minima, n)
        counts = FO.shard_counts(m.unit_blocked, n)
        for s in range(n):
            want = FO.scan_model(c, circles, s, n)
            assert (int(leaf[s]), float(cost[s]), int(counts[s])) == want, (n, s)


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("s1", FO.SMALL + FO.LARGE)
def test_shard_counts_sum_to_the_trees(s1, mode):
    """The shards' counts of any n_shards sum to the tree's, which is the
    number of blocked leaves (clamped lanes count nothing)."""
    c, circles = FO.scene_case("start_inside", s1, mode)
    m = FO.model(c, circles)
    total = int(m.blocked.sum())
    assert int(m.unit_blocked.sum()) == total
    for n in FO.n_list(s1):
        assert int(FO.shard_counts(m.unit_blocked, n).sum()) == total


@pytest.mark.parametrize("mode", ["qk21", "rect+rot"])
@pytest.mark.parametrize("s1", FO.SMALL + FO.LARGE)
def test_scenes_meet_their_conditions(s1, mode):
    """Each scene's margin (model() asserts it) and what it is there for."""
    moving = F.SHAPES[s1][0] > 1                 # (S1 = 5 has the speed 0 alone)
    n = s1 ** 3
    for name in FO.SCENES:
        c, circles = FO.scene_case(name, s1, mode)
        m = FO.model(c, circles)
        nb = int(m.blocked.sum())
        assert len(circles) <= abi.MPC_MAX_OBSTACLES
        if name == "subtree" and moving:         # all S1^2 leaves of k0 = S1 - 1, not the tree
            assert m.blocked[(s1 - 1) * s1 * s1:].all() and nb < n
        if name == "pair" and moving:            # whole pairs, fewer than a subtree
            pair = ((s1 - 1) * s1 + s1 // 2) * s1
            assert m.blocked[pair:pair + s1].all() and s1 <= nb < s1 * s1
        if name == "graze" and moving:
            (near, only2), (far_near, far_hit) = FO.reach_kinds(c, circles)
            assert near and 1 <= only2 <= 4 * s1     # within reach, a few k2 enter
            assert not far_near and far_hit == 0     # within reach of no layer-1 state
            assert m.blocked[n - 1]
        if name == "all":
            assert nb == n
            assert (F.expected_records(m.minima, 3)[0] == -1).all()
        if name == "start_inside":
            (cx, cy, r), = circles
            assert math.hypot(c.problem.x - cx, c.problem.y - cy) < r
            assert (0 < nb < n) if moving else nb == n
        if name == "far16":
            assert len(circles) == 16 and nb == 0
            assert not any(near for near, _ in FO.reach_kinds(c, circles))
        if name == "nan":
            assert np.isnan(c.costs).any()
            assert not m.blocked[np.isnan(m.states[:, 0, 0])].any()   # NaN from layer 0 on


def test_peel_ranks_sixteen_winners():
    """Sixteen rounds of the ranking scene on the replica: every round's circle
    blocks the current winner, and the winners' costs never decrease."""
    c = F.case(14, "move", "rect")
    circles, costs = [], []
    for _ in range(FO.PEEL_ROUNDS):
        m = FO.model(c, circles)
        leaf, cost, _ = F.expected_records(m.minima, 1)
        assert leaf[0] >= 0
        costs.append(float(cost[0]))
        circles.append(FO.peel_next(m))
        assert FO.model(c, circles).blocked[leaf[0]]
    assert costs == sorted(costs) and len(circles) == FO.PEEL_ROUNDS
