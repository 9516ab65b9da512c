"""The keep-out polygon tables on the host (tests/polygon_harness.cpp, a host
build of csrc/mpc_keepout.h): the world table's and the rect+cum frame table's
predicate against the numpy rule of polygon_cases, on a case's oracle states.
No GPU."""
import ctypes

import numpy as np
import pytest

import harness
import polygon_cases as pc
from diplomjourney_amd import abi

_P = ctypes.c_void_p
SLOTS = abi.MPC_MAX_POLYGONS * abi.MPC_MAX_POLYGON_VERTICES


@pytest.fixture(scope="module")
def H():
    L = harness.host_lib("polygon_harness")
    L.poly_check.argtypes = [_P, ctypes.c_int]
    L.poly_consts.argtypes = [ctypes.POINTER(abi.MpcProblem), _P]
    L.poly_tables.argtypes = [ctypes.POINTER(abi.MpcProblem), _P, ctypes.c_int, _P, _P]
    L.poly_inside.argtypes = [_P, ctypes.c_int, _P, ctypes.c_int64, _P]
    L.poly_cum_pose.argtypes = [ctypes.POINTER(abi.MpcProblem), _P, ctypes.c_int64, _P]
    return L


def _tables(H, p, polygons):
    arr, n = abi.make_polygons(polygons)
    assert H.poly_check(arr, n) == abi.MPC_OK
    world, loop = np.full((SLOTS, 3), np.nan), np.full((SLOTS, 3), np.nan)
    H.poly_tables(ctypes.byref(p), arr, n, world.ctypes.data_as(_P), loop.ctypes.data_as(_P))
    return world, loop


def _inside(H, table, n_poly, xy):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    out = np.full(len(xy), 7, dtype=np.uint8)
    H.poly_inside(table.ctypes.data_as(_P), n_poly, xy.ctypes.data_as(_P), len(xy),
                  out.ctypes.data_as(_P))
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def _points(c):
    """Every step-end state of the case as [n, 2], and the numpy rule on each."""
    x, y = c.states[:, 0, :].ravel(), c.states[:, 1, :].ravel()
    want = np.zeros(len(x), dtype=bool)
    for g in c.polygons:
        want |= pc.inside(x, y, g)
    return np.stack([x, y], axis=1), want


def _sums(H, p, xy):
    """The sums (A, B) — scaled by 1/L when L is a power of two — that cum_pose
    turns into the points, and a check that it does."""
    K = np.zeros(7)
    H.poly_consts(ctypes.byref(p), K.ctypes.data_as(_P))
    kx, ky, s0, c0, inv_l, pow2, _ = K
    dx, dy = xy[:, 0] - kx, xy[:, 1] - ky
    ab = np.stack([c0 * dx + s0 * dy, c0 * dy - s0 * dx], axis=1)
    if pow2:
        ab = ab * inv_l
    ab = np.ascontiguousarray(ab)
    back = np.empty_like(ab)
    H.poly_cum_pose(ctypes.byref(p), ab.ctypes.data_as(_P), len(ab), back.ctypes.data_as(_P))
    # far inside the cases' 1e-9 margin to every edge line
    assert np.abs(back - xy).max() < 1e-14
    return ab, bool(pow2)


@pytest.mark.parametrize("L,shape", [(0.5, (2178, 3)), (0.3, (2178, 3)), (0.3, (2177, 10))])
def test_world_and_frame_predicates_match_the_numpy_rule(H, oracle, L, shape):
    c = pc.case(shape[0], shape[1], "rect", L=L)
    pc.check_preconditions(c)
    xy, want = _points(c)
    assert 0 < want.sum() < len(want)
    world, loop = _tables(H, c.problem, c.polygons)
    assert np.array_equal(_inside(H, world, 4, xy), want)
    ab, scaled = _sums(H, c.problem, xy)
    assert scaled == (L == 0.5)
    assert np.array_equal(_inside(H, loop, 4, ab), want)
    # the frame table is another table: the sums are not the states
    assert not np.array_equal(world, loop)


def test_both_orientations_give_one_table(H, oracle):
    c = pc.case(2178, 3, "rect")
    flipped = [g[::-1] for g in c.polygons]
    for a, b in zip(_tables(H, c.problem, c.polygons), _tables(H, c.problem, flipped)):
        assert a.tobytes() == b.tobytes()
    # unit inner normals: the table's value is the signed distance
    world, _ = _tables(H, c.problem, c.polygons)
    used = world[(world[:, 0] != 0) | (world[:, 1] != 0)]
    assert len(used) == 8 + 3 + 4 + 5
    assert np.abs(np.hypot(used[:, 0], used[:, 1]) - 1.0).max() < 4e-16
    cx, cy = c.specs[0][0]
    assert np.abs(world[:8] @ np.array([cx, cy, 1.0])
                  - c.specs[0][1] * np.cos(np.pi / 8)).max() < 1e-15


@pytest.mark.parametrize("n_poly", [1, 4])
def test_padding_blocks_what_the_rule_blocks(H, oracle, n_poly):
    """Triangles in 8-edge slots, one polygon and four: every slot of the table
    evaluated (as a kernel instantiated for 4 polygons does), the unused edges
    true and the unused polygons false."""
    c = pc.case(2178, 3, "rect")
    reach = 0.05 * c.n_steps
    where = ((0.45, 0.2), (0.6, 0.35), (0.3, 0.3), (0.75, 0.3))     # (share of reach, heading)
    tris = [pc.ngon((q * reach * np.cos(h), q * reach * np.sin(h)), 0.08 * reach, 3, 1.0 + k,
                    cw=bool(k % 2)) for k, (q, h) in enumerate(where)][:n_poly]
    x, y = c.states[:, 0, :].ravel(), c.states[:, 1, :].ravel()
    want = np.zeros(len(x), dtype=bool)
    each = []
    for g in tris:
        each.append(pc.inside(x, y, g))
        want |= each[-1]
    assert all(q.any() for q in each) and not want.all()
    world, loop = _tables(H, c.problem, tris)
    xy = np.stack([x, y], axis=1)
    assert np.array_equal(_inside(H, world, abi.MPC_MAX_POLYGONS, xy), want)
    ab, _ = _sums(H, c.problem, xy)
    assert np.array_equal(_inside(H, loop, abi.MPC_MAX_POLYGONS, ab), want)
    # the padding itself: (0, 0, 1) in a used polygon, (0, 0, -1) in an unused one
    for t in (world, loop):
        t = t.reshape(abi.MPC_MAX_POLYGONS, abi.MPC_MAX_POLYGON_VERTICES, 3)
        assert (t[:n_poly, 3:, :2] == 0).all() and (t[:n_poly, 3:, 2] > 0).all()
        assert (t[n_poly:, :, :2] == 0).all() and (t[n_poly:, :, 2] < 0).all()


def test_nan_and_inf_points_are_inside_nothing(H, oracle):
    c = pc.case(2178, 3, "rect")
    cx, cy = c.specs[0][0]
    pts = np.array([[cx, cy], [np.nan, cy], [cx, np.nan], [np.nan, np.nan], [np.inf, cy],
                    [cx, -np.inf]])
    for polygons in (c.polygons, c.polygons[1:2]):          # full table, and a padded one
        for table in _tables(H, c.problem, polygons):
            got = _inside(H, table, abi.MPC_MAX_POLYGONS, pts)
            assert not got[1:].any()
    assert _inside(H, _tables(H, c.problem, c.polygons)[0], 4, pts)[0]


def test_check_polygons_is_the_entries_rule(H):
    for what, (arr, n) in pc.rejected_polygons().items():
        assert H.poly_check(arr, n) == abi.MPC_ERR_ARG, what
    assert H.poly_check(None, 0) == abi.MPC_OK
    ok = pc.polygons_array(pc.OK_POLYGON, pc.OK_POLYGON[::-1], pc.ngon((1e6, -1e6), 1e-3, 8, 0.1))
    assert H.poly_check(ok, 3) == abi.MPC_OK
