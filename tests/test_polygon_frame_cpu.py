"""The keep-out polygon tables on the host (tests/polygon_harness.cpp, a host
build of csrc/mpc_keepout.h): the world table's and the rect+cum frame table's
predicate against the numpy rule of polygon_cases, on a case's oracle states;
then, at every placement of polygon_cases.PLACEMENTS, against the exact rule,
and the header's error bound of the edge test.  No GPU."""
import math

import numpy as np
import pytest

import polygon_cases as pc
from diplomjourney_amd import abi


@pytest.fixture(scope="module")
def H():
    return pc.host()


def _tables(H, p, polygons):
    return pc.host_tables(p, polygons)


def _inside(H, table, n_poly, xy):
    return pc.host_inside(table, n_poly, xy)


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
    ab, _ = pc.sums_of(p, xy)
    back = pc.host_cum_pose(p, ab)
    # far inside the cases' 1e-9 margin to every edge line
    assert np.abs(back - xy).max() < 1e-14
    return ab, bool(pc.host_consts(p)[5])


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


# ---------------------------------------------------------------------------
# off the origin: every placement of polygon_cases.PLACEMENTS, against the exact rule
# ---------------------------------------------------------------------------
MAX_LEFT_OUT = 0.01     # share of a case's states a bound may keep out of a comparison


def _compared(got, want, judged, what):
    """got == want on the judged states; at most 1 % are not judged and a blocked
    and a free state are among the judged."""
    assert (~judged).mean() <= MAX_LEFT_OUT, (what, int((~judged).sum()))
    assert (want & judged).any() and (~want & judged).any(), what
    bad = (got != want) & judged
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:5])


@pytest.mark.parametrize("name", list(pc.PLACEMENTS))
def test_predicates_at_every_placement(oracle, name):
    """The world table on the oracle's states and the rect+cum frame table on the
    sums of those states, at every placement, against the exact rule (rational
    side of every edge line, polygon_cases.exact_inside).  A state is left out
    only within the header's bound of an edge line — plus, for the frame table,
    the printed distance between cum_pose of the sums and the state.

    Two mutants of frame_edge, built into this harness from a scratch copy of
    csrc/mpc_keepout.h: (a) without the K.x / K.y terms (c = w.c) and (b) with
    K.x and K.y swapped.  Both pass every polygon test that starts at the origin
    pose (the whole module before these placements).  Here both fail the frame
    table's comparison at all seven placements ("start", 0.2 / -0.1, included),
    and test_header_bound's frame-table assertion as well (and the rect+cum mask
    of test_ranking_cpu.py's test_polygon_case_preconditions); the world
    table's comparisons, which frame_edge does not touch, pass."""
    c = pc.placed_case(name)
    x, y = c.states[:, 0, :].ravel(), c.states[:, 1, :].ravel()
    xy = np.stack([x, y], axis=1)
    ab, err = pc.sums_of(c.problem, xy)
    want, judged = pc.exact_inside(x, y, c.polygons)
    _, judged_l = pc.exact_inside(x, y, c.polygons, extra=err)
    each = [pc.exact_inside(x, y, [g])[0] for g in c.polygons]
    print(f"{name}: {len(x)} states, {int(want.sum())} inside (per polygon "
          f"{[int(q.sum()) for q in each]}); left out: world {int((~judged).sum())}, "
          f"frame {int((~judged_l).sum())}; |cum_pose(sums) - state| <= {err:.3g}")
    assert all(q.any() for q in each[:3]) and not each[3].any() and not want.all()
    world, loop = pc.host_tables(c.problem, c.polygons)
    _compared(pc.host_inside(world, 4, xy), want, judged, f"{name} world")
    _compared(pc.host_inside(loop, 4, ab), want, judged_l, f"{name} frame")
    assert bool(pc.host_consts(c.problem)[5]) == (pc.PLACEMENTS[name][3] in (0.5, 0.25))
    assert not np.array_equal(world, loop)


# directions of the near edge's inner normal: the four axes and six others
_NORMALS = (0.0, math.pi / 2, math.pi, -math.pi / 2, 0.3, 1.1, 2.0, 2.9, -0.7, -2.3)
_HALF_SIDES = (0.07, 1.3)


def bound_sweep(name):
    """Squares with one edge line at a chosen signed distance delta from a state
    (polygon_cases.square_through), six states of the placement's case, ten
    normals, two sizes, both signs, |delta| = 2, 8, 64 times the header's bound
    at the pose and on in three equal ratios to 1e-9 — and 0, 1/16 and 1/2 of the
    bound, which assert nothing and show where the predicate does flip.  After
    the vertices are rounded the distance is the exact rule's, not delta.
    -> (rows [(exact distance, world bound, frame bound, exact inside, world
    predicate, frame predicate)], |cum_pose(sums) - state| of the placement)."""
    c = pc.placed_case(name)
    x, y = c.states[:, 0, :].ravel(), c.states[:, 1, :].ravel()
    xy = np.stack([x, y], axis=1)
    ab, err = pc.sums_of(c.problem, xy)
    px, py = pc.PLACEMENTS[name][:2]
    b0 = 8 * 2.0 ** -52 * (abs(px) + abs(py))
    mags = [0.0, b0 / 16, b0 / 2, 2 * b0, 8 * b0, 64 * b0, *np.geomspace(64 * b0, 1e-9, 4)[1:]]
    rows = []
    for k in range(0, len(xy), len(xy) // 6 + 1):
        for ang in _NORMALS:
            for h in _HALF_SIDES:
                for delta in [s * m for m in mags for s in (1.0, -1.0)]:
                    sq = pc.square_through(xy[k], ang, h, delta)
                    d = pc.exact_edge_distances(x[k], y[k], sq)
                    hb = pc.header_bound(x[k], y[k], sq)
                    near = int(np.argmin(np.abs(d)))
                    assert near == 3 and np.abs(np.delete(d, 3)).min() > 0.9 * h
                    world, loop = pc.host_tables(c.problem, [sq])
                    rows.append((d[3], hb[3], hb[3] + err, bool((d > 0).all()),
                                 bool(pc.host_inside(world, 1, xy[k:k + 1])[0]),
                                 bool(pc.host_inside(loop, 1, ab[k:k + 1])[0])))
    return rows, err


@pytest.mark.parametrize("name", list(pc.PLACEMENTS))
def test_header_bound(oracle, name):
    """include/mpc_rollout.h: a state further than 4 * 2^-52 * (|x| + |y| + |Px| +
    |Py|) from an edge line is judged as in exact arithmetic; the rect+cum test
    adds the sums' own distance from the state (sums_of's, printed)."""
    rows, err = bound_sweep(name)
    d = np.array([r[0] for r in rows])
    want = np.array([r[3] for r in rows])
    n_bound = 0
    for what, col, got_col in (("world", 1, 4), ("frame", 2, 5)):
        bound = np.array([r[col] for r in rows])
        got = np.array([r[got_col] for r in rows])
        outside = np.abs(d) > bound
        flips = got != want
        worst = float(np.abs(d[flips]).max()) if flips.any() else 0.0
        print(f"{name} {what}: {len(rows)} squares, {int(outside.sum())} beyond the bound "
              f"({bound.min():.3g}..{bound.max():.3g}), {int(flips.sum())} flips, the furthest at "
              f"|d| = {worst:.3g}; sums' distance {err:.3g}")
        assert outside.sum() >= 0.6 * len(rows) and (want & outside).any() \
            and (~want & outside).any()
        bad = flips & outside
        assert not bad.any(), (what, int(bad.sum()), float(np.abs(d[bad]).max()),
                               float(bound[bad].min()))
        n_bound += int(outside.sum())
    assert n_bound


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
