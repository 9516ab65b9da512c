"""Seeded inputs and the CPU-oracle reference of the keep-out-polygon tests
(tests/test_polygons_gpu.py, tests/test_polygon_frame_cpu.py), built on
obstacle_cases: the same pose, controls and oracles.  The blocked mask is formed
in numpy from the oracle's [N, 3, C] states with the header's real-number rule
(strictly on the inner side of every edge's line, any step, any polygon; or
inside a circle of the same call), and the expected winner is the lowest (cost,
index) among the unblocked candidates.  A case is computed once and shared
(read-only arrays).  rejected_polygons(): the polygon arguments the keep-out
entries refuse (tests/test_polygons_abi.py)."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import obstacle_cases as oc
from diplomjourney_amd.abi import (MPC_MAX_POLYGON_VERTICES, MPC_MAX_POLYGONS, MpcPolygon,
                                   make_problem)

MARGIN = oc.MARGIN


def ngon(c, R, n, rot, cw=False):
    """Regular n-gon: vertex k at c + R (cos(rot + 2 pi k / n), sin(...)); cw: the reversed list."""
    pts = [(c[0] + R * math.cos(rot + 2 * math.pi * k / n),
            c[1] + R * math.sin(rot + 2 * math.pi * k / n)) for k in range(n)]
    return pts[::-1] if cw else pts


def edge_distances(x, y, poly):
    """[n_edges, ...]: signed distance of every (x, y) from every edge's line,
    positive on the inner side (the orientation normalised by the shoelace area)."""
    P = np.asarray(poly, dtype=np.float64)
    Q = np.roll(P, -1, axis=0)
    area2 = float(np.sum(P[:, 0] * Q[:, 1] - Q[:, 0] * P[:, 1]))
    sgn = 1.0 if area2 > 0 else -1.0
    out = []
    for (px, py), (qx, qy) in zip(P, Q):
        dx, dy = qx - px, qy - py
        out.append(sgn * (dx * (y - py) - dy * (x - px)) / math.hypot(dx, dy))
    return np.stack(out)


def inside(x, y, poly):
    """Strictly inside: on the inner side of every edge's line."""
    return (edge_distances(x, y, poly) > 0).all(axis=0)


def polygon_mask(states, polygons):
    """[C]: any step, any polygon."""
    x, y = states[:, 0, :], states[:, 1, :]
    m = np.zeros(states.shape[2], dtype=bool)
    for g in polygons:
        m |= inside(x, y, g).any(axis=0)
    return m


def blocked_mask(states, polygons, circles=()):
    return polygon_mask(states, polygons) | oc.blocked_mask(states, circles)


def problem(L=0.5):
    return make_problem(oc.POSE[0], oc.POSE[1], oc.POSE[2], 2, 3, 0, 0, L, 0.05, 0.10)


@functools.lru_cache(maxsize=None)
def case(n_cand, n_steps, oracle_integ, irregular=False, mixed=False, L=0.5):
    """One seeded case.  Polygons, reach = 0.05 N: (a) a CCW octagon on the
    unconstrained oracle winner's final state, R = 0.12 reach, rot 0.3; (b) a CW
    triangle at 0.45 reach along heading 0.2, R = 0.08 reach, rot 1.0; (c) a
    square at (5, 5), R = 0.5, never reached; (d) a CW pentagon at 0.6 reach
    along heading 0.35, R = 0.05 reach, rot 0.1.  irregular: candidate `irr` has
    beta = 1.2 at step 0 (the kernels' step_safe recompute) and (c) is replaced
    by a square on its oracle state after step 2, R = 0.05 reach, rot 0.7.
    mixed: plus the circle at 0.3 reach along heading 0.3, r = 0.055 reach (at 0.05 reach the
    candidates with beta = 0 and v = 0.25 or 0.35 end step 1 on the circle itself)."""
    from oracle import oracle as O
    v, b = oc.controls(n_cand, n_steps, oc.SEED)
    irr = None
    if irregular:
        irr = n_cand // 2 + 1
        b[0, irr] = 1.2
    p = problem(L)
    res0, costs, states = O.rollout_argmin(p, v, b, integ=oracle_integ, want_costs=True,
                                           want_states=True)
    reach = 0.05 * n_steps
    w = res0.index
    # (centre, R, n, rot, cw) of each polygon: the circumscribed circle is (centre, R)
    specs = [((float(states[-1, 0, w]), float(states[-1, 1, w])), 0.12 * reach, 8, 0.3, False),
             ((0.45 * reach * math.cos(0.2), 0.45 * reach * math.sin(0.2)), 0.08 * reach, 3, 1.0,
              True),
             ((5.0, 5.0), 0.5, 4, 0.0, False),
             ((0.6 * reach * math.cos(0.35), 0.6 * reach * math.sin(0.35)), 0.05 * reach, 5, 0.1,
              True)]
    if irregular:
        specs[2] = ((float(states[1, 0, irr]), float(states[1, 1, irr])), 0.05 * reach, 4, 0.7,
                    False)
    polygons = [ngon(*s) for s in specs]
    circles = ([(0.3 * reach * math.cos(0.3), 0.3 * reach * math.sin(0.3), 0.055 * reach)]
               if mixed else [])
    mask = blocked_mask(states, polygons, circles)
    win_i, win_c = oc.expected_winner(costs, mask)
    oc._freeze(v, b, costs, states, mask)
    return SimpleNamespace(n_cand=n_cand, n_steps=n_steps, problem=p, v=v, b=b, costs=costs,
                           states=states, specs=specs, polygons=polygons, circles=circles,
                           mask=mask, n_blocked=int(mask.sum()), index=win_i, cost=win_c,
                           res0=res0, irr=irr, L=L)


def check_preconditions(c):
    """Conditions on the oracle's numbers, asserted before the GPU is looked at.
    (The mixed case is used at N = 1 and 3: at N = 10 its circle and polygons
    together block every candidate.)"""
    x, y = c.states[:, 0, :], c.states[:, 1, :]
    d = [edge_distances(x, y, g) for g in c.polygons]            # per polygon [edges, N, C]
    # the mask is the same in every arithmetic
    assert min(np.abs(q).min() for q in d) > MARGIN
    if c.circles:
        assert np.abs(oc.dist_minus_r(c.states, c.circles)).min() > MARGIN
    frac = c.n_blocked / c.n_cand
    assert 0.10 <= frac <= 0.90, frac
    assert c.mask[c.res0.index], "the unconstrained winner is not blocked"
    in_poly = [(q > 0).all(axis=0) for q in d]                   # per polygon [N, C]
    in_circ = [((x - cx) ** 2 + (y - cy) ** 2) < r * r for cx, cy, r in c.circles]
    if c.n_steps > 1:
        # blocked, with the FINAL state outside every shape: the test is per step
        final_in = np.zeros(c.n_cand, dtype=bool)
        for q in in_poly + in_circ:
            final_in |= q[-1]
        assert (c.mask & ~final_in).any()
    # inside a circumscribed circle but outside its polygon: the corners matter
    assert any(((((x - s[0][0]) ** 2 + (y - s[0][1]) ** 2) < s[1] ** 2) & ~q).any()
               for s, q in zip(c.specs, in_poly))
    # on the inner side of all edges but one: every edge matters (AND, not a vote)
    assert any(((q > 0).sum(axis=0) == q.shape[0] - 1).any() for q in d)
    for k in (0, 1, 3):
        assert in_poly[k].any(), f"polygon {k} blocks nobody"
    if c.circles:
        by_circle = np.zeros(c.n_cand, dtype=bool)
        for q in in_circ:
            by_circle |= q.any(axis=0)
        by_poly = polygon_mask(c.states, c.polygons)
        assert (by_circle & ~by_poly).any() and (by_poly & ~by_circle).any()
    assert c.index >= 0
    free = np.unique(c.costs[~c.mask & np.isfinite(c.costs)])
    if len(free) > 1:
        assert (free[1] - free[0]) > 1e-9 * free[0], (free[0], free[1])
    if c.irr is not None:
        # the replaced square alone blocks the irregular candidate, at a step that is not its last
        others = [q[:, c.irr] for k, q in enumerate(in_poly) if k != 2]
        assert not any(q.any() for q in others)
        assert in_poly[2][:-1, c.irr].any() and not in_poly[2][-1, c.irr] and c.mask[c.irr]


# ---------------------------------------------------------------------------
# arguments the entries refuse
# ---------------------------------------------------------------------------
def polygons_array(*polys, n_vertices=None):
    """MpcPolygon array of raw vertex lists (no check, no closed-form handling);
    n_vertices overrides the last polygon's count."""
    arr = (MpcPolygon * len(polys))()
    for rec, pts in zip(arr, polys):
        rec.n_vertices = len(pts)
        for i, (px, py) in enumerate(pts[:MPC_MAX_POLYGON_VERTICES]):
            rec.x[i], rec.y[i] = px, py
    if n_vertices is not None:
        arr[len(polys) - 1].n_vertices = n_vertices
    return arr


OK_POLYGON = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]


def rejected_polygons():
    """{what: (mpc_polygon_t array or None, n_polygons)}: every polygon argument a
    keep-out entry answers with MPC_ERR_ARG — a count out of range, no array, and
    each unacceptable polygon both alone and behind an acceptable one."""
    ok = OK_POLYGON
    pent = ngon((0.0, 0.0), 1.0, 5, 0.2)
    bad = {"negative count": (polygons_array(ok), -1),
           "too many": (polygons_array(*[ok] * (MPC_MAX_POLYGONS + 1)), MPC_MAX_POLYGONS + 1),
           "no array": (None, 1)}
    shapes = {
        "two vertices": (ok, 2),
        "nine vertices": (ngon((0.0, 0.0), 1.0, 8, 0.0), 9),
        "nan vertex": ([(0.0, 0.0), (1.0, math.nan), (1.0, 1.0), (0.0, 1.0)], None),
        "inf vertex": ([(0.0, 0.0), (math.inf, 0.0), (1.0, 1.0), (0.0, 1.0)], None),
        "-inf vertex": ([(0.0, 0.0), (1.0, 0.0), (1.0, -math.inf), (0.0, 1.0)], None),
        "repeated vertex": ([(0.0, 0.0), (1.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], None),
        "collinear triple": ([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (2.0, 2.0), (0.0, 2.0)], None),
        "dart": ([(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)], None),
        "bow-tie": ([(0.0, 0.0), (2.0, 2.0), (2.0, 0.0), (0.0, 1.0)], None),
        "pentagram": ([pent[k] for k in (0, 2, 4, 1, 3)], None),
        "zero area": ([(0.0, 0.0), (1.0, 1.0), (2.0, 2.0)], None),
    }
    for what, (pts, n) in shapes.items():
        bad[what] = (polygons_array(pts, n_vertices=n), 1)
        bad[what + " after a valid polygon"] = (polygons_array(ok, pts, n_vertices=n), 2)
    return bad
