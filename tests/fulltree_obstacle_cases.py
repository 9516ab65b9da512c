"""Keep-out circles in the full tree against the host replica
(tests/test_fulltree_obstacles_cpu.py, test_fulltree_obstacles_gpu.py).

The model builds on fulltree_cases: the replica's three layer states of every
leaf, the blocked mask formed in numpy (a leaf is blocked if any of its layer
states lies strictly inside any circle; a NaN state is inside nothing), blocked
costs set to +inf, then unit_minima() / expected_records() for every shard's
record, and a per-unit blocked count reduced over the shard ranges (clamped
lanes hold no leaf, so they count nothing).

Every scene keeps every finite layer state at least MARGIN away from every
circle's boundary — model() asserts it — so whether the device's predicate
rounds fma(dy, dy, dx * dx) as numpy rounds its own cannot matter.  A radius is
therefore chosen as the midpoint of a gap in the sorted distances of the states
to the centre (gap_radius).

scene(name, c) -> the circles of a scene for a case; peel_next() the ranking
scene's next circle; run_sweep() / check_sweep() the drivers (public ABI only).
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np

import fulltree_cases as F
from diplomjourney_amd.abi import FT_RESULT_BYTES, INTEGRATORS, make_obstacles

MARGIN = 1e-9
SCENES = ("subtree", "pair", "graze", "all", "start_inside", "far16", "nan")
SMALL = (5, 9, 14)            # the full sweep(s1)
LARGE = (65, 72)              # n_shards of LARGE_SHARDS
LARGE_SHARDS = (1, 2, 3, 5, 13, 89)
PEEL_ROUNDS = 16

_states = {}


def n_list(s1):
    return F.sweep(s1) if s1 in SMALL else list(LARGE_SHARDS)


def nan_index(s1):
    """The speed that scene `nan` replaces: V[1], or V[0] of a one-speed grid."""
    return min(1, F.SHAPES[s1][0] - 1)


def states_of(c):
    """The replica's layer states [S1^3, 3, 3] of every leaf of a case (read-only)."""
    key = (c.s1, c.name, c.mode, c.problem.L, bool(np.isnan(c.V).any()), c.device,
           c.device_consts)
    if key not in _states:
        st = F.layer_states(c, np.arange(c.s1 ** 3))
        st.flags.writeable = False
        _states[key] = st
    return _states[key]


def distances(st, centre):
    """Every layer state's distance to `centre` [S1^3, 3] (NaN for a NaN state)."""
    return np.hypot(st[:, :, 0] - centre[0], st[:, :, 1] - centre[1])


def gap_radius(st, centre, want):
    """The midpoint nearest to `want` of a gap of at least 4 * MARGIN in the
    sorted distances of the finite states to `centre` (below the smallest
    distance, 0 counts as one; above the largest, want itself if it is clear)."""
    d = distances(st, centre)
    d = np.unique(d[np.isfinite(d)])
    edges = np.concatenate([[0.0], d])
    lo, hi = edges[:-1], edges[1:]
    ok = (hi - lo) >= 4 * MARGIN
    mids = (lo[ok] + hi[ok]) / 2
    mids = mids[mids > MARGIN]
    cand = list(mids)
    if len(d) == 0 or want - d[-1] >= MARGIN:
        cand.append(want)
    assert cand, "no gap in the distances"
    cand = np.asarray(cand)
    return float(cand[np.argmin(np.abs(cand - want))])


def blocked_mask(st, circles):
    """[S1^3] bool: some layer state strictly inside some circle; asserts the
    scene condition |dist - r| >= MARGIN for every finite state."""
    blocked = np.zeros(len(st), dtype=bool)
    for (cx, cy, r) in circles:
        d = distances(st, (cx, cy))
        fin = np.isfinite(d)
        assert (np.abs(d[fin] - r) >= MARGIN).all(), \
            f"circle ({cx}, {cy}, {r}): a state within {MARGIN} of its boundary"
        with np.errstate(invalid="ignore"):
            blocked |= (d < r).any(axis=1)
    return blocked


def model(c, circles):
    """The expected numbers of a case with circles: blocked [S1^3], costs with
    the blocked leaves at +inf, their unit minima, the blocked leaves per unit."""
    s1 = c.s1
    st = states_of(c)
    blocked = blocked_mask(st, circles)
    costs = np.where(blocked, np.inf, c.costs)
    unit_blocked = np.bincount(F.unit_of(np.arange(s1 ** 3), s1), weights=blocked,
                               minlength=F.n_units(s1)).astype(np.int64)
    return SimpleNamespace(case=c, circles=list(circles), states=st, blocked=blocked, costs=costs,
                           minima=F.unit_minima(costs, s1), unit_blocked=unit_blocked)


def shard_counts(unit_blocked, n_shards):
    """The blocked leaves of every shard of an n_shards split."""
    nu = len(unit_blocked)
    base, rem = divmod(nu, n_shards)
    s = np.arange(n_shards)
    return np.add.reduceat(unit_blocked, s * base + np.minimum(s, rem))


def scan_model(c, circles, shard, n_shards):
    """The plain form of model(): a triple loop over (k0, k1, k2) in leaf order,
    the script's strict-< scan over the leaves whose unit the shard owns ->
    (leaf or -1, cost, blocked leaves of the shard)."""
    s1 = c.s1
    st = states_of(c)
    lo, hi = F.shard_range(shard, n_shards, s1)
    best, best_leaf, count = math.inf, -1, 0
    for k0 in range(s1):
        for k1 in range(s1):
            for k2 in range(s1):
                leaf = (k0 * s1 + k1) * s1 + k2
                u = ((k0 * s1 + k1) // 64) * s1 + k2
                if not lo <= u < hi:
                    continue
                inside = any((st[leaf, l, 0] - cx) ** 2 + (st[leaf, l, 1] - cy) ** 2 < r * r
                             for l in range(3) for (cx, cy, r) in circles)
                if inside:
                    count += 1
                elif c.costs[leaf] < best:
                    best, best_leaf = float(c.costs[leaf]), leaf
    return best_leaf, best, count


# ----------------------------------------------------------------------------
# the scenes
# ----------------------------------------------------------------------------
def vh_max(c):
    """The largest last-layer step |v * h| of a case (NaN speeds aside)."""
    return float(np.nanmax(np.abs(c.V), initial=0.0)) * (F.T_B - F.T_A)


def reach_kinds(c, circles):
    """Per circle: (some layer-1 state lies within r + one step's reach (1 %
    slack), leaves blocked at layer 2 alone by it)."""
    st = states_of(c)
    out = []
    for (cx, cy, r) in circles:
        d = distances(st, (cx, cy))
        near = bool((d[:, 1] < r + 1.01 * vh_max(c)).any())
        with np.errstate(invalid="ignore"):
            only2 = int(((d[:, 2] < r) & ~(d[:, :2] < r).any(axis=1)).sum())
        out.append((near, only2))
    return out


def scene(name, c):
    """The circles [(x, y, r)] of scene `name` for case c (states_of(c))."""
    s1 = c.s1
    st = states_of(c)
    start = (c.problem.x, c.problem.y)
    fast = s1 - 1                      # a control with the largest speed
    if name == "subtree":              # the layer-0 state of k0 = fast: its S1^2 leaves
        centre = st[fast * s1 * s1, 0, :2]
        return [(centre[0], centre[1], gap_radius(st, centre, 1e-3))]
    if name in ("pair", "nan"):        # the layer-1 state of the pair (fast, S1 // 2)
        centre = st[(fast * s1 + s1 // 2) * s1, 1, :2]
        return [(centre[0], centre[1], gap_radius(st, centre, 1e-4))]
    if name == "graze":                # the leaf state of (fast, fast, fast), and a far circle
        centre = st[s1 ** 3 - 1, 2, :2]
        return [(centre[0], centre[1], gap_radius(st, centre, 1e-4)),
                (start[0] + 100.0, start[1] - 100.0, 1.0)]
    if name == "all":
        return [(start[0], start[1], float(np.nanmax(distances(st, start))) + 1.0)]
    if name == "start_inside":         # between the rings of the slower and the faster speeds
        return [(start[0], start[1], gap_radius(st, start, 0.6 * vh_max(c) + 1e-3))]
    if name == "far16":
        return [(start[0] + 50.0 + 3.0 * i, start[1] + 40.0, 1.0) for i in range(16)]
    raise KeyError(name)


def scene_case(name, s1, mode, device=False, L=F.WHEELBASE):
    """(case, circles) of a scene: problem `move`; scene `nan` on the NaN grid."""
    if name == "nan":
        # the circle of the grid without the NaN (its finite states are a subset
        # of that grid's, so the radius' gap holds; its own pair state may be NaN)
        return (F.case(s1, "move", mode, L, nan_index(s1), device),
                scene("pair", F.case(s1, "move", mode, L, None, device)))
    c = F.case(s1, "move", mode, L, None, device)
    return c, scene(name, c)


def peel_next(m):
    """The ranking scene's next circle: a tiny one on the current winner's leaf
    state (None when the model has no winner left)."""
    leaf, _, _ = F.expected_records(m.minima, 1)
    if leaf[0] < 0:
        return None
    centre = m.states[int(leaf[0]), 2, :2]
    return (float(centre[0]), float(centre[1]), gap_radius(m.states, centre, 1e-6))


# ----------------------------------------------------------------------------
# the drivers (GPU)
# ----------------------------------------------------------------------------
def run_sweep(engine, c, circles, shards, incumbent=math.inf, count=True):
    """All shards of all n_shards of `shards` through
    mpc_fulltree_argmin_obstacles, every launch writing its record and its
    count into a row of device logs read once.  Returns (log int64 [launches,
    REC_WORDS], counts int64 [launches], [(n_shards, shard)] per row)."""
    import torch
    from diplomjourney_amd import native
    C, lib = native.calls(), engine.lib
    nv, nb = len(c.V), len(c.B)
    vg = torch.tensor(c.V, dtype=torch.float64, device=engine.device)
    bg = torch.tensor(c.B, dtype=torch.float64, device=engine.device)
    ws = engine._workspace(lib.mpc_fulltree_workspace_bytes(nv, nb))
    rows = [(n, s) for n in shards for s in range(n)]
    log = torch.zeros((len(rows), F.REC_WORDS), dtype=torch.int64, device=engine.device)
    counts = torch.full((len(rows),), -1, dtype=torch.int64, device=engine.device)
    obs, n_obs = make_obstacles(circles)
    integ = INTEGRATORS[c.mode]
    p, stream = ctypes.byref(c.problem), native.current_stream()
    vp, bp, wp, wn = vg.data_ptr(), bg.data_ptr(), ws.data_ptr(), ws.numel()
    for i, (n, s) in enumerate(rows):
        C.mpc_fulltree_argmin_obstacles(p, obs, n_obs, vp, nv, bp, nb, float(incumbent), integ, s,
                                        n, wp, wn, counts.data_ptr() + 8 * i if count else None,
                                        log.data_ptr() + i * FT_RESULT_BYTES, stream)
    return log.cpu().numpy(), counts.cpu().numpy(), rows


def check_sweep(log, counts, rows, m, shards, what=""):
    """A run_sweep() result against the model: every shard's record (leaf, cost
    bits, found, controls, layer states) and every shard's count."""
    c = m.case
    s1 = c.s1
    parts = [F.expected_records(m.minima, n) for n in shards]
    leaf = np.concatenate([p[0] for p in parts])
    cost = np.concatenate([p[1] for p in parts])
    assert len(leaf) == len(rows) == len(log)
    found = (leaf >= 0).astype(np.int64)
    states = m.states[np.where(leaf >= 0, leaf, 0)]

    def label(i):
        n, s = rows[i]
        lo, hi = F.shard_range(s, n, s1)
        return f"n_shards {n}, shard {s} (units [{lo}, {hi}))"
    F.check_records(log, s1, c.V, c.B, leaf, cost, found, states, label, what)
    want = np.concatenate([shard_counts(m.unit_blocked, n) for n in shards])
    bad = counts != want
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {label(i)}: {int(want[i])} blocked leaves expected, the "
                             f"kernel counted {int(counts[i])} ({int(bad.sum())} of {len(rows)} "
                             f"counts differ)")
    return len(rows)
