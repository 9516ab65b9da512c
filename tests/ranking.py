"""Candidate ranking by peeling (tests/test_ranking_gpu.py, test_ranking_cpu.py).

An arg-min launch reports one candidate.  Launching again after the winner's
step-0 speed has been overwritten with NaN (a NaN cost never wins,
include/mpc_rollout.h) reports the next one, and so on until the result is
index -1, found 0: the sequence of winners is the kernel's complete ordering of
its candidates by (cost, index).  It must equal the host replica's costs sorted
by (cost, index) element for element, `==` on the doubles: one wrong cost,
index, tie or mask bit anywhere in the launch changes the sequence, and the
first mismatch names the candidate, hence its tile, wave, lane and pair slot.

peel() is the driver (public ABI and production binaries only, no host
synchronisation per peel), check_ranking() the comparison, controls() the fixed
seeded input of a horizon, check_preconditions() what is asserted of the
replica's numbers before a kernel is looked at.  polygon_case() is one case of
the keep-out polygon kernels (tests/test_ranking_polygons_gpu.py): scene,
expected mask and its conditions.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from diplomjourney_amd.abi import MPC_TILE, RESULT_BYTES, make_problem

N_CAND = 1026          # two full 512-candidate tiles plus one lane pair
HORIZONS = (1, 2, 3, 4, 7, 32)
# start pose (x, y, phi, v, beta) and target of every ranked problem: the target
# lies 4 m ahead, slightly left of the heading, so that progress ranks a candidate
START = (0.2, -0.1, 0.7, 0.5, 0.0)
TARGET = (2.7, 3.0)
SEED = 100             # + n_steps; a seed that misses a precondition is replaced
RESULT_WORDS = RESULT_BYTES // 8
# words of one mpc_result_t that a peel records: cost, index, found | n_steps << 32,
# v, beta, traj[0] = (x, y, phi)
REC_WORDS = 8


def where(c):
    """Where candidate c runs in the streaming kernels (512-candidate tiles of
    four waves, two candidates per lane)."""
    c = int(c)
    if c < 0:
        return "no candidate"
    return (f"candidate {c}: tile {c // MPC_TILE}, wave {(c % MPC_TILE) // 128}, "
            f"lane {(c % 128) // 2}, pair slot {c % 2}")


# ----------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------
def result_words(buf, n=1):
    """[n, REC_WORDS] int64 view of the leading words of n mpc_result_t."""
    return buf.view(torch.int64).view(n, RESULT_WORDS)[:, :REC_WORDS]


def soa_offset(ld=0):
    """Flat offset of candidate c's step-0 v in an SoA tensor [N, C]: c itself;
    robot r of a batched [N, R * ld] tensor: r * ld + c."""
    def off(c):
        if ld:
            return c + ld * torch.arange(c.numel(), device=c.device)
        return c
    return off


def tiled_offset(n_steps):
    """The same in a tiled tensor (mpc_tiled_index at s = 0)."""
    def off(c):
        return (c // MPC_TILE) * (2 * MPC_TILE * n_steps) + c % MPC_TILE
    return off


def peel(launch, v, offset, n_peels):
    """launch() enqueues the kernel under test and returns an int64 tensor
    [R, W] (R problems; word 0 the winner's cost bits, word 1 its index, the
    rest whatever the case wants logged) on v's device.  After every launch the
    winner's step-0 v in `v` (any layout: offset(index tensor) -> flat offsets)
    is overwritten with NaN, an index of -1 leaving the tensor as it is.
    Nothing synchronises: the records go to a device log that is copied once.
    Returns the log, numpy int64 [n_peels, R, W]."""
    flat = v.view(-1)
    nan = torch.full((), math.nan, dtype=torch.float64, device=flat.device)
    log = None
    for i in range(n_peels):
        rec = launch()
        if log is None:
            log = torch.zeros((n_peels,) + tuple(rec.shape), dtype=torch.int64,
                              device=rec.device)
        log[i].copy_(rec)
        idx = rec[:, 1]
        ok = idx >= 0
        at = offset(torch.where(ok, idx, torch.zeros_like(idx)))
        ok = ok & (at < flat.numel())        # a wild index is logged, never written through
        at = torch.where(ok, at, torch.zeros_like(at))
        flat[at] = torch.where(ok, nan, flat[at])
    return log.cpu().numpy()


def _f64(words):
    return np.ascontiguousarray(words).view(np.float64)


def expected_order(costs, excluded=None):
    """Indices of the candidates with a finite cost (and not excluded), sorted
    by (cost, index)."""
    costs = np.asarray(costs)
    order = np.lexsort((np.arange(len(costs)), costs))
    keep = np.isfinite(costs)
    if excluded is not None:
        keep &= ~excluded
    return order[keep[order]]


def check_ranking(got, costs, excluded=None, states=None, top=None, what=""):
    """got: one problem's peel log [n_peels, W >= 3] (W >= 8 with states: words
    5..7 the winner's first state).  The peeled sequence must be
    expected_order() with bitwise-equal costs, every entry found, then index
    -1 / found 0 to the end of the log, which must hold at least one such
    record.  top: compare the first `top` only (no end-of-sequence check).
    Returns the number of ranked candidates."""
    order = expected_order(costs, excluded)
    n = len(order) if top is None else top
    assert top is None or len(order) >= top
    assert len(got) >= n + (top is None), f"{what}: {len(got)} peels for {n} candidates"
    g_idx, g_cost = got[:, 1], _f64(got[:, 0])
    g_found = got[:, 2] & 0xFFFFFFFF
    want_idx, want_cost = order[:n], np.asarray(costs)[order[:n]]
    bad = (g_idx[:n] != want_idx) | ~(g_cost[:n] == want_cost) | (g_found[:n] != 1)
    if bad.any():
        k = int(np.argmax(bad))
        c = int(want_idx[k])
        raise AssertionError(
            f"{what}: rank {k} of {n}: expected {where(c)} cost {want_cost[k]!r}; the kernel "
            f"reported {where(g_idx[k])} cost {g_cost[k]!r} found {g_found[k]} "
            f"({int(bad.sum())} of {n} ranks differ)")
    if states is not None:
        first = np.stack([_f64(got[:n, 5 + k]) for k in range(3)], axis=1)   # [n, 3]
        want = states[0][:, want_idx].T
        diff = ~(first == want).all(axis=1)
        if diff.any():
            k = int(np.argmax(diff))
            raise AssertionError(f"{what}: rank {k}: the reported first state of "
                                 f"{where(want_idx[k])} is {first[k]!r}, the replica's {want[k]!r}")
    if top is None:
        tail = (g_idx[n:] != -1) | (g_found[n:] != 0)
        if tail.any():
            k = n + int(np.argmax(tail))
            raise AssertionError(f"{what}: after the {n} finite candidates the kernel reported "
                                 f"{where(g_idx[k])} cost {g_cost[k]!r} found {g_found[k]}")
    return n


# ----------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------
def problem(L, pose=START[:3], t_a=0.05, t_b=0.05 + 0.05):
    """The ranked problem: an episode's first step from START (t = delta_t)."""
    return make_problem(pose[0], pose[1], pose[2], TARGET[0], TARGET[1], START[0], START[1], L,
                        t_a, t_b)


def grid_batch(n, n_steps, seed):
    """Reference-grid controls drawn as tests/test_replica.py's _case draws them."""
    from oracle import oracle as O
    from diplomjourney_amd import math_model_tree as mmt
    V = mmt.vector_of_velocities(0.5)
    B = mmt.vector_of_beta_angles(0.0)
    return O.sample_controls(V, B, n, n_steps, seed)


@functools.lru_cache(maxsize=None)
def controls(n_steps, n=N_CAND):
    """The fixed input of a horizon (read-only arrays): grid controls, then
    * every column whose whole control sequence repeats an earlier column's gets
      an off-grid step-0 speed of its own (the grid has 451 entries: at N = 1
      most of 1026 draws repeat one), so that costs tie only where meant to;
    * irregular candidates (|beta| > 1.1, |dphi| > 0.2): four with |beta| in
      (1.1, 1.25) at some step, two with a speed that makes |dphi| > 0.2, two
      with a steering angle around 1e8.  One sits in tile 2 (the last tile's
      only pair, or only candidate for n = 1025), one is the second candidate
      of a pair whose first is regular, several sit in tile 1.  Candidate 1024
      (|beta| = 1.15 at step 0) also drives faster than any grid candidate, so
      it ranks near the top in every mode;
    * two candidates with a NaN steering angle and one with v = +inf;
    * three pairs of exact duplicates (dst := src): within one lane pair,
      across two waves of a tile, across two tiles."""
    N, last = n_steps, n_steps - 1
    v, b = grid_batch(n, N, SEED + N)
    seen = set()
    for c in range(n):
        key = v[:, c].tobytes() + b[:, c].tobytes()
        if key in seen:
            v[0, c] = 0.476 + 0.048 * (c + 0.37) / n
            key = v[:, c].tobytes() + b[:, c].tobytes()
        seen.add(key)
    odd = 1025 if n > 1025 else 1023          # second of a pair whose first is regular
    # (candidate, step, v or None, beta or None)
    edits = [(1024, 0, 1.2, 1.15), (201, 0, None, -1.15), (813, N // 2, None, 1.22),
             (390, last, None, -1.24),
             (odd, min(1, last), 40.0, 0.06), (589, 0, 36.0, -0.07),
             (47, 0, None, 1e8), (950, last, None, -1.3e8),
             (5, 0, None, math.nan), (700, last, None, math.nan),
             (513, last, math.inf, None)]
    if N >= 2:
        edits.append((1024, 1, 30.0, 0.05))
    for c, s, vv, bb in edits:
        if vv is not None:
            v[s, c] = vv
        if bb is not None:
            b[s, c] = bb
    dup = ((10, 11), (30, 300), (100, 712))
    for src, dst in dup:
        v[:, dst], b[:, dst] = v[:, src], b[:, src]
    v.flags.writeable = b.flags.writeable = False
    return SimpleNamespace(n=n, n_steps=N, v=v, b=b, dup=dup,
                           beta_irregular=(1024, 201, 813, 390, 47, 950),
                           dphi_irregular=(odd, 589), nonfinite=(5, 700, 513))


def check_preconditions(inp, costs):
    """What must hold of the replica's costs of an input before a kernel is
    looked at.  Returns the number of finite costs."""
    costs = np.asarray(costs)
    fin = np.isfinite(costs)
    assert not fin[list(inp.nonfinite)].any()
    dst = [d for _, d in inp.dup]
    for s, d in inp.dup:
        assert fin[s] and costs[s] == costs[d], (s, d, costs[s], costs[d])
    rest = fin.copy()
    rest[dst] = False
    assert len(np.unique(costs[rest])) == int(rest.sum()), "an unintended tie"
    first = set(expected_order(costs)[:20].tolist())
    assert first & set(inp.beta_irregular), "no |beta| > 1.1 candidate among the first 20"
    assert int(fin.sum()) >= inp.n - 3 - 8
    return int(fin.sum())


# ----------------------------------------------------------------------------
# keep-out circles
# ----------------------------------------------------------------------------
def circles(states, winner, n_steps):
    """The three circles of obstacle_cases.case around this input: (a) on the
    unconstrained winner's final state, r = 0.10 reach; (b) at 0.45 reach ahead
    of the start pose, 0.1 rad right of its heading, r = 0.05 reach; (c) (5, 5,
    0.5), never reached; reach = 0.05 N."""
    reach = 0.05 * n_steps
    h = START[2] - 0.1
    return [(float(states[-1, 0, winner]), float(states[-1, 1, winner]), 0.10 * reach),
            (START[0] + 0.45 * reach * math.cos(h), START[1] + 0.45 * reach * math.sin(h),
             0.05 * reach),
            (5.0, 5.0, 0.5)]


def blocked(states, circ):
    """(mask, min |distance - r|) from the replica's states with the header's
    formula: any step, any circle, (x_k - x)^2 + (y_k - y)^2 < r^2; a NaN state
    is inside no circle."""
    x, y = states[:, 0, :], states[:, 1, :]
    m = np.zeros(states.shape[2], dtype=bool)
    margin = math.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for cx, cy, r in circ:
            d2 = (x - cx) ** 2 + (y - cy) ** 2
            m |= (d2 < r * r).any(axis=0)
            margin = min(margin, float(np.nanmin(np.abs(np.sqrt(d2) - r))))
    return m, margin


# ----------------------------------------------------------------------------
# keep-out polygons (tests/test_ranking_polygons_gpu.py, test_ranking_cpu.py)
# ----------------------------------------------------------------------------
IRR_BLOCKED = 201      # the beta_irregular candidate the pentagon sits on (beta = -1.15 at step 0)


def placed_circles(name, states, winner, n_steps):
    """circles() seen from a placement of polygon_cases.PLACEMENTS ("start":
    circles() itself): (c) 7 m ahead, 0.8 rad left, where the never-reached
    square is."""
    import polygon_cases as pc
    if name == "start":
        return circles(states, winner, n_steps)
    reach = 0.05 * n_steps
    return [(float(states[-1, 0, winner]), float(states[-1, 1, winner]), 0.10 * reach),
            (*pc.ahead(name, 0.45 * reach, -0.1), 0.05 * reach),
            (*pc.ahead(name, 7.0, 0.8), 0.5)]


def polygon_scene(name, states, costs, inp, n_steps, n_poly=4, through=None):
    """The polygons ranked at a placement, placed from the replica's states at
    that pose and sized by the cloud of the regular candidates (speeds within
    5 % of 0.5 m/s: after N steps a patch 0.0025 N m long and a few mm wide,
    0.025 N m ahead), reach = 0.05 N:
    (a) a CCW octagon on the unconstrained winner's final state, R = 0.12 reach
        (the winner is the fast candidate 1025, metres ahead of the cloud);
    (b) a CW triangle in the final cloud, 0.3 of the way along its bounding box
        from the low corner, R = 0.25 of the box's diagonal;
    (c) a CW pentagon on candidate IRR_BLOCKED's state after step 2 (step 1 for
        N = 1) that reaches 0.9 of the way to the middle of the regular
        candidates' states of that step;
    (d) a CCW square 7 m ahead, R = 0.5, never reached — or, through = (candidate,
        step): a square of half-side 0.3 reach with an edge line through that
        state itself, its inner normal 0.4 rad left of the heading, so that the
        rounded vertices leave the state within an ulp or two of the line, on
        whichever side.
    Rotations are relative to the heading.  -> (specs, polygons), the first
    n_poly; a spec is (centre, R, n, rot, cw) or None for the square through a
    state."""
    import polygon_cases as pc
    phi = pc.PLACEMENTS[name][2]
    reach = 0.05 * n_steps
    w = int(expected_order(costs)[0])
    regular = np.isfinite(costs)
    regular[list(inp.beta_irregular) + list(inp.dphi_irregular)] = False
    fx, fy = states[-1, 0, regular], states[-1, 1, regular]
    lo, hi = np.array([fx.min(), fy.min()]), np.array([fx.max(), fy.max()])
    k = min(1, n_steps - 1)
    on = states[k, :2, IRR_BLOCKED]
    mid = np.array([np.median(states[k, 0, regular]), np.median(states[k, 1, regular])])
    specs = [((float(states[-1, 0, w]), float(states[-1, 1, w])), 0.12 * reach, 8, phi + 0.3,
              False),
             (tuple(float(q) for q in lo + 0.3 * (hi - lo)), 0.25 * float(np.hypot(*(hi - lo))), 3,
              phi + 1.0, True),
             ((float(on[0]), float(on[1])), 0.9 * float(np.hypot(*(mid - on))), 5, phi + 0.1, True),
             (pc.ahead(name, 7.0, 0.8), 0.5, 4, phi, False)]
    polys = [pc.ngon(*q) for q in specs]
    if through is not None:
        c, kk = through
        polys[3] = pc.square_through(states[kk, :2, c], phi + 0.4, 0.3 * reach)
        specs[3] = None
    return specs[:n_poly], polys[:n_poly]


def host_polygon_mask(p, polygons, mode, states, sums=None, bad=None):
    """[N, C]: the lane hook's verdict on every state, by the host build of its
    own functions (csrc/mpc_keepout.h through tests/polygon_harness.cpp): the
    world table on the replica's states — and for rect+cum the frame table on
    the recurrence's sums (harness.replica_cum_sums), except a `bad` candidate,
    whose recomputed states meet the world table.  No margin anywhere: two fma
    and a compare are the same on both sides."""
    import polygon_cases as pc
    N, _, C = states.shape
    world, loop = pc.host_tables(p, polygons)
    flat = np.stack([states[:, 0, :].ravel(), states[:, 1, :].ravel()], axis=1)
    in_world = pc.host_inside(world, len(polygons), flat).reshape(N, C)
    if mode != "rect+cum":
        return in_world     # (the launch's loop table is the world table)
    flat = np.stack([sums[:, 0, :].ravel(), sums[:, 1, :].ravel()], axis=1)
    in_loop = pc.host_inside(loop, len(polygons), flat).reshape(N, C)
    return np.where(bad[None, :], in_world, in_loop)


def sums_distance(p, states, sums, bad):
    """rect+cum: cum_pose of the sums must be the replica's state bit for bit
    (the export is the replica's own recurrence); -> the largest distance of a
    state from the real-number image x0 + c0 A - s0 B, y0 + s0 A + c0 B of its
    sums, which is what the frame table judges — the "sums' own distance from
    the state" of the header's rect+cum bound — formed in long double."""
    import polygon_cases as pc
    N, _, C = states.shape
    ok = ~bad & np.isfinite(states[:, 0, :]).all(axis=0)
    ab = np.stack([sums[:, 0, :][:, ok].ravel(), sums[:, 1, :][:, ok].ravel()], axis=1)
    xy = np.stack([states[:, 0, :][:, ok].ravel(), states[:, 1, :][:, ok].ravel()], axis=1)
    back = pc.host_cum_pose(p, ab)
    assert back.tobytes() == np.ascontiguousarray(xy).tobytes(), "the sums are not the replica's"
    kx, ky, s0, c0, _, pow2, L = (np.longdouble(q) for q in pc.host_consts(p))
    A, B = np.longdouble(ab[:, 0]), np.longdouble(ab[:, 1])
    if pow2:
        A, B = A * L, B * L
    ex, ey = kx + (c0 * A - s0 * B) - np.longdouble(xy[:, 0]), \
        ky + (s0 * A + c0 * B) - np.longdouble(xy[:, 1])
    return float(np.hypot(ex, ey).max())


def polygon_case(name, mode, n_steps, n=N_CAND, n_poly=4, mixed=False, plant=False, device=False):
    """One ranked keep-out case: the fixed input of the horizon from a
    placement's pose, the replica's states, costs and (rect+cum) sums — with the
    device's reciprocal estimates when device, so bit for bit the kernel's — the
    scene's polygons placed from them, and the expected mask, checked by
    check_polygon_scene.  plant: the far square gives way to one with an edge
    line through the final state of the best regular candidate the other three
    polygons leave free.  mixed: plus placed_circles."""
    import polygon_cases as pc
    from harness import replica_cum_sums, replica_rollout
    inp = controls(n_steps, n)
    p = pc.placed_problem(name)
    st, costs = replica_rollout(p, inp.v, inp.b, mode, device_estimates=device)
    n_fin = check_preconditions(inp, costs)
    assert n_fin == n - 3
    sums = bad = None
    extra = 0.0
    if mode == "rect+cum":
        sums, bad = replica_cum_sums(p, inp.v, inp.b, device_estimates=device)
        assert bad[list(inp.beta_irregular)].all() and bad.sum() < 20
        extra = sums_distance(p, st, sums, bad)
    through = None
    if plant:
        _, three = polygon_scene(name, st, costs, inp, n_steps, 3)
        taken = host_polygon_mask(p, three, mode, st, sums, bad).any(axis=0)
        taken[list(inp.beta_irregular) + list(inp.dphi_irregular)] = True   # a regular one: loop()
        through = (int(expected_order(costs, excluded=taken)[0]), n_steps - 1)
    specs, polygons = polygon_scene(name, st, costs, inp, n_steps, n_poly, through)
    per_state = host_polygon_mask(p, polygons, mode, st, sums, bad)
    circ = placed_circles(name, st, int(expected_order(costs)[0]), n_steps) if mixed else []
    what = f"{name} {mode} N={n_steps}"
    mask = check_polygon_scene(inp, st, costs, polygons, specs, per_state, extra, circ, through,
                               strict=n_poly == 4, what=what)
    return SimpleNamespace(name=name, mode=mode, inp=inp, problem=p, states=st, costs=costs,
                           polygons=polygons, circles=circ, mask=mask, extra=extra,
                           through=through, n_fin=n_fin,
                           n_free=int((np.isfinite(costs) & ~mask).sum()), what=what)


def check_polygon_scene(inp, states, costs, polygons, specs, per_state, extra=0.0, circ=(),
                        through=None, strict=True, what=""):
    """What a polygon case asserts of the reference before any launch.
    per_state [N, C]: host_polygon_mask.  It must be the exact rule
    (polygon_cases.exact_inside) on every state further from every edge line
    than the header's bound plus `extra`; at most 1 % of the states are not so
    judged (the `through` state is one of them and with N = 1 the only one) and a
    blocked and a free candidate are.  Then the conditions on the mask: 10 to
    90 % of the finite candidates blocked, the unconstrained winner among them,
    one blocked at a step that is not its last while its last state is free (N >
    1), a state inside a circumscribed circle and outside its polygon, every
    polygon of the scene but the far square blocking somebody, IRR_BLOCKED
    blocked and another beta_irregular candidate free.  circ: circles of the
    same call — some candidate blocked by a circle alone, some by a polygon
    alone, some by both.  -> the call's mask [C]."""
    import polygon_cases as pc
    N, _, C = states.shape
    x, y = states[:, 0, :], states[:, 1, :]
    want, judged = pc.exact_inside(x, y, polygons, extra=extra)
    left_out = int((~judged).sum())
    if through is not None:
        assert not judged[through[1], through[0]], "the planted state is not within the bound"
    assert left_out <= max(0.01 * judged.size, 1 if through is not None else 0), (what, left_out)
    bad = (per_state != want) & judged
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5])
    fully = judged.all(axis=0)
    by_poly = per_state.any(axis=0)
    assert (by_poly & fully).any() and (~by_poly & fully).any()
    fin = np.isfinite(costs)
    mask = by_poly.copy()
    if len(circ):
        by_circle, margin = blocked(states, circ)
        assert margin > MARGIN, margin
        assert (by_circle & ~by_poly).any() and (by_poly & ~by_circle).any() \
            and (by_poly & by_circle).any(), what
        mask |= by_circle
    frac = (mask & fin).sum() / fin.sum()
    print(f"{what}: {int((mask & fin).sum())} of {int(fin.sum())} finite candidates blocked, "
          f"{left_out} of {judged.size} states within {extra:.3g} + the header's bound of an edge")
    assert mask[int(expected_order(costs)[0])], "the unconstrained winner is not blocked"
    each = [pc.exact_inside(x, y, [g])[0] for g in polygons]
    if not strict:         # fewer polygons: every one of them blocks somebody, somebody is free
        assert all(q.any() for q in each) and 0 < frac < 1, what
        return mask
    assert 0.10 <= frac <= 0.90, (what, frac)
    if N > 1:
        final_in = np.zeros(C, dtype=bool)
        for q in each:
            final_in |= q[-1]
        assert (by_poly & ~final_in & fully).any(), what
    for s, q in zip(specs, each):
        if s is None:
            continue
        if s[1] != 0.5:
            assert q.any(), (what, "a polygon blocks nobody")
        else:
            assert not q.any()
    with np.errstate(invalid="ignore"):
        assert any(((((x - s[0][0]) ** 2 + (y - s[0][1]) ** 2) < s[1] ** 2) & ~q).any()
                   for s, q in zip(specs, each) if s is not None), what
    irr = list(inp.beta_irregular)
    if len(polygons) >= 3:
        assert by_poly[IRR_BLOCKED], what
    assert not by_poly[irr].all() and (by_poly[irr].any() or len(polygons) < 3), what
    return mask


# ----------------------------------------------------------------------------
# the workload's grid shape: a top-K case
# ----------------------------------------------------------------------------
BIG_N = 2 * 2048 * 512 + N_CAND     # blocks stride over three rounds of tiles
BIG_STEPS = 4
BIG_TOP = 96


def big_positions():
    """Where the 96 best candidates are put.  The launch has 2048 tile blocks and
    4099 tiles; block k takes tiles k, 2048 + k, 4096 + k.  The first and last lane
    pair of rounds 0, 1, 2 of the first block (tiles 0, 2048, 4096) and of rounds
    0, 1 of the last block (tiles 2047, 4095: it has no third round); the lone
    pair of the final partial tile 4098; the rest over other blocks' second rounds
    and the only other third-round tile, 4097."""
    pos = []
    for t in (0, 2048, 4096, 2047, 4095):
        pos += [t * 512, t * 512 + 1, t * 512 + 510, t * 512 + 511]
    pos += [4098 * 512, 4098 * 512 + 1]
    k = 0
    while len(pos) < BIG_TOP:
        t = 4097 if k % 5 == 0 else 2048 + 1 + (k * 397) % 2046
        pos.append(t * 512 + (k * 131) % 512)
        k += 1
    assert len(set(pos)) == BIG_TOP and max(pos) < BIG_N
    return pos


def place_best(v, b, costs, positions):
    """Swap whole columns so that the len(positions) best candidates by (cost,
    index) sit at `positions`, best first (the multiset of costs is kept).
    Returns (v, b, costs) of the permuted input."""
    n = len(costs)
    best = expected_order(costs)[:len(positions)]
    perm = np.arange(n)                       # new column -> original column
    for orig, pos in zip(best, positions):
        cur = int(np.flatnonzero(perm == orig)[0])
        perm[cur], perm[pos] = perm[pos], perm[cur]
    return np.ascontiguousarray(v[:, perm]), np.ascontiguousarray(b[:, perm]), costs[perm]


# ----------------------------------------------------------------------------
# the cases' problems (shared by the CPU preconditions and the GPU cases)
# ----------------------------------------------------------------------------
MODES = ("qk21", "rect", "qk21+rot", "rect+rot", "rect+cum")
WHEELBASES = (0.5, 0.45)      # the power-of-two and the divided form
MARGIN = 1e-9                 # obstacle_cases.MARGIN
# the batched entry's robots: three poses over the same columns
BATCH_POSES = (START[:3], (0.25, -0.05, 0.8), (0.1, -0.2, 0.6))
DT = 0.05                     # config.py's delta_t


def chain_batch_a(n_steps, n=N_CAND):
    """The chained cases' first batch A: a grid batch of the ranked batch's
    shape that is never edited."""
    v, b = grid_batch(n, n_steps, 900 + n_steps)
    v.flags.writeable = b.flags.writeable = False
    return v, b


def problem_after(pose, L):
    """The second step's problem of an episode whose first step moved to `pose`
    (episode.logged_step_problems: t += delta_t per step)."""
    t = (0.0 + DT) + DT
    return problem(L, pose, t, t + DT)
