"""The preconditions of every case of tests/test_episode_keepout_gpu.py, on the
IEEE replica with the episode's constants (device_consts=True) and without a
GPU: ranking.check_polygon_scene's — the host-built mask equals the exact rule
(polygon_cases.exact_inside) on every state outside the header's bound plus
the sums' distance, at most 1 % of the states are left unjudged, 10 to 90 % of
the candidates are blocked, the unconstrained winner among them, a mid-horizon
block and the rest — and, for the chained cases, that step A's winner, which
runs under step B's tables too, lies outside every polygon of B and clear of
its circles."""
from fractions import Fraction as F

import numpy as np
import pytest

import episode_keepout_cases as KC
import episode_obstacle_cases as EC
import polygon_cases as pc
import ranking as R


@pytest.mark.parametrize("kw", KC.FIRST_STEP, ids=KC.case_id)
def test_first_step_preconditions(oracle, kw):
    c = KC.first_step(**kw)
    assert 0 < c.n_free < c.n_fin
    if c.through is not None:
        assert c.through[0] not in c.inp.beta_irregular + c.inp.dphi_irregular
    if kw.get("mixed"):
        assert len(c.circles) == 3
    # the episode's first problem: the placement's pose, its own wheelbase
    assert c.problem.as_tuple() == pc.placed_problem(kw["name"]).as_tuple()
    assert c.L == pc.PLACEMENTS[kw["name"]][3]


@pytest.mark.parametrize("L,n_steps,mixed", KC.SECOND_STEP)
def test_second_step_preconditions(oracle, L, n_steps, mixed):
    before = dict(pc.PLACEMENTS)
    c = KC.second_step(L, n_steps, mixed, device=False)
    assert pc.PLACEMENTS == before            # the scene's placement is gone again
    assert 0 < c.n_free < c.n_fin and len(c.polygons) == 4
    assert c.clear > 1e-9, c.clear
    print(f"{c.what}: A's winner {c.clear:.3g} from the nearest edge line")


def test_grid_shape_preconditions(oracle):
    va, ba = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[0])
    traj_a, pose = EC.batch_a_winner(0.5, R.BIG_STEPS, device=False, batch=(va, ba))
    v, b = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[1])
    costs, polygons, mask = KC.big_scene(R.problem_after(pose, 0.5), v, b, traj_a, device=False)
    free = costs[np.isfinite(costs) & ~mask]
    assert len(free) >= 8 and len(np.unique(np.sort(free)[:9])) == 9   # no tie among the ranked


@pytest.mark.parametrize("name", list(pc.PLACEMENTS))
def test_frame_table_is_frame_edge_of_the_episode_constants(name):
    """The harness' two tables: the world table is the one-shot builder's
    (the pose does not enter it), the frame table is frame_edge's formula on
    the EPISODE's constants operation for operation, padding included, and a
    point of the sums frame is inside a frame polygon exactly when its cum_pose
    is inside the world polygon (away from the edges)."""
    p = pc.placed_problem(name)
    x0, y0, s0, c0, inv_L, pow2, L = (float(q) for q in KC.consts(p))
    assert bool(pow2) == (L in (0.5, 0.25)) and L == pc.PLACEMENTS[name][3]
    rng = np.random.default_rng(20261021)
    polygons = [pc.ngon((x0 + rng.uniform(-1, 1), y0 + rng.uniform(-1, 1)), rng.uniform(0.05, 0.6),
                        n, rng.uniform(0, 6.0), cw) for n, cw in ((3, False), (8, True), (5, False))]
    world, frame = KC.tables(p, polygons)
    assert world.tobytes() == pc.host_tables(p, polygons)[0].tobytes()

    def fma(a, b, c):            # one rounding: exact in rationals, rounded by float()
        return float(F(a) * F(b) + F(c))

    for k, ((a, b, c), got) in enumerate(zip(world.tolist(), frame.tolist())):
        cc = fma(a, x0, fma(b, y0, c))
        want = [a * c0 + b * s0, b * c0 - a * s0, cc * inv_L if pow2 else cc]
        assert got == want, (k, got, want)
    assert (world[3 * 8:, :2] == 0).all() and (world[3 * 8:, 2] == -1).all()
    assert (frame[3 * 8:, :2] == 0).all() and (frame[3 * 8:, 2] < 0).all()      # padding keeps its sign
    n_in = n_out = 0
    for g in polygons:
        P = np.asarray(g)
        cx, cy, rad = P[:, 0].mean(), P[:, 1].mean(), np.hypot(*(P[0] - P.mean(axis=0)))
        m = 2000
        xy = np.column_stack([cx + rng.uniform(-1.3, 1.3, m) * rad, cy + rng.uniform(-1.3, 1.3, m) * rad])
        dx, dy = xy[:, 0] - x0, xy[:, 1] - y0
        ab = np.column_stack([c0 * dx + s0 * dy, c0 * dy - s0 * dx]) * (inv_L if pow2 else 1.0)
        back = KC.cum_pose(p, ab)
        d = pc.edge_distances(back[:, 0], back[:, 1], g)
        clear = (np.abs(d) > 1e-9).all(axis=0)
        in_frame = pc.host_inside(frame, 3, ab)
        in_world = pc.host_inside(world, 3, back)
        assert (in_frame == in_world)[clear].all(), name
        n_in += int((in_world & clear).sum())
        n_out += int((~in_world & clear).sum())
    assert n_in > 500 and n_out > 500


def test_sums_are_the_replicas(oracle):
    """ek_cum_sums with the episode's constants: cum_pose of the sums is the
    replica's state bit for bit (KC.sums_distance asserts it), at a placement
    where the two derivations of the constants differ."""
    from harness import replica_rollout
    inp = R.controls(3)
    differ = 0
    for name in pc.PLACEMENTS:
        p = pc.placed_problem(name)
        st, _ = replica_rollout(p, inp.v, inp.b, "rect+cum", device_consts=True)
        sums, bad = KC.cum_sums(p, inp.v, inp.b)
        assert KC.sums_distance(p, st, sums, bad) < 1e-12 * max(1.0, abs(p.x) + abs(p.y))
        differ += KC.consts(p).tobytes() != pc.host_consts(p).tobytes()
    print(f"{differ} of {len(pc.PLACEMENTS)} placements: episode constants != one-shot constants")
