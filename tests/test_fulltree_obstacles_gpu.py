"""Keep-out circles in the full-tree kernels (csrc/mpc_fulltree.h's hook,
csrc/mpc_fulltree_obs.h) against the host replica, bit for bit
(tests/fulltree_obstacle_cases.py; its model and scenes are checked without a
GPU in test_fulltree_obstacles_cpu.py).

Production library, public ABI.  Every shard of every split of a scene must
report the model's record — leaf, cost bits, found, s1, k[], v[], beta[] and the
three layer states, `==` — and the model's count of blocked leaves.  The
episodes compare the device-resident driver with the host lockstep driver,
record for record."""
import math

import numpy as np
import pytest

import fulltree_cases as F
import fulltree_obstacle_cases as FO

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-9      # the one-shot entry's host constants against the device's
COST_RTOL = 1e-12     # (the bars of tests/test_fulltree_gpu.py for the same pair)


def _scene(engine, name, s1, mode, L=F.WHEELBASE):
    c, circles = FO.scene_case(name, s1, mode, True, L)
    m = FO.model(c, circles)
    shards = FO.n_list(s1)
    what = f"{name} S1 {s1} {mode}" + (f" L {L}" if L != F.WHEELBASE else "")
    log, counts, rows = FO.run_sweep(engine, c, circles, shards)
    n = FO.check_sweep(log, counts, rows, m, shards, what)
    print(f"{what}: {n} launches, {len(circles)} circles, {int(m.blocked.sum())} of {s1 ** 3} "
          f"leaves blocked, {int((log[:, 1] < 0).sum())} shards without a winner")
    return c, circles, m, log, counts, shards


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("s1", FO.SMALL + FO.LARGE)
@pytest.mark.parametrize("name", FO.SCENES)
def test_every_shard_of_a_scene(engine, name, s1, mode):
    """The static scenes at S1 = 5 (one group, 39 clamped lanes), 9 (a 17-lane
    last group), 14 (quads and a tail of two), 65 (S1 % 4 = 1) and 72 (no
    clamped lane): records and counts of every shard."""
    c, circles, m, log, counts, shards = _scene(engine, name, s1, mode)
    if name == "all":           # no winner anywhere; the count is the shard's real leaves
        assert (log[:, 1] == -1).all() and (log[:, 2] & 0xFFFFFFFF == 0).all()
        assert counts[0] == s1 ** 3
    if name == "far16":         # nothing reachable: the plain entry's bytes, count 0
        plain, _ = F.run_sweep(engine, c, shards)
        assert np.array_equal(log, plain) and (counts == 0).all()
    if name == "nan":           # NaN leaves neither win nor count
        assert np.isnan(c.costs).any() and counts[0] == int(m.blocked.sum())
        assert not np.isnan(c.costs[log[log[:, 1] >= 0, 1]]).any()


def test_non_rotation_body(engine):
    """L = 0.25 raises the launch-wide flag: the direct-trig body with circles."""
    c, *_ = _scene(engine, "graze", 14, "rect+rot", F.WHEELBASE_NO_ROT)
    assert c.no_rot == 1


@pytest.mark.parametrize("s1,mode", [(9, "qk21"), (14, "rect"), (14, "qk21+rot"),
                                     (14, "rect+rot"), (65, "qk21"), (65, "rect+rot")])
def test_peel_ranks_the_top_leaves(engine, s1, mode):
    """Sixteen rounds: a tiny circle on the current winner's leaf state, launch
    again (1 and 3 shards); the device names the model's next winner every time."""
    c = F.case(s1, "move", mode, F.WHEELBASE, None, True)
    circles, winners = [], []
    for rnd in range(FO.PEEL_ROUNDS):
        m = FO.model(c, circles)
        log, counts, rows = FO.run_sweep(engine, c, circles, [1, 3])
        FO.check_sweep(log, counts, rows, m, [1, 3], f"peel round {rnd} S1 {s1} {mode}")
        winners.append(int(log[0, 1]))
        nxt = FO.peel_next(m)
        if nxt is None:
            break
        circles.append(nxt)
    assert len(set(winners)) == len(winners) == FO.PEEL_ROUNDS
    print(f"peel S1 {s1} {mode}: winners {winners}")


def _batched(engine, problems, incumbents, V, B, mode, circles, count=True,
             window=(F.WHEELBASE, F.T_A, F.T_B)):
    import torch
    from diplomjourney_amd.abi import FT_RESULT_BYTES, MpcFulltreeProblem
    from diplomjourney_amd.expansion import fulltree_argmin_batched
    arr = (MpcFulltreeProblem * len(problems))(*problems)
    pd = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(engine.device)
    inc = torch.tensor(incumbents, dtype=torch.float64, device=engine.device)
    vg = torch.tensor(V, dtype=torch.float64, device=engine.device)
    bg = torch.tensor(B, dtype=torch.float64, device=engine.device)
    out = torch.zeros(len(problems) * FT_RESULT_BYTES, dtype=torch.uint8, device=engine.device)
    counts = torch.full((len(problems),), -1, dtype=torch.int64, device=engine.device)
    fulltree_argmin_batched(engine, pd, inc, *window, vg, bg, mode, out=out,
                            obstacles=circles, n_blocked=counts if count else None)
    return (out.cpu().numpy().view(np.int64).reshape(len(problems), F.REC_WORDS),
            counts.cpu().numpy())


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("s1", [14, 65])
def test_batched_entry_one_table(engine, s1, mode):
    """mpc_fulltree_argmin_batched_obstacles on the five batch problems with ONE
    table (the start_inside and pair circles of problem `move`, which `stay`
    and `near` share the pose of), against the replica with the device's
    constants: each robot's record and count."""
    cases = [F.case(s1, name, mode, F.WHEELBASE, None, True, True) for name in F.BATCH_PROBLEMS]
    circles = FO.scene("start_inside", cases[0]) + FO.scene("pair", cases[0])
    models = [FO.model(c, circles) for c in cases]
    win = [F.expected_records(m.minima, 1) for m in models]
    leaf = np.array([w[0][0] for w in win])
    cost = np.array([w[1][0] for w in win])
    states = np.stack([m.states[max(int(l), 0)] for m, l in zip(models, leaf)])
    found = np.arange(len(cases)) % 2
    inc = np.where(found == 1, np.nextafter(cost, math.inf), cost)
    found = found * (leaf >= 0)
    log, counts = _batched(engine, [c.problem for c in cases], inc, cases[0].V, cases[0].B, mode,
                           circles)
    F.check_records(log, s1, cases[0].V, cases[0].B, leaf, cost, found, states,
                    lambda i: f"robot {i} (problem {F.BATCH_PROBLEMS[i]})",
                    f"batched with circles S1 {s1} {mode}")
    assert counts.tolist() == [int(m.blocked.sum()) for m in models]
    assert counts[0] > 0


@pytest.mark.parametrize("mode", ["qk21", "rect+rot"])
def test_no_circles_is_the_plain_entry(engine, mode):
    """n_obstacles == 0: the plain entries' bytes, and a count of 0."""
    s1 = 14
    c = F.case(s1, "move", mode, F.WHEELBASE, None, True)
    shards = [1, 3, 5]
    log, counts, _ = FO.run_sweep(engine, c, [], shards)
    plain, _ = F.run_sweep(engine, c, shards)
    assert np.array_equal(log, plain) and (counts == 0).all()
    problems = [F.problem(name) for name in F.BATCH_PROBLEMS]
    inc = [math.inf] * len(problems)
    got, counts = _batched(engine, problems, inc, c.V, c.B, mode, [])
    assert np.array_equal(got, F.run_batched(engine, problems, inc, c.V, c.B, mode))
    assert (counts == 0).all()


# ----------------------------------------------------------------------------
# the episodes
# ----------------------------------------------------------------------------
def _episode_scene(rmm):
    """12 of the script's episodes, a circle across the routes of the first six,
    robot 6 starting inside a circle it can leave; and a thirteenth robot walled
    in from its first call (every state it can reach lies inside its circle)."""
    starts = rmm.draw_starts(12, seed=3)
    step = rmm.v_max * rmm.delta_t
    circles = []
    for (x0, y0, _, xt, yt) in starts[:6]:
        d = math.hypot(xt - x0, yt - y0)
        circles.append((x0 + 3 * step * (xt - x0) / d, y0 + 3 * step * (yt - y0) / d,
                        1.2 * step))
    circles.append((starts[6][0], starts[6][1], 0.6 * step))
    walled = (40.0, 40.0, 0.3, 45.0, 44.0)
    circles.append((walled[0], walled[1], 1.0))
    return starts, walled, circles


@pytest.mark.parametrize("integ", ["qk21", "rect+rot"])
def test_device_episodes_equal_lockstep_driver_with_circles(engine, integ):
    """run_batched(obstacles=...) == run_batched_lockstep(obstacles=...), record
    for record (the comparison of test_device_episodes_equal_lockstep_driver),
    at workload G's grid (S1 = 5 x 13); the per-robot counts are the sums of the
    lockstep driver's per-call counts; chunk=4 equals one chunk; the walled-in
    robot raises the script's TypeError in both drivers and stops on the device
    with MPC_EP_NO_TRAJ after one call, every leaf blocked."""
    from diplomjourney_amd import run_math_model as rmm
    from diplomjourney_amd.abi import MPC_EP_NO_TRAJ
    rmm.configure(0.25, math.radians(10))
    try:
        starts, walled, circles = _episode_scene(rmm)
        s1 = int(rmm.size_max_1)
        ref_stats, dev_stats = {}, {}
        ref = rmm.run_batched_lockstep(starts, max_calls=9, integrator=integ, obstacles=circles,
                                       stats=ref_stats)
        dev = rmm.run_batched(starts, max_calls=9, integrator=integ, obstacles=circles,
                              stats=dev_stats)
        assert sum(len(r) for r, _ in dev) > 50
        for (rd, sd), (rr, sr) in zip(dev, ref):
            assert sd == sr and len(rd) == len(rr)
            for a, b in zip(rd, rr):
                assert a["ret"] == b["ret"] and a["optimal_criterion"] == b["optimal_criterion"]
                assert a["pre"] == b["pre"]
        # the circles matter: not the episodes of the open plane
        assert dev != rmm.run_batched(starts, max_calls=9, integrator=integ, obstacles=())
        assert rmm.run_batched(starts, max_calls=9, integrator=integ, chunk=4,
                               obstacles=circles) == dev
        # counts: per robot over one run of all calls, walled-in robot included
        eps = rmm.device_ft_episodes(starts + [walled], 9, integ, 16, obstacles=circles)
        eps.run(9)
        blocked = eps.read_blocked()
        calls, stop, _ = eps.read_progress()
        assert blocked[:len(starts)].tolist() == ref_stats["blocked"]
        assert dev_stats["blocked"] == sum(ref_stats["blocked"]) > 0
        assert blocked[6] > 0                               # started inside, and left
        assert len(dev[6][0]) > 1 and dev[6][0][0]["ret"][:2] != list(starts[6][:2])
        assert calls[-1] == 1 and stop[-1] & MPC_EP_NO_TRAJ and blocked[-1] == s1 ** 3
        for fn in (rmm.run_batched, rmm.run_batched_lockstep):
            with pytest.raises(TypeError):
                fn(starts + [walled], max_calls=3, integrator=integ, obstacles=circles)
    finally:
        rmm.configure()


def test_predictive_control_reads_the_barriers(engine):
    """The drop-in predictive_control with a registered barrier returns the
    batched entry's result of the same problem and table (the one-shot entry's
    host constants against the device's: the bars of tests/test_fulltree_gpu.py),
    and not the open plane's."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import run_math_model as rmm
    from diplomjourney_amd.abi import MpcFulltreeProblem
    rmm.configure(0.25, math.radians(20))
    try:
        start = rmm.draw_starts(1, seed=11)[0]
        rmm.start_episode(*start)
        free = rmm.predictive_control(rmm.x, rmm.y, rmm.phi, rmm.v, rmm.x_t, rmm.y_t)
        circle = (free[0], free[1], 0.2 * rmm.v_max * rmm.delta_t)   # on the free winner's layer 0
        mmt.clear_barriers()
        mmt.add_barrier_circle(*circle)
        rmm.start_episode(*start)
        inc = rmm.optimal_criterion
        got = rmm.predictive_control(rmm.x, rmm.y, rmm.phi, rmm.v, rmm.x_t, rmm.y_t)
        assert got != free
        assert math.hypot(got[0] - circle[0], got[1] - circle[1]) >= circle[2]
        p = MpcFulltreeProblem(float(start[0]), float(start[1]), float(start[2]), float(start[3]),
                               float(start[4]), float(start[0]), float(start[1]),
                               float(np.arctan(start[3] / start[4])), float(rmm.L), float(rmm.t),
                               float(rmm.t + rmm.delta_t))
        log, _ = _batched(engine, [p], [inc], rmm.vector_v, rmm.vector_beta, rmm.INTEGRATOR,
                          [circle], count=False,
                          window=(float(rmm.L), p.t_a, p.t_b))
        assert log[0, 2] & 0xFFFFFFFF == 1
        w = log[0].copy().view(np.float64)
        assert got[3:] == [w[6], w[9]]                                # v[0], beta[0]
        assert max(abs(a - b) for a, b in zip(got[:3], w[12:15])) <= STATE_TOL
        assert math.isclose(rmm.optimal_criterion, w[0], rel_tol=COST_RTOL)
    finally:
        mmt.clear_barriers()
        rmm.configure()
