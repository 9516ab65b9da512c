"""Keep-out polygons in the device-resident episode steps
(mpc_episode_step_keepout, mpc_episode_chain_step_keepout through
DeviceEpisode(polygons=...)).

Every expectation is the host replica's (harness.replica_rollout with the
device's reciprocal estimates and constants: its costs are the kernels' bit for
bit).  The expected mask has no margin in any mode: it is the verdict of the
host build of the kernels' own table functions with the episode's constants
(tests/episode_keepout_harness.cpp through episode_keepout_cases) on the
replica's states, or for rect+cum on the recurrence's sums.  Before a result is
looked at that mask is compared with the exact rule and the scene's conditions
are asserted (ranking.check_polygon_scene).  The ranked cases peel every
unblocked candidate (tests/ranking.py); n_blocked must be the mask's count in
every launch."""
import sys

import numpy as np
import pytest
import torch

import episode_keepout_cases as KC
import episode_obstacle_cases as EC
import polygon_cases as pc
import ranking as R
from harness import replica_rollout
from test_episode_obstacles_gpu import (_LOG_SEL, COST_RTOL, INC_MAX, STATE_TOL, _dev, _resident)

pytestmark = pytest.mark.gpu

assert INC_MAX == float(sys.maxsize)


def _episode(engine, n, n_steps, mode, L, start=R.START, target=R.TARGET, **kw):
    from diplomjourney_amd.episode import DeviceEpisode
    kw.setdefault("log_capacity", 8)
    return DeviceEpisode(engine, n, n_steps, integrator=mode, start=start, target=target,
                         incumbent0=INC_MAX, L=L, **kw)


def _square(c, h):
    return [(c[0] - h, c[1] - h), (c[0] + h, c[1] - h), (c[0] + h, c[1] + h), (c[0] - h, c[1] + h)]


# ----------------------------------------------------------------------------
# 1. the first step ranked, two-launch form
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", KC.FIRST_STEP, ids=KC.case_id)
def test_rank_first_step(engine, kw):
    """DeviceEpisode.step(controls=...) from reset() at a placement's pose, with
    that placement's scene: every unblocked candidate in the replica's order,
    n_blocked the mask's count in every launch.  (n = 1025: the scalar path;
    mixed: the 16-circle instantiations; every other case polygons alone.)"""
    from diplomjourney_amd.episode import logged_step_problems
    c = KC.first_step(**kw, device=True)
    x, y, phi, L = pc.PLACEMENTS[c.name]
    n, n_steps = c.inp.n, c.inp.n_steps
    ep = _episode(engine, n, n_steps, c.mode, L, start=(x, y, phi) + R.START[3:],
                  target=(c.problem.x_t, c.problem.y_t), polygons=c.polygons, obstacles=c.circles)
    vd, bd = _dev(c.inp.v), _dev(c.inp.b)
    assert n % 2 or (vd.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0)
    # the episode's first problem is the placement's, before any result is looked at
    ep.step(controls=(vd, bd))
    first = logged_step_problems(ep.read_log()[:1], ep.cfg)[0][0]
    assert first.as_tuple() == pc.placed_problem(c.name).as_tuple() == c.problem.as_tuple()

    def launch():
        ep.reset()
        ep.step(controls=(vd, bd))
        return torch.cat([R.result_words(ep.local), ep.n_blocked.view(1, 1)], dim=1)

    got = R.peel(launch, vd, R.soa_offset(), c.n_free + 2)[:, 0]
    n_blocked = int(c.mask.sum())
    assert (got[:, R.REC_WORDS] == n_blocked).all(), (got[0, R.REC_WORDS], n_blocked)
    assert R.check_ranking(got, c.costs, excluded=c.mask, states=c.states,
                           what=c.what) == c.n_free
    print(f"{c.what}: ranked {c.n_free} candidates ({n_blocked} blocked, {len(c.polygons)} "
          f"polygons, {len(c.circles)} circles"
          f"{', an edge through candidate %d' % c.through[0] if c.through else ''})")


# ----------------------------------------------------------------------------
# 2 and 3. the second step ranked, chained form
# ----------------------------------------------------------------------------
def _rank_second_step(engine, tiled, L, n_steps, make_b, va, ba, top=None, what=""):
    """test_episode_obstacles_gpu._rank_second_step with polygons: per peel
    reset, step A (fixed), step B (ranked), flush, so B's rollout runs with A
    pending and its tile blocks wait for block 0 to publish B's pose.  B's
    problem is rebuilt from A's log record; make_b(problem, pose, traj_a) ->
    (v, b, states, costs, polygons, circles, mask).  A runs under B's tables
    too (make_b asserts its winner clear of them): it must be the unobstructed
    one in every peel."""
    from diplomjourney_amd.abi import MPC_EP_ARRIVED, MPC_EP_BREAK, MPC_EP_LIMIT
    from diplomjourney_amd.episode import logged_step_problems
    n = va.shape[1]
    ep = _episode(engine, n, n_steps, "rect+cum", L, chain=True)
    A = _resident(va, ba, tiled)

    def steps(batches):
        ep.reset()
        for c in batches:
            ep.step(controls=c)
        ep.flush()

    steps([A])
    rec_a = ep.read_log()[0]
    assert rec_a.found == 1 and rec_a.index >= 0
    assert not rec_a.status & (MPC_EP_ARRIVED | MPC_EP_BREAK | MPC_EP_LIMIT)
    p_b = logged_step_problems([rec_a, rec_a], ep.cfg)[1][0]
    pose = (rec_a.x, rec_a.y, rec_a.phi)
    assert p_b.as_tuple() == R.problem_after(pose, L).as_tuple()
    traj_a, pose_a = EC.batch_a_winner(L, n_steps, device=True, batch=(va, ba))
    assert pose_a == pose
    v, b, st, costs, polygons, circ, mask = make_b(p_b, pose, traj_a)
    ep.set_polygons(polygons)
    ep.set_obstacles(circ)
    B = _resident(v, b, tiled)
    sel = torch.tensor(_LOG_SEL, device="cuda")

    def launch():
        steps([A, B])
        words = ep.log.view(torch.int64).index_select(0, sel)
        return torch.cat([R.result_words(ep.local)[0], words, ep.n_blocked]).view(1, -1)

    n_free = int((np.isfinite(costs) & ~mask).sum())
    n_peels = top if top is not None else n_free + 2
    off = R.tiled_offset(n_steps) if tiled else R.soa_offset()
    got = R.peel(launch, B if tiled else B[0], off, n_peels)[:, 0]
    assert ep.chain_error() == 0
    a_idx, a_cost = got[:, R.REC_WORDS], got[:, R.REC_WORDS + 1]
    assert (a_idx == rec_a.index).all() and (a_cost == a_cost[0]).all()
    assert R._f64(a_cost[:1])[0] == rec_a.cost
    assert (got[:, -1] == int(mask.sum())).all(), (got[0, -1], int(mask.sum()))
    n_ranked = R.check_ranking(got, costs, excluded=mask, states=st, top=top,
                               what=what + " (result)")
    R.check_ranking(got[:, R.REC_WORDS + 2:], costs, excluded=mask, states=st, top=top,
                    what=what + " (log)")
    if top is None:
        assert n_ranked == n_free
    return n_ranked


@pytest.mark.parametrize("L,n_steps,mixed", KC.SECOND_STEP)
@pytest.mark.parametrize("layout", ("soa", "tiled"))
def test_rank_chained_second_step(engine, layout, L, n_steps, mixed):
    va, ba = R.chain_batch_a(n_steps)

    def make_b(p_b, pose, traj_a):
        c = KC.second_step(L, n_steps, mixed, device=True, pose=pose, traj_a=traj_a)
        assert c.problem.as_tuple() == p_b.as_tuple()
        assert len(c.polygons) == 4 and len(c.circles) == (3 if mixed else 0)
        return c.inp.v, c.inp.b, c.states, c.costs, c.polygons, c.circles, c.mask

    what = f"chained {layout} L={L} N={n_steps}, 4 polygons{' and 3 circles' if mixed else ''}"
    n = _rank_second_step(engine, layout == "tiled", L, n_steps, make_b, va, ba, what=what)
    print(f"{what}: ranked {n} candidates")


def test_chained_tiled_at_grid_shape(engine):
    """ranking.BIG_N x BIG_STEPS, tiled: 2048 tile blocks stride over three
    rounds of tiles and form the frame table anew for each tile (behind pre0's
    barrier).  One octagon on the
    unconstrained winner's final state; n_blocked is the mask's count over all
    candidates; the first 8 peeled winners are the replica's."""
    va, ba = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[0])
    top = 8

    def make_b(p_b, pose, traj_a):
        v, b = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[1])
        costs, polygons, mask = KC.big_scene(p_b, v, b, traj_a, device=True)
        assert (np.isfinite(costs) & ~mask).sum() >= top
        return v, b, None, costs, polygons, [], mask

    what = "chained tiled at the grid shape, one octagon"
    assert _rank_second_step(engine, True, 0.5, R.BIG_STEPS, make_b, va, ba, top=top,
                             what=what) == top


# ----------------------------------------------------------------------------
# 4. a restart inside a chain
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.WHEELBASES)
@pytest.mark.parametrize("layout", ("soa", "tiled"))
def test_restart_inside_a_chain(engine, layout, L):
    """max_steps = 1: every step ends its episode, so every chained launch
    follows a restart.  Each logged winner is the replica's best unblocked
    candidate of the problem rebuilt from the log."""
    from diplomjourney_amd.abi import MPC_EP_LIMIT
    from diplomjourney_amd.episode import logged_step_problems
    n_steps, tiled = 3, layout == "tiled"
    inp = R.controls(n_steps)
    va, ba = R.chain_batch_a(n_steps)
    with KC.placement(f"START, L={L}", R.START[:3], L) as name:
        c = KC.scene(name, R.problem(L), "rect+cum", inp, n_steps, device=True)
    ep = _episode(engine, inp.n, n_steps, "rect+cum", L, chain=True, max_steps=1,
                  polygons=c.polygons)
    host = [(inp.v, inp.b), (va, ba), (inp.v, inp.b)]
    for v, b in host:
        ep.step(controls=_resident(v, b, tiled))
    log = ep.read_log()
    assert len(log) == 3 and ep.chain_error() == 0
    probs = logged_step_problems(log, ep.cfg)
    for k, (rec, (p, _), (v, b)) in enumerate(zip(log, probs, host)):
        assert rec.status & MPC_EP_LIMIT
        st, costs = replica_rollout(p, v, b, "rect+cum", device_estimates=True,
                                    device_consts=True)
        sums, bad = KC.cum_sums(p, v, b, device=True)
        mask = KC.host_mask(p, c.polygons, "rect+cum", st, sums, bad).any(axis=0)
        assert mask.sum() < inp.n
        if v is inp.v:      # (the scene was made for this batch)
            assert mask.sum() > 0
            assert mask[int(R.expected_order(costs)[0])], "the unconstrained winner is not blocked"
        want = int(R.expected_order(costs, excluded=mask)[0])
        assert (rec.index, rec.found) == (want, 1), (k, R.where(rec.index), R.where(want))
        assert rec.cost == costs[want]
        assert (rec.x, rec.y, rec.phi) == tuple(st[0, :, want])


# ----------------------------------------------------------------------------
# 5. a polygon nothing reaches
# ----------------------------------------------------------------------------
FORMS = ("sampler", "controls", "chained soa", "chained tiled")


@pytest.mark.parametrize("form", FORMS)
def test_unreached_polygon_changes_nothing(engine, form):
    """12 steps (max_steps = 5: restarts included) with a square 7 m away: the
    log, its raw bytes and the EpisodeState bytes are those of the same episode
    without polygons, and nothing is counted."""
    n_steps, n = 3, R.N_CAND
    batches = [R.grid_batch(n, n_steps, 700 + i) for i in range(3)]
    far = [pc.ngon(pc.ahead("start", 7.0, 0.8), 0.5, 4, R.START[2])]

    def run(polygons):
        ep = _episode(engine, n, n_steps, "rect+cum", 0.5, chain=form.startswith("chained"),
                      max_steps=5, log_capacity=16, polygons=polygons)
        res = [_resident(v, b, form == "chained tiled") for v, b in batches]
        for i in range(12):
            ep.step(controls=None if form == "sampler" else res[i % 3])
        log = ep.read_log()
        torch.cuda.synchronize()
        assert ep.chain_error() == 0
        return ([bytes(r) for r in log], ep.state.cpu().numpy().tobytes(),
                int(ep.n_blocked.item()), ep.log.cpu().numpy().tobytes())

    plain, fenced = run(()), run(far)
    assert len(plain[0]) == 12
    assert fenced[0] == plain[0] and fenced[3] == plain[3]
    assert fenced[1] == plain[1]
    assert fenced[2] == 0


# ----------------------------------------------------------------------------
# 6. the keep-out entries without polygons
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("counted", (True, False))
@pytest.mark.parametrize("circles", (False, True))
@pytest.mark.parametrize("form", ("controls", "chained soa", "chained tiled"))
def test_keepout_entries_without_polygons(engine, form, circles, counted):
    """The _keepout entries with n_polygons = 0, reached through a DeviceEpisode
    whose hook takes them without polygons, with a counted and with a NULL
    n_blocked_out: 6 steps (max_steps = 3: a restart included) over 1026
    candidates leave the log, its raw bytes and the EpisodeState bytes of the
    plain entries (no circles) or of the _obstacles entries (circles), and the
    same count."""
    from diplomjourney_amd.episode import DeviceEpisode
    n_steps, n = 3, 1026
    batches = [R.grid_batch(n, n_steps, 800 + i) for i in range(3)]
    # on the path: 0.07 to 0.13 m ahead of the start pose, which every step's rollout crosses
    circ = [(*pc.ahead("start", 0.1, 0.0), 0.03), (5.0, 5.0, 0.5)] if circles else []

    class KeepoutEntries(DeviceEpisode):
        def _polygon_args(self):
            return None, 0

        def _obstacle_args(self):
            return self._obs, self._n_obs, self.n_blocked.data_ptr() if counted else None

    def run(cls):
        ep = cls(engine, n, n_steps, integrator="rect+cum", start=R.START, target=R.TARGET,
                 incumbent0=INC_MAX, L=0.5, chain=form.startswith("chained"), max_steps=3,
                 log_capacity=8, obstacles=circ)
        ep.n_blocked.fill_(77)       # (the obstacle and keep-out entries zero it on the stream)
        res = [_resident(v, b, form == "chained tiled") for v, b in batches]
        for i in range(6):
            ep.step(controls=res[i % 3])
        log = ep.read_log()
        torch.cuda.synchronize()
        assert ep.chain_error() == 0
        assert len(log) == 6 and max(r.episode for r in log) >= 2, "no restart"
        return ([bytes(r) for r in log], ep.log.cpu().numpy().tobytes(),
                ep.state.cpu().numpy().tobytes(), int(ep.n_blocked.item()))

    plain, entries = run(DeviceEpisode), run(KeepoutEntries)
    assert entries[:3] == plain[:3]
    if circles:
        assert plain[3] > 0, "the circle blocks nobody"
        assert entries[3] == (plain[3] if counted else 77)
    else:
        assert plain[3] == 77 and entries[3] == (0 if counted else 77)


# ----------------------------------------------------------------------------
# 7. everything blocked
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("two-launch", "chained"))
def test_everything_blocked(engine, form):
    from diplomjourney_amd.abi import MPC_EP_STALE, result_from_bytes
    n_steps = 3
    va, ba = R.chain_batch_a(n_steps)
    n = va.shape[1]
    assert np.isfinite(va).all() and np.isfinite(ba).all()
    ep = _episode(engine, n, n_steps, "rect+cum", 0.5, chain=form == "chained",
                  polygons=[_square(R.START[:2], 10.0)])
    ep.step(controls=_resident(va, ba, False))
    rec, = ep.read_log()
    assert (rec.found, rec.index) == (0, -1) and rec.status & MPC_EP_STALE
    assert (rec.x, rec.y, rec.phi) == R.START[:3]
    assert int(ep.n_blocked.item()) == n
    res = result_from_bytes(ep.local.cpu().numpy().tobytes())
    assert (res.found, res.index) == (0, -1)
    assert ep.chain_error() == 0


# ----------------------------------------------------------------------------
# 8. closed loop against the host episode
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("rect", "rect+rot", "rect+cum"))
def test_closed_loop_avoids_the_square(engine, mode):
    """Episode(polygons=g) against DeviceEpisode(polygons=g), 120 steps of
    20 000 x 10: a square of half-side 0.15 sits on the unobstructed run's pose
    at step 25.  rect and rect+rot are world frame (the host's and the device's
    tables are the same numbers): every step's index, p, found and status
    identical.  rect+cum (the device's own frame table): no found step ends
    strictly inside."""
    import math
    from diplomjourney_amd.episode import DeviceEpisode, Episode
    n, ns, steps = 20_000, 10, 120
    free = DeviceEpisode(engine, n, ns, integrator=mode, log_capacity=512)
    for _ in range(steps):
        free.step()
    path = free.read_log()
    g = _square((path[25].x, path[25].y), 0.15)

    def inside(r):
        return bool(pc.inside(np.float64(r.x), np.float64(r.y), g))

    assert any(inside(r) for r in path)
    dev = DeviceEpisode(engine, n, ns, integrator=mode, log_capacity=512, polygons=[g])
    for _ in range(steps):
        dev.step()
    got = dev.read_log()
    assert len(got) == steps
    assert not any(inside(r) for r in got if r.found)
    if mode == "rect+cum":
        return
    host = Episode(engine, n, ns, integrator=mode, polygons=[g])
    want = []
    for _ in range(steps):
        host.step()
        want.append(host.last_log)
    for a, w in zip(got, want):
        assert (a.index, a.p, a.found, a.status) == (w[0], w[2], w[8], w[9])
        assert math.isclose(a.cost, w[1], rel_tol=COST_RTOL)
        assert max(abs(p - q) for p, q in zip((a.x, a.y, a.phi, a.v, a.beta), w[3:8])) <= STATE_TOL


# ----------------------------------------------------------------------------
# 9. refused forms, and set_polygons on a pending chained step
# ----------------------------------------------------------------------------
def test_refused_combinations(engine):
    from diplomjourney_amd.episode import DeviceEpisode
    one = [pc.OK_POLYGON]
    for kw in (dict(generate=True), dict(split=False), dict(chain=True, exchange=True),
               dict(chain=True, exchange=True, p2p=True),
               dict(chain=True, exchange=True, overlap=True)):
        with pytest.raises(ValueError, match="circles and polygons: the two-launch step"):
            DeviceEpisode(engine, 1024, 3, integrator="rect+cum", polygons=one, **kw)
        ep = DeviceEpisode(engine, 1024, 3, integrator="rect+cum", **kw)
        try:
            with pytest.raises(ValueError, match="chained step"):
                ep.set_polygons(one)
            ep.set_polygons(())            # none: every form takes that
        finally:
            ep.close()
    ep = DeviceEpisode(engine, 1024, 3, integrator="rect+cum", chain=True, polygons=one)
    v, b = R.grid_batch(1024, 3, 5)
    with pytest.raises(ValueError, match="run"):
        ep.run([(_dev(v), _dev(b))])
    with pytest.raises(ValueError, match="at most 4"):
        ep.set_polygons(one * 5)
    with pytest.raises(ValueError, match="convex pieces"):
        ep.set_polygons([[(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)]])
    # the supported forms take them: split two-launch, also as the multi-GPU step on one rank
    for kw in (dict(), dict(chain=True)):
        DeviceEpisode(engine, 1024, 3, integrator="rect+cum", polygons=one, **kw).step()
    ep = DeviceEpisode(engine, 1024, 3, integrator="rect+cum", polygons=[_square((0.0, 0.0), 10.0)],
                       exchange=True)
    ep.expand()
    torch.cuda.synchronize()
    assert int(ep.n_blocked.item()) == 1024


@pytest.mark.parametrize("layout", ("soa", "tiled"))
def test_set_polygons_completes_a_pending_step(engine, layout):
    """set_polygons() on a chained episode with a step pending: that step is
    flushed first (its rollout ran under the previous polygons), so its record
    is the unobstructed winner's, and the next step runs under the new ones."""
    n_steps = 3
    va, ba = R.chain_batch_a(n_steps)
    n = va.shape[1]
    ep = _episode(engine, n, n_steps, "rect+cum", 0.5, chain=True)
    A = _resident(va, ba, layout == "tiled")
    ep.step(controls=A)
    assert ep._pending is not None and ep.steps_enqueued == 0
    ep.set_polygons([_square(R.START[:2], 10.0)])
    assert ep._pending is None and ep.steps_enqueued == 1
    ep.step(controls=A)
    first, second = ep.read_log()
    traj_a, pose = EC.batch_a_winner(0.5, n_steps, device=True, batch=(va, ba))
    assert first.found == 1 and (first.x, first.y, first.phi) == pose
    assert (second.found, second.index) == (0, -1)
    assert int(ep.n_blocked.item()) == n and ep.chain_error() == 0
