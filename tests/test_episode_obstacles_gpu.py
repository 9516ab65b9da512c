"""Keep-out circles in the device-resident episode steps
(mpc_episode_step_obstacles, mpc_episode_chain_step_obstacles through
DeviceEpisode(obstacles=...)).

Every expectation is the host replica's (harness.replica_rollout with the
device's reciprocal estimates and constants: its costs are the kernels' bit for
bit), with the blocked mask formed from its states by the header's formula
(ranking.blocked).  The preconditions of episode_obstacle_cases.masked are
asserted before a result is looked at.  The ranked cases peel every unblocked
candidate (tests/ranking.py)."""
import sys

import numpy as np
import pytest
import torch

import episode_obstacle_cases as EC
import ranking as R
from harness import replica_rollout

pytestmark = pytest.mark.gpu

INC_MAX = float(sys.maxsize)
STATE_TOL = 1e-9          # tests/test_gpu_parity.py
COST_RTOL = 1e-12
NOWHERE = [(5.0, 5.0, 0.5)]


def _dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def _episode(engine, n, n_steps, mode, L, **kw):
    from diplomjourney_amd.episode import DeviceEpisode
    kw.setdefault("log_capacity", 8)
    return DeviceEpisode(engine, n, n_steps, integrator=mode, start=R.START, target=R.TARGET,
                         incumbent0=INC_MAX, L=L, **kw)


def _resident(v, b, tiled):
    from diplomjourney_amd.expansion import soa_to_tiled
    vd, bd = _dev(v), _dev(b)
    return soa_to_tiled(vd, bd) if tiled else (vd, bd)


# ----------------------------------------------------------------------------
# 1. the first step ranked, two-launch form
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,L,n_steps,n", EC.FIRST_STEP)
def test_rank_first_step(engine, mode, L, n_steps, n):
    """DeviceEpisode.step(controls=...) from reset(), with 1, 4 and 16 circles
    (every streaming instantiation; 1025 columns: the scalar path's): every
    unblocked candidate in the replica's order, n_blocked the mask's count in
    every launch."""
    inp, st, costs = EC.first_step(mode, L, n_steps, n, device=True)
    assert R.check_preconditions(inp, costs) == n - 3
    for k, (circ, mask) in EC.masked(st, costs, n_steps, EC.counts_of(n)).items():
        n_free = int((np.isfinite(costs) & ~mask).sum())
        ep = _episode(engine, n, n_steps, mode, L, obstacles=circ)
        vd, bd = _dev(inp.v), _dev(inp.b)
        assert (vd.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0)

        def launch():
            ep.reset()
            ep.step(controls=(vd, bd))
            return torch.cat([R.result_words(ep.local), ep.n_blocked.view(1, 1)], dim=1)

        got = R.peel(launch, vd, R.soa_offset(), n_free + 2)[:, 0]
        what = f"episode step {mode} L={L} N={n_steps} n={n}, {k} circles"
        assert (got[:, R.REC_WORDS] == int(mask.sum())).all(), (got[0, R.REC_WORDS],
                                                                int(mask.sum()))
        assert R.check_ranking(got, costs, excluded=mask, states=st, what=what) == n_free
        print(f"{what}: ranked {n_free} candidates, {int(mask.sum())} blocked")


# ----------------------------------------------------------------------------
# 2 and 3. the second step ranked, chained form
# ----------------------------------------------------------------------------
LOG_WORDS = 10                # sizeof(mpc_episode_log_t) / 8
# A's record (slot 0): index, cost; B's (slot 1): cost, index, found | status << 32,
# then x, y, phi at the words check_ranking reads a first state from
_LOG_SEL = (1, 4, LOG_WORDS + 4, LOG_WORDS + 1, LOG_WORDS + 3, 0, 0, LOG_WORDS + 5,
            LOG_WORDS + 6, LOG_WORDS + 7)


def _rank_second_step(engine, tiled, L, n_steps, make_b, va, ba, count, top=None, what=""):
    """The structure of test_ranking_gpu._rank_second_step: per peel reset,
    step A (fixed), step B (ranked), flush, so B's rollout runs with A pending
    and its tile blocks start before block 0 has published B's constants.
    B's problem is rebuilt from A's log record; make_b(problem) -> (v, b, states,
    costs, circles, mask).  A runs under B's circles too: its winner must be
    the unobstructed one in every peel."""
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
    assert p_b.as_tuple() == R.problem_after((rec_a.x, rec_a.y, rec_a.phi), L).as_tuple()
    v, b, st, costs, circ, mask = make_b(p_b)
    assert len(circ) == count
    # A's winner, as logged, is clear of B's circles
    traj_a, pose = EC.batch_a_winner(L, n_steps, device=True, batch=(va, ba))
    assert pose == (rec_a.x, rec_a.y, rec_a.phi)
    EC.a_unblocked(traj_a, circ)
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


@pytest.mark.parametrize("count", (4, 16))
@pytest.mark.parametrize("L,n_steps", EC.SECOND_STEP)
@pytest.mark.parametrize("layout", ("soa", "tiled"))
def test_rank_chained_second_step(engine, layout, L, n_steps, count):
    inp = R.controls(n_steps)
    va, ba = R.chain_batch_a(n_steps)

    def make_b(p_b):
        st, costs = replica_rollout(p_b, inp.v, inp.b, "rect+cum", device_estimates=True,
                                    device_consts=True)
        assert R.check_preconditions(inp, costs) == inp.n - 3
        circ, mask = EC.masked(st, costs, n_steps, (count,))[count]
        return inp.v, inp.b, st, costs, circ, mask

    what = f"chained {layout} L={L} N={n_steps}, {count} circles"
    n = _rank_second_step(engine, layout == "tiled", L, n_steps, make_b, va, ba, count, what=what)
    print(f"{what}: ranked {n} candidates")


def test_chained_tiled_at_grid_shape(engine):
    """ranking.BIG_N x BIG_STEPS, tiled: 2048 tile blocks stride over three
    rounds of tiles, and the later rounds find the constants final in pre0.
    n_blocked is the mask's count over all candidates; the first 8 peeled
    winners are the replica's."""
    va, ba = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[0])
    top = 8

    def make_b(p_b):
        v, b = R.grid_batch(R.BIG_N, R.BIG_STEPS, EC.BIG_SEEDS[1])
        st, costs = replica_rollout(p_b, v, b, "rect+cum", device_estimates=True,
                                    device_consts=True)
        circ, mask = EC.masked(st, costs, R.BIG_STEPS, (4,), EC.big_circles(st, costs))[4]
        assert (np.isfinite(costs) & ~mask).sum() >= top
        return v, b, None, costs, circ, mask

    what = "chained tiled at the grid shape, 4 circles"
    assert _rank_second_step(engine, True, 0.5, R.BIG_STEPS, make_b, va, ba, 4, top=top,
                             what=what) == top


# ----------------------------------------------------------------------------
# 4. a restart inside a chain
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.WHEELBASES)
@pytest.mark.parametrize("layout", ("soa", "tiled"))
def test_restart_inside_a_chain(engine, layout, L):
    """max_steps = 1: every step ends its episode, so every chained launch
    follows a restart (t is reset: the step size differs from the one a tile
    block would speculate).  Each logged winner is the replica's best unblocked
    candidate in the problem rebuilt from the log."""
    from diplomjourney_amd.abi import MPC_EP_LIMIT
    from diplomjourney_amd.episode import logged_step_problems
    n_steps, tiled = 3, layout == "tiled"
    inp = R.controls(n_steps)
    va, ba = R.chain_batch_a(n_steps)
    _, st0, costs0 = EC.first_step("rect+cum", L, n_steps, inp.n, device=True)
    circ, _ = EC.masked(st0, costs0, n_steps, (4,))[4]
    ep = _episode(engine, inp.n, n_steps, "rect+cum", L, chain=True, max_steps=1,
                  obstacles=circ)
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
        mask, margin = R.blocked(st, circ)
        assert margin > R.MARGIN and 0 < mask.sum() < inp.n
        if v is inp.v:      # (the circles were made for this batch; they only graze batch A)
            assert mask[int(R.expected_order(costs)[0])], "the unconstrained winner is not blocked"
        want = int(R.expected_order(costs, excluded=mask)[0])
        assert (rec.index, rec.found) == (want, 1), (k, R.where(rec.index), R.where(want))
        assert rec.cost == costs[want]
        assert (rec.x, rec.y, rec.phi) == tuple(st[0, :, want])


# ----------------------------------------------------------------------------
# 5. a circle nothing reaches
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("sampler", "controls", "chained soa", "chained tiled"))
def test_unreached_circle_changes_nothing(engine, form):
    """12 steps (max_steps = 5: restarts included) with the circle (5, 5, 0.5):
    the log and the EpisodeState bytes are those of the same episode without
    circles."""
    n_steps, n = 3, R.N_CAND
    batches = [R.grid_batch(n, n_steps, 700 + i) for i in range(3)]

    def run(circles):
        ep = _episode(engine, n, n_steps, "rect+cum", 0.5, chain=form.startswith("chained"),
                      max_steps=5, log_capacity=16, obstacles=circles)
        res = [_resident(v, b, form == "chained tiled") for v, b in batches]
        for i in range(12):
            ep.step(controls=None if form == "sampler" else res[i % 3])
        log = ep.read_log()
        torch.cuda.synchronize()
        return ([bytes(r) for r in log], ep.state.cpu().numpy().tobytes(),
                int(ep.n_blocked.item()), ep.log.cpu().numpy().tobytes())

    plain, circled = run(()), run(NOWHERE)
    assert len(plain[0]) == 12
    assert circled[0] == plain[0] and circled[3] == plain[3]
    assert circled[1] == plain[1]
    assert circled[2] == 0


@pytest.mark.parametrize("counted", (True, False))
@pytest.mark.parametrize("form", ("controls", "chained soa", "chained tiled"))
def test_obstacle_entries_without_circles(engine, form, counted):
    """The obstacle entries with n_obstacles = 0 (they launch the plain
    kernels), reached through a DeviceEpisode whose hook takes them without
    circles, with a counted and with a NULL n_blocked_out: 6 steps (max_steps
    = 3: a restart included) over 1026 candidates (two full 512-tiles and one of
    a single pair) leave the log, its raw bytes and the EpisodeState bytes of
    the plain entries, and count nothing."""
    from diplomjourney_amd.episode import DeviceEpisode
    n_steps, n = 3, 1026
    batches = [R.grid_batch(n, n_steps, 800 + i) for i in range(3)]

    class ObstacleEntries(DeviceEpisode):
        def _obstacle_args(self):
            return None, 0, self.n_blocked.data_ptr() if counted else None

    def run(cls):
        ep = cls(engine, n, n_steps, integrator="rect+cum", start=R.START, target=R.TARGET,
                 incumbent0=INC_MAX, L=0.5, chain=form.startswith("chained"), max_steps=3,
                 log_capacity=8)
        if counted:
            ep.n_blocked.fill_(77)       # (the obstacle entries zero it on the stream)
        res = [_resident(v, b, form == "chained tiled") for v, b in batches]
        for i in range(6):
            ep.step(controls=res[i % 3])
        log = ep.read_log()
        torch.cuda.synchronize()
        assert ep.chain_error() == 0
        assert len(log) == 6 and max(r.episode for r in log) >= 2, "no restart"
        return ([bytes(r) for r in log], ep.log.cpu().numpy().tobytes(),
                ep.state.cpu().numpy().tobytes(), int(ep.n_blocked.item()))

    plain, entries = run(DeviceEpisode), run(ObstacleEntries)
    assert entries[:3] == plain[:3]
    assert plain[3] == (77 if counted else 0) and entries[3] == 0


# ----------------------------------------------------------------------------
# 6. everything blocked
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("two-launch", "chained"))
def test_everything_blocked(engine, form):
    from diplomjourney_amd.abi import MPC_EP_STALE
    n_steps = 3
    va, ba = R.chain_batch_a(n_steps)
    n = va.shape[1]
    assert np.isfinite(va).all() and np.isfinite(ba).all()
    ep = _episode(engine, n, n_steps, "rect+cum", 0.5, chain=form == "chained",
                  obstacles=[(R.START[0], R.START[1], 10.0)])
    ep.step(controls=_resident(va, ba, False))
    rec, = ep.read_log()
    assert (rec.found, rec.index) == (0, -1) and rec.status & MPC_EP_STALE
    assert (rec.x, rec.y, rec.phi) == R.START[:3]
    assert int(ep.n_blocked.item()) == n
    from diplomjourney_amd.abi import result_from_bytes
    res = result_from_bytes(ep.local.cpu().numpy().tobytes())
    assert (res.found, res.index) == (0, -1)


# ----------------------------------------------------------------------------
# 7. closed loop against the host episode
# ----------------------------------------------------------------------------
def _inside(x, y, c):
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 < c[2] * c[2]


@pytest.mark.parametrize("mode", ("rect", "rect+rot", "rect+cum"))
def test_closed_loop_avoids_the_circle(engine, mode):
    """Episode(obstacles=c) against DeviceEpisode(obstacles=c), 120 steps: the
    circle sits on the unobstructed run's pose at step 25.  rect and rect+rot
    are world frame (the host's and the device's tables are the same numbers):
    every step's index, p, found and status identical.  rect+cum (the device's
    own frame table): the run leaves its unobstructed path and no found step
    ends inside the circle."""
    import math
    from diplomjourney_amd.episode import DeviceEpisode, Episode
    n, ns, steps = 20_000, 10, 120
    free = DeviceEpisode(engine, n, ns, integrator=mode, log_capacity=512)
    for _ in range(steps):
        free.step()
    path = free.read_log()
    c = (path[25].x, path[25].y, 0.15)
    assert any(_inside(r.x, r.y, c) for r in path)
    dev = DeviceEpisode(engine, n, ns, integrator=mode, log_capacity=512, obstacles=[c])
    for _ in range(steps):
        dev.step()
    got = dev.read_log()
    assert len(got) == steps
    assert not any(_inside(r.x, r.y, c) for r in got if r.found)
    if mode == "rect+cum":
        return
    host = Episode(engine, n, ns, integrator=mode, obstacles=[c])
    want = []
    for _ in range(steps):
        host.step()
        want.append(host.last_log)
    for g, w in zip(got, want):
        assert (g.index, g.p, g.found, g.status) == (w[0], w[2], w[8], w[9])
        assert math.isclose(g.cost, w[1], rel_tol=COST_RTOL)
        assert max(abs(a - b) for a, b in zip((g.x, g.y, g.phi, g.v, g.beta), w[3:8])) <= STATE_TOL


# ----------------------------------------------------------------------------
# 8. refused combinations
# ----------------------------------------------------------------------------
def test_refused_combinations(engine):
    from diplomjourney_amd.episode import DeviceEpisode
    one = [(1.0, 1.0, 0.2)]
    for kw in (dict(generate=True), dict(split=False), dict(chain=True, exchange=True),
               dict(chain=True, exchange=True, p2p=True),
               dict(chain=True, exchange=True, overlap=True)):
        with pytest.raises(ValueError, match="two-launch step"):
            DeviceEpisode(engine, 1024, 3, integrator="rect+cum", obstacles=one, **kw)
        ep = DeviceEpisode(engine, 1024, 3, integrator="rect+cum", **kw)
        try:
            with pytest.raises(ValueError, match="chained step"):
                ep.set_obstacles(one)
            ep.set_obstacles(())            # none: every form takes that
        finally:
            ep.close()
    ep = DeviceEpisode(engine, 1024, 3, integrator="rect+cum", chain=True, obstacles=one)
    v, b = R.grid_batch(1024, 3, 5)
    with pytest.raises(ValueError, match="run"):
        ep.run([(_dev(v), _dev(b))])
    with pytest.raises(ValueError, match="at most 16"):
        ep.set_obstacles(one * 17)
    # the supported forms take them: split two-launch, also as the multi-GPU step on one rank
    for kw in (dict(), dict(chain=True)):
        DeviceEpisode(engine, 1024, 3, integrator="rect+cum", obstacles=one, **kw).step()
    # (its rollout and selection; advance() is the unchanged exchange over a process group)
    ep = DeviceEpisode(engine, 1024, 3, integrator="rect+cum", obstacles=[(0.0, 0.0, 10.0)],
                       exchange=True)
    ep.expand()
    torch.cuda.synchronize()
    assert int(ep.n_blocked.item()) == 1024
