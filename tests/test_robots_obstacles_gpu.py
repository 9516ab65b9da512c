"""Keep-out circles in the batched robots' device-resident episodes
(mpc_episodes_run_obstacles, k_episodes_run with an obstacle hook in
csrc/mpc_episodes.h, through DeviceEpisodes) pinned to the host model, bit for bit.

Every comparison is robots_model.compare on the whole state tensor, every log
ring and the progress records — `==` on the bits — plus read_blocked() ==
the model's counts after every launch.  The expected values come from
tests/robots_obstacle_model.py: the replica's states of every candidate of
every step of every robot, ranking.blocked of them (the header's formula in
world coordinates), blocked costs at +inf, and the unchanged winner and
update.  Every case first asserts its preconditions on that model — the margin
between any state and any rim above ranking.MARGIN among them, so that the
mask depends neither on last bits nor on the rect+cum frame rotation — before
any kernel is looked at (tests/test_robots_obstacles_cpu.py checks the same
with the IEEE replica)."""
import numpy as np
import pytest

import robots_bench as RB
import robots_cases as RC
import robots_model as RM
import robots_obstacle_cases as OC
import robots_obstacle_model as OM
from diplomjourney_amd.abi import MPC_EP_BREAK, MPC_EP_STALE, MPC_EP_STUCK
from diplomjourney_amd.device_episodes import DeviceEpisodes

pytestmark = pytest.mark.gpu


def check(engine, case, count, precondition=None):
    """The model run (shared by the counts of one case), its preconditions,
    then the device against it -> the models, their records and the device's
    (state, log, progress) bytes with read_blocked() after every launch."""
    models, recs, first = OC.model_run(case, device=True)
    assert min(M.margin for M in models) > OC.MARGIN, min(M.margin for M in models)
    if precondition:
        precondition(models, recs, first)
    got, blocked, _ = RB.episodes_run(engine, case, OC.table(case, count))
    name = f"{case['name']} x{count}"
    RB.assert_model(dict(case, name=name), got, models, recs)
    RB.assert_counts(name, blocked, OM.launch_counts(models, case["launches"]))
    return models, recs, (*got, blocked)


# ----------------------------------------------------------------------------
# 1. every unblocked candidate wins once
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ,n_steps,L,count", OC.MATRIX_A)
def test_every_unblocked_candidate_wins_once(engine, integ, n_steps, L, count):
    """robots_cases' case A under circles: 549 robots, robot c's target on
    candidate c's final state, six steps.  The blocked robots' first winner is
    an unblocked candidate, every other robot's its own: every lane, both
    passes and both pair slots win and lose once, by a final state and by an
    earlier one alone."""
    case = OC.case_a(integ, n_steps, L, count == 1)
    models, recs, _ = check(engine, case, count,
                            lambda models, recs, first: OC.check_case_a(case, models, first))
    mask = models[0].masks[0][0]
    assert [rr[0]["index"] for c, rr in enumerate(recs) if not mask[c]] == list(
        np.flatnonzero(~mask))


# ----------------------------------------------------------------------------
# 2. flagged candidates
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", (3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_flagged_candidates_are_tested_by_their_safe_states(engine, integ, n_steps):
    """Case B's two sets under a circle on a flagged candidate's final state
    and one on a first-layer state: the recompute resets the flag and tests
    every step_safe state against the world table."""
    case = OC.case_b(integ, n_steps)
    check(engine, case, 4, lambda models, recs, first: OC.check_case_b(case, models, recs))


# ----------------------------------------------------------------------------
# 3. the frame moves with the robot
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("count", (4, 16))
@pytest.mark.parametrize("integ,L", (("rect+cum", 0.5), ("rect+cum", 0.45), ("qk21", 0.5)))
def test_the_frame_moves_with_the_robot(engine, integ, L, count):
    """Eight robots drive around one circle for 40 steps over launches of 5, 7
    and 28: rect+cum's frame table is formed per step of each robot (one
    formed per launch is wrong from the launch's second step on)."""
    case = OC.case_c(integ, L)
    check(engine, case, count, lambda models, recs, first: OC.check_case_c(case, models, recs))


# ----------------------------------------------------------------------------
# 4. edges
# ----------------------------------------------------------------------------
EDGE_MODES = ("qk21", "rect+cum")


@pytest.mark.parametrize("integ", EDGE_MODES)
def test_every_candidate_blocked(engine, integ):
    """r = 10 around the start: found 0, index -1, stale steps until the stuck
    rule ends the episode, n_blocked equal to candidates."""
    models, recs, got = check(engine, OC.case_all_blocked(integ), 1)
    none = MPC_EP_STALE | MPC_EP_STUCK
    assert [q["status"] for q in recs[0]] == [none, none | MPC_EP_BREAK]
    assert [(q["index"], q["found"]) for q in recs[0]] == [(-1, 0), (-1, 0)]
    assert int(got[3][0][0]) == models[0].candidates == 2 * 549


@pytest.mark.parametrize("integ", EDGE_MODES)
def test_start_inside_a_circle(engine, integ):
    """The start pose is not tested: the candidates that leave the circle with
    their first step are free, and one of them wins."""
    models, recs, _ = check(engine, OC.case_start_inside(integ), 4)
    assert 0 < models[0].blocked_steps[0] < 549 and recs[0][0]["found"] == 1


@pytest.mark.parametrize("integ", EDGE_MODES)
def test_clamped_grid_of_4096(engine, integ):
    """64 x 64 candidates: eight passes of both pair slots, 16 circles."""
    models, recs, _ = check(engine, OC.case_clamped(integ), 16)
    assert models[0].sizes[0] == (64, 64) and 0 < models[0].blocked_steps[0] < 4096
    assert models[0].margin > OC.MARGIN


@pytest.mark.parametrize("integ", EDGE_MODES)
def test_grid_of_one_candidate(engine, integ):
    """One candidate (one lane, no partner): free for two steps, then blocked."""
    models, recs, _ = check(engine, OC.case_single(integ), 1)
    assert models[0].blocked_steps == [0, 0, 1, 1] and models[0].margin > OC.MARGIN


@pytest.mark.parametrize("integ", EDGE_MODES)
def test_operator_schedule_with_a_circle(engine, integ):
    """Case E's turn right, turn left and new target with a circle on the path."""
    models, recs, _ = check(engine, OC.case_schedule(integ), 4)
    assert sum(models[0].blocked_steps) > 0 and models[0].margin > OC.MARGIN


# ----------------------------------------------------------------------------
# 5. zero circles through the obstacle entry
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("integ", EDGE_MODES)
def test_obstacle_entry_without_circles(engine, integ):
    """mpc_episodes_run_obstacles with n_obstacles = 0 launches the plain
    kernels: the bytes of the plain entry and of the model, a zero count."""
    class ObstacleEntry(DeviceEpisodes):
        def _obstacle_args(self):
            return None, 0, self.n_blocked.data_ptr()

    case = dict(RC.case_b(integ, 3, 0.5), launches=(2, 4), name=f"zero circles {integ}")
    models, recs, _ = RC.model_run(case, device=True)
    plain, none, _ = RB.episodes_run(engine, case, ())
    entry, zeros, _ = RB.episodes_run(engine, case, (), ObstacleEntry)
    assert entry == plain
    assert not RM.compare(case, *entry, models, recs)
    assert all((b == 0).all() for b in zeros + none)


# ----------------------------------------------------------------------------
# 6. run_tree_batched equals run_tree_episode with barriers
# ----------------------------------------------------------------------------
def test_tree_batched_equals_sequential_with_barriers(engine, monkeypatch):
    """The six starts of test_tree_episode_loop_batched_equals_sequential, a
    barrier circle at the midpoint of each start-target segment: the batched
    driver (obstacles=None: math_model_tree.barriers at the call) returns what
    the sequential driver returns — the same stop, the same length, (v, beta)
    identical, pose within 1e-12 — and the barriers change an episode."""
    import ranking
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import run_math_model as rmm
    starts = rmm.draw_starts(6, seed=20261015)
    circles = [((s[0] + s[3]) / 2, (s[1] + s[4]) / 2, 0.1513) for s in starts]
    margins = []
    step = mmt.predictive_control

    def watched(*a, **k):
        out = step(*a, **k)
        if mmt.barriers:
            margins.append(ranking.blocked(mmt.last_tree.states.cpu().numpy(), mmt.barriers)[1])
        return out

    monkeypatch.setattr(mmt, "predictive_control", watched)
    try:
        free = [rmm.run_tree_episode(s, max_calls=120) for s in starts]
        mmt.reset_state()
        for c in circles:
            mmt.add_barrier_circle(*c)
        seq = [rmm.run_tree_episode(s, max_calls=120) for s in starts]
        stats = {}
        bat = rmm.run_tree_batched(starts, max_calls=120, integrator="qk21", engine=engine,
                                   stats=stats)
        none = rmm.run_tree_batched(starts, max_calls=120, integrator="qk21", engine=engine,
                                    obstacles=())
    finally:
        mmt.reset_state()
    assert len(margins) == sum(len(r) for r, _ in seq) and min(margins) > ranking.MARGIN
    assert any(a != b for a, b in zip(free, seq)), "the barriers change no sequential episode"
    assert stats["blocked"] > 0
    for (rs, ss), (rb, sb) in zip(seq, bat):
        assert ss == sb and len(rs) == len(rb)
        for a, b in zip(rs, rb):
            assert a[3:] == b[3:]
            assert max(abs(p - q) for p, q in zip(a[:3], b[:3])) <= 1e-12
    for (rs, ss), (rb, sb) in zip(free, none):     # () overrides the list
        assert ss == sb and [a[3:] for a in rs] == [b[3:] for b in rb]
