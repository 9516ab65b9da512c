"""The batched robots' episode kernel (k_episodes_run, csrc/mpc_episodes.h,
through DeviceEpisodes) pinned to the host replica and the host model, bit for
bit: `==` on the raw bits of every field, no tolerance anywhere.

The kernel restates the rollout kernels' arithmetic (two candidates per lane,
an unrolled and a generic horizon, lane-parallel winner states, a hand-made
clamp of short horizons, its own scan and arg-min) and promises their bits.
The expected values come from tests/robots_model.py: the host build of
rollout_candidate for every candidate of every step of every robot, the
lowest (cost, index), and tests/episode_model.py's update in its no-restart
form.  Only the reciprocal estimates of the steering tangent come from the
device (one fetch per step, no miss allowed).

Compared per case (tests/robots_cases.py): the whole state tensor — every
field of every RobotState (h, st, stop, calls, candidates) and the
configurations copied behind them — the whole log ring of every robot (every
record of every step still in it, the cost as bits, and zero in every slot no
step wrote) and the progress records.  h.nv and h.nb, which k_episodes_run
never writes (its grid lives in LDS), are compared like every other field:
they must hold what k_episodes_reset left, 0.  The comparison and its report
are robots_model.compare (checked on the CPU with planted differences)."""
import pytest

import robots_bench as RB
import robots_cases as RC
import robots_model as RM
from diplomjourney_amd.abi import (LOG_BYTES, MPC_EP_ARRIVED, MPC_EP_BREAK, MPC_EP_EVENT,
                                   MPC_EP_LIMIT, MPC_EP_STALE, MPC_EP_STUCK, MpcEpisodeLog)

pytestmark = pytest.mark.gpu


def check(engine, case):
    """-> the models, their records and the device's (state, log, progress)
    bytes with read_logs() behind them."""
    models, recs, first = RC.model_run(case, device=True)
    if case.get("every_candidate") and sum(case["launches"]):   # before any kernel is looked at
        assert RC.excluded(case, first) == []
    got, _, eps = RB.episodes_run(engine, case)
    RB.assert_model(case, got, models, recs)
    return models, recs, (*got, eps.read_logs())


@pytest.mark.parametrize("n_steps,L", RC.SHAPES_A)
@pytest.mark.parametrize("integ", RC.MODES)
def test_every_candidate_wins_once(engine, integ, n_steps, L):
    """Case A: 549 robots, robot c placed so that candidate c of its first step
    is the strict minimum: every lane, both passes and both pair slots are the
    winner once and every candidate's cost is compared once; five more steps
    follow from 549 different states (finishing logic, arrival, step limit)."""
    models, recs, _ = check(engine, RC.case_a(integ, n_steps, L))
    assert [rr[0]["index"] for rr in recs] == list(range(549))
    assert (MPC_EP_ARRIVED if n_steps == 1 else MPC_EP_LIMIT) in {M.stop for M in models}


@pytest.mark.parametrize("n_steps,L", RC.SHAPES_B)
@pytest.mark.parametrize("integ", RC.MODES)
def test_flagged_candidates(engine, integ, n_steps, L):
    """Case B: |beta| > kTanMax on the grid, and a start heading above
    kFastMax; flagged candidates win steps in both sets (the safe recurrence of
    the costs and of the winner's states, wave_winner_states_l's fallback)."""
    case = RC.case_b(integ, n_steps, L)
    models, recs, _ = check(engine, case)
    assert all(len(f) >= 1 for f in RC.flagged_winners(case, recs))


@pytest.mark.parametrize("integ", RC.MODES)
def test_ties_report_the_first_index(engine, integ):
    """Case C: exact ties over a whole beta row (standing candidates) and over
    the nine speeds of a slow-down step, between lanes (9 x 61) and inside a
    lane (9 x 64): the lowest index is logged."""
    models, recs, _ = check(engine, RC.case_c(integ))
    assert max(max(M.ties) for M in models[:8]) >= 61
    assert all(max(M.ties) >= 9 for M in models[8:])
    assert all(M.sizes[1] == (9, 64) and M.ties[1] == 9 for M in models[16:])


@pytest.mark.parametrize("n_steps", (1, 2, 3, 4))
@pytest.mark.parametrize("integ", RC.MODES)
def test_degenerate_grids(engine, integ, n_steps):
    """Case D: grids of 1, 15, 4096 (clamped) and 0 candidates, targets at +inf
    and NaN with either first incumbent, a robot that starts on its target."""
    models, recs, _ = check(engine, RC.case_d(integ, n_steps))
    none = MPC_EP_STALE | MPC_EP_STUCK
    for r in (3, 4, 5, 7, 8):
        assert [q["status"] for q in recs[r]] == [none, none | MPC_EP_BREAK]
        assert [q["index"] for q in recs[r]] == [-1, -1]
    assert (models[6].calls, models[6].stop, recs[6]) == (0, MPC_EP_ARRIVED, [])
    assert [M.candidates for M in models[:2]] == [6, 90] and models[3].candidates == 0


@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_operator_schedule(engine, integ):
    """Case E: the turn right, the turn left and the new target on steps 2, 3
    and 4 of the reference's configuration, ten steps."""
    models, recs, _ = check(engine, RC.case_e(integ))
    assert [q["p"] for q in recs[0] if q["status"] & MPC_EP_EVENT] == [2, 3, 4]
    assert models[0].calls == 10


def test_launch_splits_carry_the_state(engine):
    """Case F: six steps as run(6), as three run(2) and as six run(1): state,
    log and progress identical, `candidates` summed across the launches."""
    runs = []
    for launches in ((6,), (2, 2, 2), (1,) * 6):
        models, recs, got = check(engine, RC.case_f(launches))
        runs.append(got[:3])
    assert runs[0] == runs[1] == runs[2]
    assert sum(M.candidates for M in models) > 549 * 549


def test_log_ring_wraps(engine):
    """Case F with a ring of two: after six calls slot 0 holds step 4 and slot
    1 step 5, and read_logs() returns the two in order."""
    case = RC.case_f((6,), cap=2)
    models, recs, got = check(engine, case)
    six = [r for r, M in enumerate(models) if M.calls == 6]
    assert len(six) > 50
    for r in six:
        ring = got[1][r * 2 * LOG_BYTES:(r + 1) * 2 * LOG_BYTES]
        assert [MpcEpisodeLog.from_buffer_copy(ring[s * LOG_BYTES:(s + 1) * LOG_BYTES]).step
                for s in (0, 1)] == [4, 5]
    for r, M in enumerate(models):
        want = recs[r][-2:]
        assert [int(q) for q in got[3][r]["step"]] == [q["step"] for q in want], r
        assert [q.tobytes() for q in got[3][r]] == [
            bytes(RM.EM.log_struct(q)) for q in want], r


def test_no_call_leaves_the_reset_state(engine):
    """max_calls = 0: the state is k_episodes_reset's, nothing is logged."""
    models, recs, got = check(engine, RC.case_f((0,)))
    assert all(M.calls == 0 for M in models) and got[1] == bytes(len(got[1]))
