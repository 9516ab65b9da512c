"""The host model of the batched robots (tests/robots_model.py) and the case
table of its GPU test (tests/robots_cases.py) checked on the CPU: the
RobotState mirror against the compiler and the library, the preconditions a
case must meet before tests/test_robots_replica_gpu.py means anything (host
1.0 / q in place of the device's reciprocal estimates), the model's driver
against the reference's recorded run, and EpisodeModel.advance(restart=False)
against the restarting form."""
import copy
import ctypes
import math

import numpy as np
import pytest

import episode_model as EM
import episode_state as ES
import robots_cases as RC
import robots_model as RM
from diplomjourney_amd.abi import (MPC_EP_ARRIVED, MPC_EP_BREAK, MPC_EP_EVENT, MPC_EP_STALE,
                                   MPC_EP_STUCK, MpcEpisodeConfig, MpcEpisodeLog,
                                   MpcEpisodesProgress)
from diplomjourney_amd.episode_config import reference_episode_config


def test_robot_state_mirror_matches_the_compiler_and_the_library():
    """sizeof(RobotState) and its offsets against the host build of
    csrc/mpc_episodes.h, and mpc_episodes_state_bytes(n) ==
    align256(n * sizeof(RobotState)) + n * sizeof(mpc_episode_config_t)."""
    from diplomjourney_amd import native
    assert ES.check_robot_layout() == 8
    size, cfg = ctypes.sizeof(ES.RobotState), ctypes.sizeof(MpcEpisodeConfig)
    assert size == 8 * ES.STORED_WORDS + 16
    lib = native.lib()
    for n in range(1, 65):
        want = ((n * size + 255) // 256) * 256 + n * cfg
        assert lib.mpc_episodes_state_bytes(n) == want == ES.robots_state_bytes(n), n


def test_where_names_the_scan_position():
    assert RM.where(0) == "candidate 0: pass 0, wave 0, lane 0, pair slot 0"
    assert RM.where(256 + 64) == "candidate 320: pass 0, wave 1, lane 0, pair slot 1"
    assert RM.where(548) == "candidate 548: pass 1, wave 0, lane 36, pair slot 0"
    assert RM.where(-1) == "no candidate"


@pytest.mark.parametrize("n_steps,L", RC.SHAPES_A)
@pytest.mark.parametrize("integ", RC.MODES)
def test_case_a_excludes_no_robot(integ, n_steps, L):
    """Candidate c is the strict (cost, index) minimum of robot c's first
    step, for all 549 robots, and no robot has arrived before it."""
    case = RC.case_a(integ, n_steps, L)
    models, recs, first = RM.run(case["cfgs"], n_steps, integ, 1, device=False)
    assert all(M.calls == 1 for M in models)
    assert RC.excluded(case, first) == []
    assert [rr[0]["index"] for rr in recs] == list(range(549))
    assert sum(c.max_steps == 3 for c in case["cfgs"]) == 78


@pytest.mark.parametrize("n_steps,L", RC.SHAPES_B)
@pytest.mark.parametrize("integ", RC.MODES)
def test_case_b_flagged_candidates_win(integ, n_steps, L):
    """Every first-step cost is finite; in each set a candidate with |beta| >
    kTanMax wins a step; in the second set every heading of a direct-form
    rollout is above kFastMax."""
    case = RC.case_b(integ, n_steps, L)
    models, recs, first = RC.model_run(case, device=False)
    assert all(np.isfinite(costs).all() and len(costs) == 21 for costs, _ in first)
    assert all(len(f) >= 1 for f in RC.flagged_winners(case, recs))
    assert [rr[0]["index"] for rr in recs] == list(range(21)) * 2
    _, _, states, _ = RC.first_step(case["cfgs"][21], n_steps, integ)
    assert (np.abs(states[:, 2, :]) > RC.K_FAST_MAX).all()
    _, B, states, _ = RC.first_step(case["cfgs"][0], n_steps, integ)
    assert max(B) > RC.K_TAN_MAX and (np.abs(states[:, 2, :]) < RC.K_FAST_MAX).all()


@pytest.mark.parametrize("integ", RC.MODES)
def test_case_c_ties(integ):
    """Standing candidates tie over a whole beta row and win with index 0;
    after the event every step's winner ties with its eight siblings of the
    other speeds and has the lowest index of them (a = 0); with 64 betas
    three of the nine run in the winner's own lane."""
    case = RC.case_c(integ)
    models, recs, _ = RC.model_run(case, device=False)
    standing = [(r, s) for r in range(8) for s, rec in enumerate(recs[r])
                if rec["found"] and rec["v"] == 0.0]
    assert len(standing) >= 4
    # (a whole row of the step's B: 61 betas, fewer where the bound cuts the grid)
    assert all(models[r].ties[s] >= 30 and recs[r][s]["index"] == 0 for r, s in standing)
    assert sum(models[r].ties[s] == 61 for r, s in standing) >= 2
    assert any(recs[r][-1]["status"] == MPC_EP_STUCK | MPC_EP_BREAK for r in range(8))
    for r in range(8, 24):
        assert recs[r][0]["status"] == MPC_EP_EVENT and models[r].ties[0] == 1
        assert all(t % 9 == 0 and t >= 9 for t in models[r].ties[1:4]), models[r].ties
        assert all(rec["index"] < models[r].sizes[s][1] for s, rec in enumerate(recs[r][:4]) if s)
    # set 3: 9 x 64 on the second step, so the winner's lane holds three of the tied
    assert all(models[r].sizes[1] == (9, 64) and models[r].ties[1] == 9 for r in range(16, 24))


@pytest.mark.parametrize("integ", ("qk21", "rect+cum"))
def test_case_d_and_e_reach_their_branches(integ):
    """Case D's grids have 1, 15, 4096 (both grids clamped to 64) and 0
    candidates; the robots without a grid or without a finite cost are stale
    and stuck, then break; the last has arrived before a step.  Case E fires
    its three events."""
    none = MPC_EP_STALE | MPC_EP_STUCK
    for n_steps in (1, 3):
        case = RC.case_d(integ, n_steps)
        models, recs, _ = RC.model_run(case, device=False)
        assert [M.sizes[0][0] * M.sizes[0][1] if M.sizes else None
                for M in models] == list(case["n_grid"])
        assert models[2].sizes[0] == (64, 64)
        for r in (3, 4, 5, 7, 8):
            assert [q["status"] for q in recs[r]] == [none, none | MPC_EP_BREAK]
            assert [(q["index"], q["found"], q["cost"]) for q in recs[r]] == [
                (-1, 0, math.inf)] * 2
        assert (models[6].calls, models[6].stop, recs[6]) == (0, MPC_EP_ARRIVED, [])
    models, recs, _ = RC.model_run(RC.case_e(integ), device=False)
    assert [q["p"] for q in recs[0] if q["status"] & MPC_EP_EVENT] == [2, 3, 4]


def test_robot_model_replays_the_reference_run(scenario):
    """RobotModel with the reference's configuration, qk21, horizon 3, over
    the host replica: the 151 recorded calls — chosen (v, beta) equal, pose
    within 1e-6, events at p = 60, 90, 110, arrival on the last call."""
    calls = [c for c in scenario["calls"] if not c["isActual"]]
    cfg = reference_episode_config(enumerate=True, incumbent0=10000050990.195135)
    models, recs, _ = RM.run([cfg], 3, "qk21", 400, device=False)
    M, recs = models[0], recs[0]
    assert M.calls == len(recs) == len(calls) == 151
    worst = 0.0
    for i, (rec, g) in enumerate(zip(calls, recs)):
        assert (g["step"], g["p"], g["episode"], g["found"]) == (i, i + 1, 1, int(rec["found"])), i
        assert [g["v"], g["beta"]] == rec["ret"][3:5], i
        worst = max(worst, max(abs(g[k] - w) for k, w in zip(("x", "y", "phi"), rec["ret"][:3])))
    assert worst <= 1e-6, worst
    assert [g["p"] for g in recs if g["status"] & MPC_EP_EVENT] == [60, 90, 110]
    assert [i for i, g in enumerate(recs) if g["status"] & MPC_EP_ARRIVED] == [150]
    assert M.stop == recs[-1]["status"] and M.stop & MPC_EP_ARRIVED
    assert M.candidates == sum(len(c["V"]) * len(c["B"]) for c in calls)


class _Counting(EM.EpisodeModel):
    """EpisodeModel that counts its prepare() and restart() calls."""
    prepares = restarts = 0

    def prepare(self):
        self.prepares += 1
        super().prepare()

    def restart(self):
        self.restarts += 1
        super().restart()


def _fields(M):
    skip = ("trace", "c", "sincos", "prepares", "restarts")
    return {k: copy.deepcopy(v) for k, v in vars(M).items() if k not in skip}


def test_advance_without_restart_against_the_restarting_form():
    """advance(restart=False) and advance() over the same winners: the same
    record always; the same state when the step does not end.  When it ends,
    the restarting form restarts and prepares, the other does neither: it
    keeps the state the record describes — episodes, t, K and seed are the
    ended step's, the pose is the logged one — which is also RobotModel's."""
    ended = not_ended = 0
    for case in (RC.case_c("rect"), RC.case_d("rect", 3), RC.case_a("rect", 3, 0.5)):
        for cfg in case["cfgs"][:40]:
            if math.isnan(cfg.target_x):             # (NaN fields never compare equal)
                continue
            A, B, R = _Counting(cfg), _Counting(cfg), RM.RobotModel(cfg, 3, "rect")
            while not R.stop and R.calls < 6:
                before = _fields(B)
                counts = (A.prepares, A.restarts, B.prepares, B.restarts)
                R.mpc_step()
                row = R.last[1]
                ra, rb = A.advance([row]), B.advance([row], restart=False)
                assert ra == rb
                after = (A.prepares, A.restarts, B.prepares, B.restarts)
                if not rb["status"] & RM.EP_ENDED:
                    not_ended += 1
                    assert after == (counts[0] + 1, counts[1], counts[2] + 1, counts[3])
                    assert _fields(A) == _fields(B)
                    continue
                ended += 1
                assert after == (counts[0] + 1, counts[1] + 1, counts[2], counts[3])
                fb = _fields(B)
                assert (fb["episodes"], fb["t"], fb["K"], fb["seed"]) == (
                    before["episodes"], before["t"], before["K"], before["seed"])
                assert (fb["x"], fb["y"], fb["phi"], fb["v"], fb["beta"]) == tuple(
                    rb[k] for k in ("x", "y", "phi", "v", "beta"))
                assert fb["step"] == before["step"] + 1 and fb["incumbent"] == EM.INC_MAX
                assert A.episodes == before["episodes"] + 1 and A.p == 1       # the restart
                fr = _fields(R)                      # the robot's model made the same update
                assert all(fr[k] == v for k, v in fb.items())
                assert R.stop == rb["status"]
    assert ended >= 20 and not_ended >= 100, (ended, not_ended)


def test_compare_names_robot_step_field_and_lane():
    """robots_model.compare on planted differences: a batch's bytes as the
    models predict them compare clean; one winner layer state, one K field,
    one logged cost and index, one progress count changed in them are each
    reported with the robot (= the candidate, its pass, wave, lane and pair
    slot), the step, the element's own name and both values."""
    case = RC.case_a("rect", 3, 0.5)
    models, recs, _ = RC.model_run(case, device=False)
    state, log, progress = RM.expected(case, models, recs)
    assert RM.compare(case, state, log, progress, models, recs) == []
    size, LOG = ctypes.sizeof(ES.RobotState), ctypes.sizeof(MpcEpisodeLog)
    for r, k, q in ((0, 0, 1), (300, 1, 1), (548, 2, 2)):
        R = ES.RobotState.from_buffer_copy(state[r * size:(r + 1) * size])
        was = R.st.ot[k][q]
        R.st.ot[k][q] = math.nextafter(was, math.inf)
        R.h.K.inv_den = -R.h.K.inv_den
        got = state[:r * size] + bytes(R) + state[(r + 1) * size:]
        (line,) = RM.compare(case, got, log, progress, models, recs)
        assert line.startswith(f"robot {r} ({RM.where(r)}) state after step {models[r].step - 1} ")
        assert f"('st.ot[{k}][{q}]', '{R.st.ot[k][q].hex()}', '{was.hex()}')" in line
        assert f"('h.K.inv_den', '{R.h.K.inv_den.hex()}', '{(-R.h.K.inv_den).hex()}')" in line
        assert line.count("('") == 2
    r, s = 300, 1                                    # robot 300's second step, ring slot 1
    at = (r * case["cap"] + s) * LOG
    rec = MpcEpisodeLog.from_buffer_copy(log[at:at + LOG])
    want_cost, want_index = rec.cost, rec.index
    rec.cost, rec.index = math.nextafter(rec.cost, 0.0), 44
    (line,) = RM.compare(case, state, log[:at] + bytes(rec) + log[at + LOG:], progress, models,
                         recs)
    assert line.startswith(f"robot 300 ({RM.where(300)}) log slot 1 (device step 1, model step 1, "
                           f"device chose {RM.where(44)})")
    assert f"('index', 44, {want_index})" in line
    assert f"('cost', '{rec.cost.hex()}', '{want_cost.hex()}')" in line
    P = MpcEpisodesProgress.from_buffer_copy(progress[16 * 7:16 * 8])
    P.candidates -= 549
    (line,) = RM.compare(case, state, log, progress[:16 * 7] + bytes(P) + progress[16 * 8:],
                         models, recs)
    assert line == (f"robot 7 ({RM.where(7)}) progress (field, device, model): "
                    f"[('candidates', {P.candidates}, {P.candidates + 549})]")
    # two NaNs that differ in their bits are told apart
    a, b = ES.StaleTraj(), ES.StaleTraj()
    a.ot[2][0], b.ot[2][0] = math.nan, -math.nan
    assert ES.named_diff(a, b) == [("ot[2][0]", "nan 0x7ff8000000000000",
                                    "nan 0xfff8000000000000")]
