"""One robot of the batched device episodes (csrc/mpc_episodes.h) restated on
the host: k_episodes_reset and one iteration of k_episodes_run's loop, with
all of RobotState, so that a test can compare the kernel's state, log ring and
progress record with `==` on the bits.

RobotModel is an episode_model.EpisodeModel (the grids, the finishing logic,
the stuck rules, the events, arrival and the step limit, field for field) plus
what the kernel adds: the step's candidates k = a * |B| + b with constant
controls, their costs and states from the host build of rollout_candidate
(harness.replica_rollout with the device's consts_from_problem), the lowest
(cost, index) among the costs below +inf, the update in its no-restart form
(episode_advance<false>), and stop / calls / candidates.  Nothing is read from
a device except, in a GPU run, the reciprocal estimates of the steering
tangent's denominators (v_rcp_f64 is not an IEEE operation): run() fetches
them once per step for all robots and asserts that no rollout needed one it
did not have.  Test infrastructure only."""
import ctypes
import math

import numpy as np

import episode_model as EM
import episode_state as ES
import harness
from diplomjourney_amd.abi import (LOG_BYTES, MPC_EP_ARRIVED, MPC_EP_BREAK, MPC_EP_LIMIT,
                                   PROGRESS_BYTES, MpcEpisodeLog, MpcEpisodesProgress)

EP_ENDED = MPC_EP_ARRIVED | MPC_EP_BREAK | MPC_EP_LIMIT      # kEpEnded
K_BLOCK = 256                                                # kBlock


def enumerate_controls(V, B, n_steps):
    """The step's candidates k = a * |B| + b, constant over the horizon: SoA
    [n_steps, |V| * |B|]."""
    vv = np.repeat(np.array(V, dtype=np.float64), len(B))
    bb = np.tile(np.array(B, dtype=np.float64), len(V))
    return np.tile(vv, (n_steps, 1)), np.tile(bb, (n_steps, 1))


def winner(states, costs, v, b):
    """The Result of the lowest (cost, index) among the costs below +inf (the
    kernel's keys: NaN and +inf never win); none: index -1, cost +inf."""
    n_steps = v.shape[0]
    ok = np.flatnonzero(costs < math.inf)
    if not len(ok):
        return EM.Result(math.inf, -1, n_steps, 0.0, 0.0, [[0.0] * 3] * min(n_steps, 3))
    i = int(ok[np.argmin(costs[ok])])         # argmin: the first of equal minima
    return EM.Result(float(costs[i]), i, n_steps, float(v[0, i]), float(b[0, i]),
                     [[float(states[s, q, i]) for q in range(3)] for s in range(min(n_steps, 3))])


def where(c):
    """Where candidate c runs in k_episodes_run: lane l scans l, l + 256, ...
    two per pass."""
    c = int(c)
    if c < 0:
        return "no candidate"
    t = c % K_BLOCK
    return (f"candidate {c}: pass {c // (2 * K_BLOCK)}, wave {t // 64}, lane {t % 64}, "
            f"pair slot {(c // K_BLOCK) % 2}")


class RobotModel(EM.EpisodeModel):
    """After the constructor: k_episodes_reset's RobotState.  mpc_step(): one
    iteration of k_episodes_run's loop (None once the robot has stopped)."""

    def __init__(self, cfg, n_steps, integ, sincos=EM.device_sincos):
        super().__init__(cfg, sincos)
        self.n_steps, self.integ = int(n_steps), integ
        ex, ey = self.xt - self.x, self.yt - self.y
        self.stop = MPC_EP_ARRIVED if ex * ex + ey * ey <= cfg.eps else 0
        self.calls = 0
        self.candidates = 0
        self.last = None          # the last step's (costs, Result)
        self.ties = []            # per step: how many candidates have the winner's cost
        self.sizes = []           # per step: (|V|, |B|)

    def mpc_step(self):
        if self.stop:
            return None
        V, B, _ = self.grids()
        n_grid = len(V) * len(B)
        self.sizes.append((len(V), len(B)))
        prob, _ = self.begin_step()
        v, b = enumerate_controls(V, B, self.n_steps)
        if n_grid:
            states, costs = harness.replica_rollout(prob, v, b, self.integ, device_consts=True)
        else:
            states, costs = np.empty((self.n_steps, 3, 0)), np.empty(0)
        costs = self.score(states, costs, v, b)
        row = winner(states, costs, v, b)
        self.last = (costs, row)
        self.ties.append(int((costs == row.cost).sum()) if row.index >= 0 else 0)
        rec = self.advance([row], restart=False)
        if rec["status"] & EP_ENDED:
            self.stop = rec["status"]
        self.calls += 1
        self.candidates += n_grid
        return rec

    def score(self, states, costs, v, b):
        """The costs the winner is chosen from, given the rollout's (a subclass
        overrides this: robots_obstacle_model blocks candidates here)."""
        return costs

    def to_robot(self):
        """RobotState.  h.nv and h.nb: k_episodes_run keeps its grid in LDS and
        writes neither, so they are what k_episodes_reset left (0)."""
        S = self.to_state()
        R = ES.RobotState()
        ctypes.memmove(ctypes.addressof(R.h), ctypes.addressof(S.h), ctypes.sizeof(ES.EpisodeHead))
        ctypes.memmove(ctypes.addressof(R.st), ctypes.addressof(S.st), ctypes.sizeof(ES.StaleTraj))
        R.stop, R.calls, R.candidates = self.stop, self.calls, self.candidates
        return R

    def progress(self):
        return MpcEpisodesProgress(calls=self.calls, stop=self.stop, candidates=self.candidates)


def run(cfgs, n_steps, integ, max_calls, device=False, model=RobotModel):
    """Every robot's model — model(cfg, n_steps, integ): RobotModel or a factory
    of a subclass — run for up to max_calls steps, in lockstep (robots do not
    interact: the order is free).  Per step ONE table of reciprocal estimates
    for the union of the running robots' B grids (device=True: the GPU's;
    False: the host's 1.0 / q) and no miss.  Returns (models, records per
    robot, first-step (costs, Result) per robot)."""
    models = [model(c, n_steps, integ) for c in cfgs]
    recs = [[] for _ in models]
    first = [None] * len(models)
    for call in range(max_calls):
        live = [(r, M) for r, M in enumerate(models) if not M.stop]
        if not live:
            break
        betas = np.unique(np.concatenate([np.array(M.grids()[1], dtype=np.float64)
                                          for _, M in live]))
        with harness.estimates_installed(betas, device) as misses:
            for r, M in live:
                recs[r].append(M.mpc_step())
                if call == 0:
                    first[r] = M.last
            assert misses() == 0, f"step {call}: a denominator without its device estimate"
    return models, recs, first


def ring(recs, cap):
    """The robot's log ring after its steps: [cap] records' bytes, slot
    step % cap, untouched slots zero (as the batch allocates them)."""
    slots = [bytes(LOG_BYTES)] * cap
    for rec in recs:
        slots[rec["step"] % cap] = bytes(EM.log_struct(rec))
    return b"".join(slots)


def expected(case, models, recs):
    """(state, log, progress) bytes of a batch as the models predict them
    after the case's launches: RobotState[n], the configurations at
    episodes_cfg_offset(n); every robot's ring; the progress records (zero
    when no launch ran a step: mpc_episodes_run then launches nothing)."""
    n = len(models)
    state = bytearray(ES.robots_state_bytes(n))
    size = ctypes.sizeof(ES.RobotState)
    for r, M in enumerate(models):
        state[r * size:(r + 1) * size] = bytes(M.to_robot())
    cfgs = b"".join(bytes(c) for c in case["cfgs"])
    state[ES.robots_cfg_offset(n):ES.robots_cfg_offset(n) + len(cfgs)] = cfgs
    log = b"".join(ring(recs[r], case["cap"]) for r in range(n))
    launched = any(k > 0 for k in case["launches"])
    progress = b"".join(bytes(M.progress()) if launched else bytes(PROGRESS_BYTES)
                        for M in models)
    return bytes(state), log, progress


def compare(case, state, log, progress, models, recs):
    """Every difference between a batch's bytes (state tensor, log rings,
    progress records) and expected(): one line each, naming the robot — in an
    every-candidate case the robot IS its first step's candidate, so its pass,
    wave, lane and pair slot are named — the log slot and step, and every
    differing field with the device's and the model's value."""
    n, cap = len(models), case["cap"]
    every = bool(case.get("every_candidate"))
    tag = (lambda r: f"robot {r} ({where(r)})") if every else (lambda r: f"robot {r}")
    want_state, want_log, want_progress = expected(case, models, recs)
    bad = []
    robots, cfg_bytes = ES.read_robots(state, n)
    want_robots, want_cfgs = ES.read_robots(want_state, n)
    if cfg_bytes != want_cfgs:
        bad.append("the configurations behind the robots differ from those given")
    for r in range(n):
        d = ES.named_diff(robots[r], want_robots[r])
        if d:
            calls = want_robots[r].calls
            after = f"after step {calls - 1}" if calls else "after reset"
            bad.append(f"{tag(r)} state {after} (field, device, model): {d}")
        for s in range(cap):
            at = (r * cap + s) * LOG_BYTES
            a, b = log[at:at + LOG_BYTES], want_log[at:at + LOG_BYTES]
            if a != b:
                g, w = MpcEpisodeLog.from_buffer_copy(a), MpcEpisodeLog.from_buffer_copy(b)
                chose = f", device chose {where(g.index)}" if every else ""
                bad.append(f"{tag(r)} log slot {s} (device step {g.step}, model step {w.step}"
                           f"{chose}) (field, device, model): {ES.named_diff(g, w)}")
        at = r * PROGRESS_BYTES
        a, b = progress[at:at + PROGRESS_BYTES], want_progress[at:at + PROGRESS_BYTES]
        if a != b:
            bad.append(f"{tag(r)} progress (field, device, model): " + str(ES.named_diff(
                MpcEpisodesProgress.from_buffer_copy(a), MpcEpisodesProgress.from_buffer_copy(b))))
    return bad
