"""Batches of device-resident episodes: R robots' episodes in HBM, advanced by
one host call for up to k MPC steps of every robot (mpc_episodes_* and
mpc_fulltree_episodes_*)."""
import ctypes

import numpy as np
import torch

from . import native
from .abi import (INTEGRATORS, LOG_BYTES, MPC_MAX_OBSTACLES, PROGRESS_BYTES, MpcEpisodeConfig,
                  MpcFulltreeEpisodeConfig, make_obstacles)

# numpy view of mpc_episode_log_t (include/mpc_rollout.h), 80 bytes
_LOG_DTYPE = [("step", "<i8"), ("index", "<i8"), ("p", "<i4"), ("episode", "<i4"),
              ("found", "<i4"), ("status", "<i4"), ("cost", "<f8"), ("x", "<f8"), ("y", "<f8"),
              ("phi", "<f8"), ("v", "<f8"), ("beta", "<f8")]


class _RobotBatch:
    """What the two batched forms share: the robots' state, per robot a log
    ring and a progress record in HBM, and their decoding."""

    def __init__(self, device, n_robots, state_bytes, integrator, log_capacity):
        self.lib = native.lib()
        self._C = native.calls()
        self.R = n_robots
        self._integ = INTEGRATORS[integrator]
        self.state = torch.zeros(state_bytes(self.R), dtype=torch.uint8, device=device)
        self.log_capacity = int(log_capacity)
        self.log = torch.zeros(self.R * self.log_capacity * LOG_BYTES, dtype=torch.uint8,
                               device=device)
        self.progress = torch.zeros(self.R * PROGRESS_BYTES, dtype=torch.uint8, device=device)

    def read_progress(self):
        """(calls, stop, work) per robot (numpy arrays; syncs).  work: the
        candidates (DeviceEpisodes) or leaves (DeviceFtEpisodes) rolled out."""
        raw = self.progress.cpu().numpy()
        p = np.frombuffer(raw.tobytes(), dtype=[("calls", "<i4"), ("stop", "<i4"),
                                                ("candidates", "<i8")])
        return p["calls"].copy(), p["stop"].copy(), p["candidates"].copy()

    def read_logs(self, first_step=None):
        """Per robot, its log records (numpy structured array, mpc_episode_log_t
        fields) of steps [first, calls): first = first_step[r] if given, else
        everything still in the ring (the last log_capacity steps)."""
        calls, _, _ = self.read_progress()
        raw = np.frombuffer(self.log.cpu().numpy().tobytes(), dtype=_LOG_DTYPE)
        raw = raw.reshape(self.R, self.log_capacity)
        out = []
        for r in range(self.R):
            n = int(calls[r])
            lo = max(0, n - self.log_capacity)
            if first_step is not None:
                lo = max(lo, int(first_step[r]))
            out.append(raw[r, [s % self.log_capacity for s in range(lo, n)]])
        return out


class DeviceEpisodes(_RobotBatch):
    """R robots' MPC episodes in HBM (mpc_episodes_*, csrc/mpc_episodes.h):
    one block per robot runs its episode's MPC steps back to back — the grid
    around its control, the reference's enumeration of the step's |V| x |B|
    constant sequences, the N-step rollout, the strict-< first minimum, the
    winner's layer states and the episode update — so `run(k)` is ONE launch
    for up to k MPC steps of every robot, with no host round trip and no
    lockstep.  cfgs: one MpcEpisodeConfig per robot (start, target and rules:
    `tree_episode_config` for run_math_model.py's loop, the reference_episode_
    config of math_mpc for the operator scenario).

    obstacles / set_obstacles(): keep-out circles (x, y, r) in world
    coordinates, at most 16, ONE table for all robots (one map), with the
    semantics of the one-shot entries (mpc_rollout_partials_obstacles): a
    candidate that ends a step of its horizon strictly inside one never wins;
    if all of a step's candidates do, the step has no winner (MPC_EP_STALE).
    They are passed with every run() (mpc_episodes_run_obstacles) and are not
    part of the state.  read_blocked(): per robot the candidates blocked in
    the steps of the last run().  With no circles run() is the call made
    without the feature.  Robots as each other's obstacles: DeviceFleet,
    below (predict=True: their circles move with them; predict="plan": along
    their own plans).  Not provided: a table
    per robot, a radius per robot.  (The full-tree episodes take circles too:
    DeviceFtEpisodes.)"""

    def __init__(self, engine, cfgs, n_steps=3, integrator="qk21", log_capacity=1024,
                 obstacles=()):
        self.eng = engine
        self.cfgs = list(cfgs)
        self.n_steps = int(n_steps)
        self.integrator = integrator
        super().__init__(engine.device, len(self.cfgs), native.lib().mpc_episodes_state_bytes,
                         integrator, log_capacity)
        self.n_blocked = torch.zeros(self.R, dtype=torch.int64, device=engine.device)
        self._obs, self._n_obs, self._counted = None, 0, False
        self.set_obstacles(obstacles)
        self.reset()

    def reset(self):
        arr = (MpcEpisodeConfig * self.R)(*self.cfgs)
        self._C.mpc_episodes_reset(ctypes.byref(arr), self.R, self.state.data_ptr(),
                                   native.current_stream())
        self.progress.zero_()
        self._counted = False        # (read_blocked(): zeros until the next run())

    def set_obstacles(self, circles):
        """The keep-out circles of the run() calls from now on."""
        obs, n = make_obstacles(circles)
        if n > MPC_MAX_OBSTACLES:
            raise ValueError(f"at most {MPC_MAX_OBSTACLES} obstacles")
        self._obs, self._n_obs = obs, n

    def _obstacle_args(self):
        """None (the plain entry), or what mpc_episodes_run_obstacles takes
        besides: (circles, count, n_blocked_out)."""
        if not self._n_obs:
            return None
        return self._obs, self._n_obs, self.n_blocked.data_ptr()

    def run(self, max_calls):
        """Enqueue up to max_calls MPC steps of every still-running robot."""
        args = (self.R, self.n_steps, self._integ, int(max_calls), self.log.data_ptr(),
                self.log_capacity, self.progress.data_ptr())
        extra = self._obstacle_args()
        self._counted = extra is not None
        if extra is None:
            self._C.mpc_episodes_run(self.state.data_ptr(), *args, native.current_stream())
        else:
            *circles, blocked = extra
            self._C.mpc_episodes_run_obstacles(self.state.data_ptr(), *circles, *args, blocked,
                                               native.current_stream())

    def read_blocked(self):
        """Per robot (numpy int64; syncs) the candidates that the circles
        blocked in the steps of the last run() (zeros after a run() without
        circles: nothing can be blocked)."""
        if not self._counted:
            return np.zeros(self.R, dtype=np.int64)
        return self.n_blocked.cpu().numpy().copy()


def fleet_reach(cfgs, n_steps, clearance, predict=False):
    """The reach beyond which a robot cannot matter to another within one
    fleet call: max over the cfgs of n_steps * delta_t * max(|v_max|, |v_min|)
    — the farthest any step-end state of the horizon lies from the start, every
    layer driven at the velocity bound — times (1 + 2**-40) for the roundings
    of the step length and the recurrence, plus clearance.  A robot at that
    distance or beyond has its circle out of every candidate's states.
    predict=True (DeviceFleet(predict=True)): 2 * far * (1 + 2**-40) +
    clearance — a neighbour's step-N circle lies up to one horizon's travel
    from where the neighbour stands.  DeviceFleet(predict="plan") takes the
    same reach: the two plan points a neighbour publishes are at most one
    step's travel apart, so its step-N circle, a2 + (N - 2) * (a2 - a1), lies
    within one horizon of the neighbour too."""
    far = max(int(n_steps) * c.delta_t * max(abs(c.v_max), abs(c.v_min)) for c in cfgs)
    if predict:
        return 2 * far * (1.0 + 2.0 ** -40) + float(clearance)
    return far * (1.0 + 2.0 ** -40) + float(clearance)


class DeviceFleet(DeviceEpisodes):
    """DeviceEpisodes whose robots keep clear of each other
    (mpc_episodes_fleet_begin / _run, csrc/mpc_episodes_fleet.h): a FLEET CALL
    advances every still-running robot by exactly one MPC step, during which
    robot r's circles are the static `obstacles` and one circle of radius
    `clearance` around each chosen other robot, where that robot stood when
    the call began (ended robots stay where they stand and stay obstacles).
    Chosen: of the robots nearer than `reach`, the 16 - len(obstacles) nearest,
    ties to the lower index.  `run(k)` is ONE ABI call for k fleet calls (one
    launch each: lockstep is the stream's order, nothing waits).

    predict=True (mpc_episodes_fleet_run_predicted): each chosen neighbour's
    circle moves over the horizon with the neighbour's last displacement — at
    step j it stands at (x_q + j * dx_q, y_q + j * dy_q), and the state after
    step j is tested against the step-j circles only.  A robot that has ended,
    or has not moved yet (fleet call 0), stands still.  The object then owns
    the motion board too (two sides of R {dx, dy}, the pose board's parity).

    predict="plan" (mpc_episodes_fleet_run_planned): each chosen neighbour's
    circle follows the neighbour's own plan, the arc of its last winner.  Every
    robot publishes two points (a1, a2) of it — the layers it means to reach
    in the next call and the one after; a robot that has ended, took no step
    or found no winner publishes its position twice — and a neighbour's circle
    stands at a1 for step 1, at a2 for step 2 and at a2 + (j - 2) * (a2 - a1)
    for step j >= 3.  The object then owns the plan board (`self.plan`: two
    sides of R {x1, y1, x2, y2}, the pose board's parity); `self.motion` stays
    None.  Any other value of predict raises ValueError.

    reach=None: fleet_reach(cfgs, n_steps, clearance, bool(predict)), the
    largest distance a robot of the batch covers in one horizon (predict: two
    horizons, the neighbour's travel too) plus clearance; a larger reach
    changes nothing, a smaller one ignores robots that could have mattered.
    The object owns the pose board, the count of fleet calls since reset()
    and the neighbour buffer.  read_blocked(): per robot the candidates
    blocked over the fleet calls of the last run().  read_neighbours(): the
    last fleet call's (within reach before the cap, chosen robots in ascending
    (distance, index) order) per robot.
    Not provided: any prediction but the constant displacement and the two
    plan points, per-robot radii, per-robot static tables."""

    def __init__(self, engine, cfgs, clearance, n_steps=3, integrator="qk21", log_capacity=1024,
                 obstacles=(), reach=None, predict=False):
        cfgs = list(cfgs)
        self.clearance = float(clearance)
        if predict != "plan" and predict not in (True, False):
            raise ValueError(f"predict is False, True or 'plan', not {predict!r}")
        self.predict = predict if predict == "plan" else bool(predict)
        self.reach = (fleet_reach(cfgs, n_steps, clearance, bool(self.predict)) if reach is None
                      else float(reach))
        n = len(cfgs)
        self.motion = (torch.zeros(native.lib().mpc_episodes_fleet_motion_bytes(n),
                                   dtype=torch.uint8, device=engine.device)
                       if self.predict is True else None)
        self.plan = (torch.zeros(native.lib().mpc_episodes_fleet_plan_bytes(n),
                                 dtype=torch.uint8, device=engine.device)
                     if self.predict == "plan" else None)
        self.board = torch.zeros(native.lib().mpc_episodes_fleet_board_bytes(n), dtype=torch.uint8,
                                 device=engine.device)
        self.neighbours = torch.full((n, 1 + MPC_MAX_OBSTACLES), -1, dtype=torch.int32,
                                     device=engine.device)
        self.neighbours[:, 0] = 0
        self.call0 = 0
        super().__init__(engine, cfgs, n_steps, integrator, log_capacity, obstacles)

    def reset(self):
        super().reset()
        self._C.mpc_episodes_fleet_begin(self.state.data_ptr(), self.R, self.board.data_ptr(),
                                         native.current_stream())
        self.call0 = 0
        self.neighbours.fill_(-1)        # (read_neighbours(): (0, []) until the next run())
        self.neighbours[:, 0] = 0

    def run(self, n_calls):
        """Enqueue n_calls fleet calls: one MPC step of every still-running
        robot each."""
        n_calls = int(n_calls)
        rest = (self.call0, self._obs, self._n_obs, self.clearance, self.reach, self.R,
                self.n_steps, self._integ, n_calls, self.log.data_ptr(), self.log_capacity,
                self.progress.data_ptr(), self.n_blocked.data_ptr(), self.neighbours.data_ptr(),
                native.current_stream())
        if self.predict == "plan":
            self._C.mpc_episodes_fleet_run_planned(self.state.data_ptr(), self.board.data_ptr(),
                                                   self.plan.data_ptr(), *rest)
        elif self.predict:
            self._C.mpc_episodes_fleet_run_predicted(self.state.data_ptr(), self.board.data_ptr(),
                                                     self.motion.data_ptr(), *rest)
        else:
            self._C.mpc_episodes_fleet_run(self.state.data_ptr(), self.board.data_ptr(), *rest)
        if n_calls > 0:
            self._counted = True
            self.call0 += n_calls

    def read_neighbours(self):
        """Per robot (within, chosen) of the last fleet call (syncs): the robots
        within reach before the cap, and the chosen ones' indices, nearest
        first; (0, []) for a robot that took no step in it."""
        raw = self.neighbours.cpu().numpy()
        return [(int(row[0]), [int(q) for q in row[1:] if q >= 0]) for row in raw]


class DeviceFtEpisodes(_RobotBatch):
    """R robots' run_math_model.py episodes with the script's own full-tree MPC
    step, in HBM (mpc_fulltree_episodes_*, csrc/mpc_ftepisodes.h): `run(k)`
    enqueues up to k calls of every robot with no host step in between — per
    call the robots still running are compacted and every one's S1^3 leaves
    are spread over the whole GPU (the load-balanced lockstep form).  cfgs:
    MpcFulltreeEpisodeConfig per robot; v_grid / beta_grid: the script's grids
    as device tensors.

    obstacles / set_obstacles(): keep-out circles (x, y, r) in world
    coordinates, at most 16, ONE table for all robots and all calls of a
    run() (mpc_fulltree_episodes_run_obstacles): a leaf with a layer state
    strictly inside one never wins; a call whose leaves are all blocked has
    no winner (the stale one is returned again; on a robot's first call the
    episode stops with MPC_EP_NO_TRAJ).  A robot that starts inside a circle
    can leave it.  read_blocked(): per robot the leaves blocked in the calls
    of the last run().  With no circles run() is the call made without the
    feature."""

    def __init__(self, engine, cfgs, v_grid, beta_grid, L, delta_t, eps, integrator="qk21",
                 log_capacity=256, obstacles=()):
        self.cfgs = (MpcFulltreeEpisodeConfig * len(cfgs))(*cfgs)
        self.vg, self.bg = v_grid, beta_grid
        self.L, self.delta_t, self.eps = float(L), float(delta_t), float(eps)
        super().__init__(engine.device, len(cfgs), native.lib().mpc_fulltree_episodes_state_bytes,
                         integrator, log_capacity)
        self.n_blocked = torch.zeros(self.R, dtype=torch.int64, device=engine.device)
        self._obs, self._n_obs, self._counted = None, 0, False
        self.set_obstacles(obstacles)
        self.reset()

    def reset(self):
        self._C.mpc_fulltree_episodes_reset(ctypes.byref(self.cfgs), self.R,
                                            self.state.data_ptr(), native.current_stream())
        self.progress.zero_()
        self._counted = False        # (read_blocked(): zeros until the next run())

    def set_obstacles(self, circles):
        """The keep-out circles of the run() calls from now on."""
        obs, n = make_obstacles(circles)
        if n > MPC_MAX_OBSTACLES:
            raise ValueError(f"at most {MPC_MAX_OBSTACLES} obstacles")
        self._obs, self._n_obs = obs, n

    def read_blocked(self):
        """Per robot (numpy int64; syncs) the leaves that the circles blocked
        in the calls of the last run() (zeros after a run() without circles)."""
        if not self._counted:
            return np.zeros(self.R, dtype=np.int64)
        return self.n_blocked.cpu().numpy().copy()

    def run(self, max_calls):
        """Enqueue up to max_calls MPC calls of every still-running robot
        (three launches per call, each bounded by one call's S1^3 leaves per
        robot spread over the GPU: no launch approaches the compute-lockup
        timeout whatever S1 and max_calls are)."""
        args = (self.R, self.vg.data_ptr(), self.vg.numel(), self.bg.data_ptr(), self.bg.numel(),
                self.L, self.delta_t, self.eps, self._integ, int(max_calls), self.log.data_ptr(),
                self.log_capacity, self.progress.data_ptr())
        self._counted = bool(self._n_obs)
        if not self._n_obs:
            self._C.mpc_fulltree_episodes_run(self.state.data_ptr(), *args,
                                              native.current_stream())
        else:
            self._C.mpc_fulltree_episodes_run_obstacles(
                self.state.data_ptr(), self._obs, self._n_obs, *args, self.n_blocked.data_ptr(),
                native.current_stream())
