"""MPC episode at scale: the reference's math_mpc loop (math_model_tree.py:515-635)
driving sampled candidate sets of arbitrary size and horizon on one or more
GPUs.

Per MPC step (one `Episode.step()`):
  1. host: the reference's acceleration-limited grid around the current
     (v, beta) (:239-256), slow-down override (:312-316)            <= 451 entries
  2. device: k_sample_controls -> fp64 SoA [N, C_local] in HBM
     (candidates 0..|grid|-1 are the reference's constant sequences)
  3. device: k_rollout_argmin (the HBM-streaming kernel) + k_finalize
  4. multi-GPU: all_gather of the 808-B winner records + k_select_winner
  5. one 808-B device->host read; host applies the reference's finishing
     logic (:366-429) — on the stale optimal_trajectory when no candidate
     beat the incumbent — the stuck detector (:559-563) and the operator
     events (p = 60 / 90 / 110, :564-569)
The incumbent is sys.maxsize after the first call, as in the reference
(:428); an episode that ends (on target, :542, or "Recursive error",
:559-561) restarts from the start pose.

The device-resident forms live in device_episode.py, device_episodes.py and
streams.py, the configs in episode_config.py; their names import from here too.
"""
import math
import sys
import time

import torch

from . import math_model_tree as mmt
from .abi import (MPC_EP_ARRIVED, MPC_EP_BREAK, MPC_EP_EVENT, MPC_EP_LIMIT, MPC_EP_STALE,
                  MPC_EP_STUCK, make_problem, polygon_vertices)
from .device_episode import DeviceEpisode  # noqa: F401
from .device_episodes import DeviceEpisodes, DeviceFleet, DeviceFtEpisodes  # noqa: F401
from .distributed import exchange_winner, shard_range
from .episode_config import (CHAIN_ERRORS, ChainError, reference_episode_config,  # noqa: F401
                             tree_episode_config)
from .streams import cu_reserved_stream, cu_share_stream  # noqa: F401

def criterion0(x_t, y_t, x_0, y_0):
    """The reference's control_criterion of a line origin (an episode's first
    incumbent, math_model_tree.py:676), under its target and origin."""
    saved = (mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0)
    mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0 = x_t, y_t, x_0, y_0
    try:
        return mmt.control_criterion([x_0, y_0, 0.0])
    finally:
        mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0 = saved


class Episode:
    def __init__(self, engine, n_cand_total, n_steps, rank=0, world=1, seed=20261015,
                 integrator="rect", group=None, start=(0.0, 0.0, 0.0, 0.0, 0.0), target=(2, 3),
                 max_steps=0, obstacles=(), polygons=()):
        self.eng = engine
        self.max_steps = int(max_steps)
        # keep-out circles (x, y, r): candidates that enter one never win
        self.obstacles = [tuple(o) for o in obstacles]
        # convex keep-out polygons, each a sequence of (x, y): likewise
        self.polygons = [polygon_vertices(g) for g in polygons]
        # module globals of the reference that outlive an episode: the last
        # winner's layer states, result_v, result_beta (None: the initial
        # [[[0]]], which has no layer states)
        self.ot = None
        self.last_log = None
        self.n_total = int(n_cand_total)
        self.n_steps = int(n_steps)
        self.rank, self.world, self.group = rank, world, group
        self.lo, self.hi = shard_range(self.n_total, rank, world)
        self.n_local = self.hi - self.lo
        self.seed = seed
        self.integrator = integrator
        self.start, self.target = start, target
        dev = engine.device
        self.v_sc = torch.empty((self.n_steps, self.n_local), dtype=torch.float64, device=dev)
        self.b_sc = torch.empty_like(self.v_sc)
        self._grid_host = torch.empty(2 * 451, dtype=torch.float64).pin_memory()
        self._grid_dev = torch.empty(2 * 451, dtype=torch.float64, device=dev)
        self.kernel_ms = []          # device time of the streaming kernel, per step
        self.step_ms = []            # host wall time per MPC step
        self._ev = None
        self.reset()

    # -- episode state (reference globals of math_mpc) -------------------------
    def reset(self):
        x, y, phi, v, beta = self.start
        self.x, self.y, self.phi, self.v, self.beta = x, y, phi, v, beta
        self.x_t, self.y_t = self.target
        self.x_0, self.y_0 = x, y
        self.t = 0.0
        self.p = 1
        self.m = 0
        self.steps_for_slowing = 0
        self.episodes = getattr(self, "episodes", 0) + 1
        self.x_prev, self.y_prev = x, y
        self.recursive = False
        self.incumbent = criterion0(self.x_t, self.y_t, self.x_0, self.y_0)

    # -- one MPC step -------------------------------------------------------------
    def _grids(self):
        V = mmt.vector_of_velocities(self.v)
        B = mmt.vector_of_beta_angles(self.beta)
        if self.steps_for_slowing > 0 and V:
            vel = min(V) if min(V) > mmt.v_min else mmt.v_min
            V = [vel] * len(V)
        return V, B

    def step(self, time_kernel=False, events=None):
        t0 = time.perf_counter()
        V, B = self._grids()
        nv, nb = len(V), len(B)
        self._grid_host[:nv] = torch.tensor(V, dtype=torch.float64)
        self._grid_host[nv:nv + nb] = torch.tensor(B, dtype=torch.float64)
        self._grid_dev[:nv + nb].copy_(self._grid_host[:nv + nb], non_blocking=True)
        self.t += mmt.delta_t
        seed = (self.seed + 0x9E3779B9 * (self.p + 1000 * self.episodes)) & 0xFFFFFFFFFFFFFFFF
        self.eng.sample_controls(self._grid_dev[:nv], self._grid_dev[nv:nv + nb], self.n_local,
                                 self.n_steps, seed, index_base=self.lo, v_out=self.v_sc,
                                 beta_out=self.b_sc)
        prob = make_problem(self.x, self.y, self.phi, self.x_t, self.y_t, self.x_0, self.y_0,
                            mmt.L, self.t, self.t + mmt.delta_t)
        if time_kernel and events is None:
            events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        if events:
            events[0].record()
        self.eng.partials(prob, self.v_sc, self.b_sc, self.integrator, obstacles=self.obstacles,
                          polygons=self.polygons)
        if events:
            events[1].record()
        out = self.eng.finalize(prob, self.v_sc, self.b_sc, index_base=self.lo,
                                incumbent=self.incumbent, integrator=self.integrator,
                                out=self.eng.result)
        if self.world > 1:
            exchange_winner(self.eng, out, incumbent=self.incumbent, group=self.group)
        res = self.eng.fetch()
        if time_kernel:
            self.kernel_ms.append(events[0].elapsed_time(events[1]))
        self._advance(res)
        self.step_ms.append((time.perf_counter() - t0) * 1e3)
        return res

    def _advance(self, res):
        """The rest of math_mpc's loop body (:542-574 with :351-429); the same
        update as the device's episode_advance (csrc/mpc_episode.h)."""
        self.steps_for_slowing -= 1
        self.incumbent = float(sys.maxsize)
        step_p, status = self.p, 0
        if res.found:
            traj = res.trajectory()
            last = self.n_steps - 1
            self.ot = [list(traj[min(k, last)]) for k in range(3)]
            self.ot_v, self.ot_beta = res.v, res.beta
        else:
            status |= MPC_EP_STALE
            if self.ot is None:           # [[[0]]] has no layers: stay at the pose
                self.ot = [[self.x, self.y, self.phi] for _ in range(3)]
                self.ot_v, self.ot_beta = self.v, self.beta
        k = 0
        if self.m == 2:
            k = 2
        elif self.m == 1:
            k = 1
            self.m += 1
        elif mmt.is_on_target(self.ot[2][0], self.ot[2][1], self.x_t, self.y_t)[0]:
            self.m += 1
        self.x, self.y, self.phi = self.ot[k]
        self.v, self.beta = self.ot_v, self.ot_beta
        ended = False
        if self.recursive:                # "Recursive error." (:559-561)
            status |= MPC_EP_BREAK
            ended = True
        else:
            if self.x == self.x_prev and self.y == self.y_prev:
                self.recursive = True
                status |= MPC_EP_STUCK
            if self.p == 60:
                self._turn(-1)
                status |= MPC_EP_EVENT
            if self.p == 90:
                self._turn(+1)
                status |= MPC_EP_EVENT
            if self.p == 110:
                self._new_target(2, 3)
                status |= MPC_EP_EVENT
            self.x_prev, self.y_prev = self.x, self.y
            self.p += 1
            if mmt.is_on_target(self.x, self.y, self.x_t, self.y_t)[0]:
                status |= MPC_EP_ARRIVED
                ended = True
            elif self.max_steps > 0 and self.p > self.max_steps:
                status |= MPC_EP_LIMIT
                ended = True
        self.last_log = (res.index if res.found else -1, res.cost, step_p, self.x, self.y,
                         self.phi, self.v, self.beta, int(bool(res.found)), status)
        if ended:
            self.reset()

    def _new_target(self, tx, ty):
        self.x_t, self.y_t = tx, ty
        self.x_0, self.y_0 = self.x, self.y
        self.steps_for_slowing = 10          # slow_down(radians(30)), :128

    def _turn(self, sign):
        tx, ty = mmt._turn_target(self.x, self.y, self.phi, 2, sign)
        self._new_target(tx, ty)
        self.steps_for_slowing = 20          # slow_down(radians(90)), :175/:213


def logged_step_problems(log, cfg):
    """The problem and incumbent every logged step of a device episode was
    solved on, rebuilt on the host from the log records before it — the
    bookkeeping of episode_advance (csrc/mpc_episode.h) / Episode._advance:
    t += delta_t per step (math_model_tree.py:302), the pose of the previous
    record, the incumbent (the episode's first from cfg.incumbent0 or the
    criterion of the line origin, :676; then float(sys.maxsize), :428), the
    operator events at cfg.p_turn_right / p_turn_left / p_new_target
    (:564-569: new target, line origin at the pose) and a restart after a step
    that ended the episode (ARRIVED / LIMIT / BREAK).  `log`: the records of
    an episode from its first step on (a fresh DeviceEpisode).  Returns
    [(mpc_problem_t, incumbent)], one per record."""
    ended = MPC_EP_ARRIVED | MPC_EP_LIMIT | MPC_EP_BREAK

    def start():
        return (cfg.start_x, cfg.start_y, cfg.start_phi, 0.0, cfg.target_x, cfg.target_y,
                cfg.start_x, cfg.start_y)

    def first_incumbent(xt, yt, x0, y0):
        return cfg.incumbent0 if cfg.incumbent0 != 0.0 else criterion0(xt, yt, x0, y0)

    x, y, phi, t, xt, yt, x0, y0 = start()
    inc = first_incumbent(xt, yt, x0, y0)
    out = []
    for rec in log:
        t = t + cfg.delta_t
        out.append((make_problem(x, y, phi, xt, yt, x0, y0, cfg.L, t, t + cfg.delta_t), inc))
        inc = float(sys.maxsize)
        x, y, phi = rec.x, rec.y, rec.phi
        if rec.status & ended:
            x, y, phi, t, xt, yt, x0, y0 = start()
            inc = first_incumbent(xt, yt, x0, y0)
            continue
        if rec.p == cfg.p_turn_right:
            xt, yt = mmt._turn_target(x, y, phi, cfg.turn_distance, -1)
            x0, y0 = x, y
        if rec.p == cfg.p_turn_left:
            xt, yt = mmt._turn_target(x, y, phi, cfg.turn_distance, +1)
            x0, y0 = x, y
        if rec.p == cfg.p_new_target:
            xt, yt, x0, y0 = cfg.event_target_x, cfg.event_target_y, x, y
    return out


def percentile(xs, q):
    if not xs:
        return math.nan
    s = sorted(xs)
    i = min(len(s) - 1, max(0, int(round(q / 100.0 * (len(s) - 1)))))
    return s[i]
