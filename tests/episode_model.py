"""The device-resident episode's bookkeeping restated in plain Python with ALL
of its state: what csrc/mpc_episode.h (episode_restart, episode_prepare,
episode_early_prepare, turn_target, episode_advance), select_index
(csrc/mpc_kernels.h) and episode_grids (csrc/mpc_generated.h) compute, field
for field, so a test can compare an EpisodeState with `==` on the bits.

EpisodeModel extends oracle.parity.OracleMpcEpisode (pinned to the reference's
recorded model run by tests/test_parity_oracle.py; this model is pinned to it
and to the same recording by tests/test_episode_model_cpu.py) with what that
class lacks: the run_math_model.py stuck rule (cfg.stop_rule 1), the horizon
clamp of the winner's layers, the selection over n gathered results, the grids
from the cfg's own fields with the kEpMaxGrid clamp, the sampler seed, the
early-publication record, and the step / t / K / seed conventions of the
device head (t, K and seed are those of the NEXT step, as episode_prepare
leaves them).  Differences from the reference that include/mpc_rollout.h
documents are stated here as the device has them: squares are x * x (the
reference's `** 2` is libm pow), a step without winner and without a
trajectory stays at the pose (the reference's [[[0]]] would raise).

sin / cos of turn_target come from the host build of sincos_fast
(harness.trig_eval) unless another pair is switched in; K and the restart
incumbent of incumbent0 == 0 from the host build of consts_from_problem and
cost (harness.replica_consts / replica_cost).  Nothing is read from a device.
Test infrastructure only."""
import ctypes
import math
from collections import namedtuple

import numpy as np

import episode_state as ES
import harness
from diplomjourney_amd.abi import MPC_MAX_STEPS, MpcEpisodeLog, MpcResult, make_problem
from oracle import parity as P

INC_MAX = 9223372036854775808.0        # float(sys.maxsize), :428
INT64_MAX = 2 ** 63 - 1
U64 = 2 ** 64 - 1
NO_KEY = (1, 0.0)                      # cost_key's ~0: NaN, +inf, or index < 0

# One gathered result row (mpc_result_t).  traj: at least min(n_steps, 3)
# layer states [x, y, phi]; the device reads no layer at or past n_steps.
Result = namedtuple("Result", "cost index n_steps v beta traj")

LOG_FIELDS = tuple(n for n, _ in MpcEpisodeLog._fields_)


def device_sincos(x):
    _, s, c = harness.trig_eval(np.array([x], dtype=np.float64))
    return float(s[0]), float(c[0])


def libm_sincos(x):
    return math.sin(x), math.cos(x)


def result_from_row(row):
    """oracle.parity's ROW (cost, index, v, beta, three clamped layers) as a Result."""
    return Result(float(row[0]), int(row[1]), 3, float(row[2]), float(row[3]),
                  [[float(q) for q in row[4 + 3 * k:7 + 3 * k]] for k in range(3)])


def result_struct(r, found=0, poison=None):
    """mpc_result_t of a Result; layers past r.traj hold `poison` (never read)."""
    out = MpcResult(cost=r.cost, index=r.index, found=found, n_steps=r.n_steps, v=r.v,
                    beta=r.beta)
    for s in range(MPC_MAX_STEPS):
        for q in range(3):
            out.traj[s][q] = r.traj[s][q] if s < len(r.traj) else (
                poison if poison is not None else 0.0)
    return out


def cost_key(cost, index):
    """(key, index) as select_index orders the rows (cost_key, rec_less)."""
    if index < 0:
        return NO_KEY, INT64_MAX
    if not cost < math.inf:
        return NO_KEY, index
    return (0, cost + 0.0), index


def select(results):
    """select_index: (row number of the lexicographic (cost, index) minimum,
    whether its key is a cost's).  Row 0 when no row has an index."""
    best, bk, bi = 0, None, None
    for r, row in enumerate(results):
        k, i = cost_key(row.cost, row.index)
        if r == 0 or (k, i) < (bk, bi):
            best, bk, bi = r, k, i
    return best, bk != NO_KEY


def turn_target(ax, ay, aphi, d, R, sign, sincos):
    """turn_target (mpc_episode.h) = math_model_tree.py:142-215: the four
    heading sectors in the reference's order, each with its expressions."""
    pi = math.pi
    if pi / 2 <= aphi <= 3 * pi / 2:
        if aphi <= pi:
            sn, cs = sincos(aphi - pi / 2)
            return (ax - sign * d * cs - R * sn, ay - sign * d * sn + R * cs), 0
        sn, cs = sincos(aphi - pi)
        return (ax + sign * d * sn - R * cs, ay - sign * d * cs - R * sn), 1
    if aphi <= 2 * pi:
        sn, cs = sincos(aphi - 3 * pi / 2)
        return (ax + sign * d * cs + R * sn, ay + sign * d * sn - R * cs), 2
    sn, cs = sincos(aphi)
    return (ax - sign * d * sn + R * cs, ay + sign * d * cs + R * sn), 3


class EpisodeModel(P.OracleMpcEpisode):
    """The whole EpisodeState's worth of an episode.  After the constructor
    the model is k_episode_reset's state; advance(results) is one
    k_episode_advance; sample() what a step's grids publish."""

    def __init__(self, cfg, sincos=device_sincos):
        self.sincos = sincos
        self.step = 0
        self.nv = self.nb = 0
        self.grid_v, self.grid_b = [0.0] * ES.EP_MAX_GRID, [0.0] * ES.EP_MAX_GRID
        self.v = self.beta = 0.0
        # the launches' hand-off words: no part of the bookkeeping, carried along
        self.done = self.chain_error = self.p2p_seq = self.gathered_tag = 0
        self.chain_pub = [0] * ES.PUB_WORDS
        self.trace = {}
        super().__init__(cfg)          # episodes = 0, no trajectory, restart()
        self.has_traj = 0
        self.prepare()
        self.early = self.early_prepare()

    # -- start of an episode / of a step ------------------------------------
    def consts(self, x, y, phi, t_a, t_b):
        return harness.replica_consts(
            make_problem(x, y, phi, self.xt, self.yt, self.x0, self.y0, self.c.L, t_a, t_b),
            ctypes.sizeof(ES.Consts))

    def restart(self):
        """episode_restart."""
        c = self.c
        self.x, self.y, self.phi = c.start_x, c.start_y, c.start_phi
        self.v, self.beta = c.start_v, c.start_beta
        self.xt, self.yt = c.target_x, c.target_y
        self.x0, self.y0 = c.start_x, c.start_y
        self.t, self.p, self.m, self.slowing = 0.0, 1, 0, 0
        self.episodes += 1
        self.recursive = 0
        if c.incumbent0 != 0.0:
            self.incumbent = c.incumbent0
        else:
            self.incumbent = harness.replica_cost(
                self.consts(self.x0, self.y0, 0.0, 0.0, c.delta_t), self.x0, self.y0)

    def seed_rule(self):
        return (self.c.seed + 0x9E3779B9 * ((self.p + 1000 * self.episodes) & U64)) & U64

    def prepare(self):
        """episode_prepare: t += dt, the step's constants and sampler seed."""
        t = self.t + self.c.delta_t
        self.K = self.consts(self.x, self.y, self.phi, t, t + self.c.delta_t)
        self.t = t
        self.seed = self.seed_rule()

    def pose_ok(self, x, y):
        """early_pose_ok."""
        c = self.c
        if c.stop_rule == 1 and x == self.x and y == self.y and self.recursive >= 1:
            return False
        ex, ey = self.xt - x, self.yt - y
        return not ex * ex + ey * ey <= c.eps

    def early_prepare(self):
        """episode_early_prepare: the EarlyPub record of the next step."""
        c = self.c
        t = self.t + c.delta_t
        common = (not (c.stop_rule == 0 and self.recursive) and self.p != c.p_turn_right
                  and self.p != c.p_turn_left and self.p != c.p_new_target
                  and not (c.max_steps > 0 and self.p + 1 > c.max_steps))
        k = 2 if self.m == 2 else (1 if self.m == 1 else 0)
        x, y, ph = self.ot[k] if self.has_traj else (self.x, self.y, self.phi)
        return dict(step=self.step, k=k if common else -1, alt=1 if self.pose_ok(x, y) else 0,
                    t=t, h=(t + c.delta_t) - t, hl=0.5 * ((t + c.delta_t) - t), x=x, y=y, ph=ph)

    def begin_step(self):
        """(mpc_problem_t, incumbent) of the step the head is prepared for."""
        return (make_problem(self.x, self.y, self.phi, self.xt, self.yt, self.x0, self.y0,
                             self.c.L, self.t, self.t + self.c.delta_t), self.incumbent)

    # -- the step's grids ------------------------------------------------------
    def grids(self):
        """episode_grids: (V, B, seed) from the cfg's fields (:239-256), each
        clamped to kEpMaxGrid points, the slow-down override (:312-316) with the
        minimum over the whole unclamped V."""
        c = self.c
        V = []
        for i in range(1 + 2 * int(c.ratio_v)):
            cand = self.v + c.delta_v * (float(i) - c.ratio_v)
            if (not cand < 0.0) and cand < c.v_max:
                V.append(cand)
        vmin = min(V) if V else math.inf
        V = V[:ES.EP_MAX_GRID]
        if self.slowing > 0 and V:
            V = [vmin if vmin > c.v_min else c.v_min] * len(V)
        B = []
        for i in range(1 + 2 * int(c.ratio_beta)):
            cand = self.beta + c.delta_beta * (float(i) - c.ratio_beta)
            if abs(cand) <= c.beta_bound:
                B.append(cand)
        return V, B[:ES.EP_MAX_GRID], self.seed_rule()

    def sample(self):
        """What a step's sampler publishes in the state: nv, nb, the grids."""
        V, B, seed = self.grids()
        self.nv, self.nb = len(V), len(B)
        self.grid_v[:len(V)] = V
        self.grid_b[:len(B)] = B
        return V, B, seed

    # -- the update -------------------------------------------------------------
    def advance(self, results, incumbent=None, end_chain=True, restart=True):
        """advance_from_results + episode_advance + episode_prepare over the
        gathered rows (a list of Result, or one oracle.parity ROW); returns the
        log record as a dict of mpc_episode_log_t's fields.  `incumbent`, when
        given, must be the model's own (OracleMpcEpisode's signature).
        restart=False is episode_advance<false> (the batched robots of
        csrc/mpc_episodes.h): a step that ends the episode returns right after
        its log record — no restart, no prepare, so t, K and seed stay those
        of the step that ended it."""
        if isinstance(results, np.ndarray):
            results = [result_from_row(results)]
        assert incumbent is None or incumbent == self.incumbent
        c = self.c
        best, keyed = select(results)
        r = results[best]
        found = bool(keyed and r.cost < self.incumbent)
        rec = dict(step=self.step, index=r.index if found else -1, p=self.p,
                   episode=self.episodes, found=int(found), cost=r.cost)
        tr = dict(m0=self.m, found=int(found), had_traj=int(bool(self.has_traj)), row=best)
        self.slowing -= 1
        self.incumbent = INC_MAX
        self.step += 1
        status = 0
        if found:
            last = r.n_steps - 1
            self.ot = [list(r.traj[min(k, last)]) for k in range(3)]
            self.ot_v, self.ot_beta = r.v, r.beta
            self.has_traj = 1
        else:
            status |= P.STALE
            if not self.has_traj:
                self.ot = [[self.x, self.y, self.phi] for _ in range(3)]
                self.ot_v, self.ot_beta = self.v, self.beta
        k = 0
        if self.m == 2:
            k = 2
        elif self.m == 1:
            k = 1
            self.m += 1
        else:
            ex, ey = self.xt - self.ot[2][0], self.yt - self.ot[2][1]
            if ex * ex + ey * ey <= c.eps:
                self.m += 1
        tr.update(k=k, m1=self.m)
        x_prev, y_prev = self.x, self.y
        self.x, self.y, self.phi = self.ot[k]
        self.v, self.beta = self.ot_v, self.ot_beta
        same = self.x == x_prev and self.y == y_prev
        ended = None
        if c.stop_rule == 0 and self.recursive:
            status |= P.BREAK
            ended = "break"
        elif same and c.stop_rule == 1 and self.recursive >= 1:
            self.recursive += 1
            status |= P.STUCK | P.BREAK
            ended = "stuck_break"
        else:
            if same:
                self.recursive += 1
                status |= P.STUCK
            sectors = []
            for p_ev, sign in ((c.p_turn_right, -1.0), (c.p_turn_left, +1.0)):
                if self.p == p_ev:
                    (self.xt, self.yt), sector = turn_target(
                        self.x, self.y, self.phi, c.turn_distance, c.radius_u_turn, sign,
                        self.sincos)
                    sectors.append(sector)
                    self.x0, self.y0 = self.x, self.y
                    self.slowing = c.slow_turn
                    status |= P.EVENT
            if self.p == c.p_new_target:
                self.xt, self.yt = c.event_target_x, c.event_target_y
                self.x0, self.y0 = self.x, self.y
                self.slowing = c.slow_new_target
                status |= P.EVENT
            tr.update(sectors=sectors)
            self.p += 1
            ex, ey = self.xt - self.x, self.yt - self.y
            if ex * ex + ey * ey <= c.eps:
                status |= P.ARRIVED
                ended = "arrived"
            elif c.max_steps > 0 and self.p > c.max_steps:
                status |= P.LIMIT
                ended = "limit"
        rec.update(status=status, x=self.x, y=self.y, phi=self.phi, v=self.v, beta=self.beta)
        tr.update(status=status, ended=ended)
        self.trace = tr
        if ended and not restart:
            return rec
        if ended:
            self.restart()
        self.prepare()
        if end_chain:
            self.chain_pub = [0] * ES.PUB_WORDS
        return rec

    # -- the state's bytes --------------------------------------------------------
    def to_state(self):
        S = ES.EpisodeState()
        h = S.h
        ctypes.memmove(ctypes.addressof(h.K), self.K, ctypes.sizeof(ES.Consts))
        h.incumbent = self.incumbent
        h.x, h.y, h.phi, h.v, h.beta = self.x, self.y, self.phi, self.v, self.beta
        h.x_t, h.y_t, h.x_0, h.y_0, h.t = self.xt, self.yt, self.x0, self.y0, self.t
        h.seed, h.step = self.seed, self.step
        h.p, h.m, h.steps_for_slowing, h.episodes = self.p, self.m, self.slowing, self.episodes
        h.nv, h.nb, h.recursive, h.has_traj = self.nv, self.nb, int(self.recursive), int(
            self.has_traj)
        for k in range(3):
            for q in range(3):
                S.st.ot[k][q] = self.ot[k][q]
        S.st.v, S.st.beta = self.ot_v, self.ot_beta
        for name, val in self.early.items():
            setattr(S.early, name, val)
        for i in range(ES.EP_MAX_GRID):
            S.grid_v[i], S.grid_b[i] = self.grid_v[i], self.grid_b[i]
        S.done, S.chain_error, S.p2p_seq = self.done, self.chain_error, self.p2p_seq
        for i in range(ES.PUB_WORDS):
            S.chain_pub[i] = self.chain_pub[i]
        S.gathered_tag = self.gathered_tag
        return S

    @classmethod
    def from_state(cls, cfg, S, sincos=device_sincos):
        """The model of a state that was written or read back.  (The model
        keeps K as bytes: it is taken over, not re-derived.)"""
        M = cls.__new__(cls)
        M.c, M.sincos, M.trace = cfg, sincos, {}
        h = S.h
        M.K = bytes(h.K)
        M.incumbent = h.incumbent
        M.x, M.y, M.phi, M.v, M.beta = h.x, h.y, h.phi, h.v, h.beta
        M.xt, M.yt, M.x0, M.y0, M.t = h.x_t, h.y_t, h.x_0, h.y_0, h.t
        M.seed, M.step = h.seed, h.step
        M.p, M.m, M.slowing, M.episodes = h.p, h.m, h.steps_for_slowing, h.episodes
        M.nv, M.nb, M.recursive, M.has_traj = h.nv, h.nb, h.recursive, h.has_traj
        M.ot = [[S.st.ot[k][q] for q in range(3)] for k in range(3)]
        M.ot_v, M.ot_beta = S.st.v, S.st.beta
        M.early = {n: getattr(S.early, n) for n, _ in ES.EarlyPub._fields_}
        M.grid_v, M.grid_b = list(S.grid_v), list(S.grid_b)
        M.done, M.chain_error, M.p2p_seq = S.done, S.chain_error, S.p2p_seq
        M.chain_pub = list(S.chain_pub)
        M.gathered_tag = S.gathered_tag
        return M


def log_struct(rec):
    """mpc_episode_log_t of advance()'s record."""
    return MpcEpisodeLog(**{n: rec[n] for n in LOG_FIELDS})
