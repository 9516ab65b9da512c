"""A fleet of the batched device episodes (mpc_episodes_fleet_run and
mpc_episodes_fleet_run_predicted, csrc/mpc_episodes_fleet.h) restated on the
host: R robots' models in lockstep.  Per fleet call a snapshot of every robot's
position is taken; each still-running robot's circles become the static ones
and one per chosen neighbour; then its mpc_step() runs.  Ended robots take no
step, keep their position and stay in the snapshot.

Fleet(predict=False): robots_obstacle_model.ObstacleRobotModels, a neighbour's
circle (x_q, y_q, clearance) standing for the whole horizon.  predict=True:
MotionRobotModels, whose `score` masks the state after horizon step j with
step j's circles only — the static ones, unmoved, and each chosen neighbour's
at (x_q + j * dx_q, y_q + j * dy_q), (dx_q, dy_q) its last call's displacement.

The neighbours are chosen by a brute-force restatement of the header's rule:
of the robots q != r with d2 < reach * reach the K = 16 - len(static) smallest
by (d2, q).  d2 and the moved centres are the host builds of the device's
fleet_d2 and fleet_predict (tests/fleet_harness.cpp: numpy has no fused
multiply-add), so a tie or a last bit on the device is one here.

The fleet keeps, beside what the robots' models keep (the blocked count per
step, the margin between any state and any rim, moving or not): per call the
positions and displacements (`boards`, `motions`) and per robot the (within
reach, chosen) pair, the smallest |sqrt(d2) - reach| over every pair a running
robot looked at, and the smallest d2 gap between the K-th and the (K+1)-th
neighbour of a capped selection.  A GPU test asserts these margins before it
looks at a kernel, unless exact ties are what it is about.  A MotionRobotModel
keeps besides, per MPC step, which (horizon step, table entry) hits which
candidate, the candidates' beta, and the blocked count, winner and mask under
each WRONG MULTIPLIER of the displacement: 0 (the circle stands), j - 1, j + 1,
N and 1 — a test asserts that a kernel which used any of them would have been
caught.  Test infrastructure only."""
import ctypes
import math

import numpy as np

import harness
import robots_model as RM
import robots_obstacle_model as OM
from diplomjourney_amd.abi import MPC_MAX_OBSTACLES

_P = ctypes.c_void_p
CAP_GAP = 1e-12          # the d2 gap a capped selection must have at its boundary
ROW = 1 + MPC_MAX_OBSTACLES
WRONG = {"0": lambda j, n: 0, "j-1": lambda j, n: j - 1, "j+1": lambda j, n: j + 1,
         "N": lambda j, n: n, "1": lambda j, n: 1}


def _lib():
    L = harness.host_lib("fleet_harness")
    for fn in (L.fleet_d2_row, L.fleet_predict_row):
        fn.argtypes = [_P, _P, ctypes.c_int64, ctypes.c_int64, _P]
        fn.restype = None
    return L


def d2_row(pos, r):
    """fleet_d2(robot r, robot q) for every q: the device function's host build."""
    x = np.ascontiguousarray([p[0] for p in pos], dtype=np.float64)
    y = np.ascontiguousarray([p[1] for p in pos], dtype=np.float64)
    out = np.empty(len(pos))
    _lib().fleet_d2_row(x.ctypes.data_as(_P), y.ctypes.data_as(_P), len(pos), int(r),
                        out.ctypes.data_as(_P))
    return out


def centres(x, d, j):
    """fleet_predict(x[q], d[q], j) for every q: the device function's host build."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    out = np.empty(len(x))
    _lib().fleet_predict_row(x.ctypes.data_as(_P), d.ctypes.data_as(_P), len(x), int(j),
                             out.ctypes.data_as(_P))
    return out


def select(d2, r, reach, keep):
    """The rule, by brute force, from robot r's row of d2: (robots within reach
    before the cap, the chosen in ascending (d2, q) order, |sqrt(d2) - reach|'s
    minimum, the d2 gap at the cap's boundary or inf)."""
    reach2 = reach * reach
    others = [q for q in range(len(d2)) if q != r]
    near = sorted((q for q in others if d2[q] < reach2), key=lambda q: (d2[q], q))
    edge = min((abs(math.sqrt(d2[q]) - reach) for q in others), default=math.inf)
    gap = float(d2[near[keep]] - d2[near[keep - 1]]) if 0 < keep < len(near) else math.inf
    return len(near), near[:keep], edge, gap


class MotionRobotModel(OM.ObstacleRobotModel):
    """ObstacleRobotModel whose circles are `circles` (static: (x, y, r)) and
    then `moving` ((x, y, dx, dy, r) per chosen neighbour), set per call."""

    def __init__(self, cfg, n_steps, integ, circles):
        super().__init__(cfg, n_steps, integ, circles)
        self.moving = []
        self.hits = []      # per MPC step: bool [N, circles, candidates]
        self.betas = []     # per MPC step: the candidates' beta
        self.states = []    # per MPC step: the candidates' states [N, 3, candidates]
        self.wrong = {k: [] for k in WRONG}   # per MPC step: (blocked, winner, mask)

    def circles_at(self, k):
        """The table with the displacement taken k times."""
        out = list(self.circles)
        if self.moving:
            mv = np.array(self.moving, dtype=np.float64)
            cx, cy = centres(mv[:, 0], mv[:, 2], k), centres(mv[:, 1], mv[:, 3], k)
            out += [(float(a), float(b), float(r)) for a, b, r in zip(cx, cy, mv[:, 4])]
        return out

    def _hits(self, states, mult):
        """bool [N, circles, candidates] and the smallest |distance - r|: the
        state after step j against the circles moved mult(j, N) times (the
        header's formula, a NaN state inside nothing)."""
        n = self.n_steps
        n_circ = len(self.circles) + len(self.moving)
        hit = np.zeros((n, n_circ, states.shape[2]), dtype=bool)
        margin = math.inf
        if not n_circ:
            return hit, margin
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(1, n + 1):
                x, y = states[j - 1, 0, :][None, :], states[j - 1, 1, :][None, :]
                cx, cy, r = (np.array(col)[:, None] for col in zip(*self.circles_at(mult(j, n))))
                d2 = (x - cx) ** 2 + (y - cy) ** 2
                hit[j - 1] = d2 < r * r
                gap = np.abs(np.sqrt(d2) - r)
                if not np.isnan(gap).all():
                    margin = min(margin, float(np.nanmin(gap)))
        return hit, margin

    def score(self, states, costs, v, b):
        n_grid = len(costs)
        self.states.append(states)
        self.betas.append(np.array(b[0], dtype=np.float64) if n_grid else np.zeros(0))
        if n_grid:
            hit, margin = self._hits(states, lambda j, n: j)
        else:
            hit, margin = np.zeros((self.n_steps, 0, 0), dtype=bool), math.inf
        mask, early = hit.any(axis=(0, 1)), hit[:-1].any(axis=(0, 1))
        for name, mult in WRONG.items():
            wm = self._hits(states, mult)[0].any(axis=(0, 1)) if n_grid else mask
            self.wrong[name].append((int(wm.sum()),
                                     RM.winner(states, np.where(wm, math.inf, costs), v, b).index,
                                     wm))
        self.hits.append(hit)
        return self.scored(states, costs, v, b, mask, early, margin)


class Fleet:
    """After the constructor: every robot as k_episodes_reset leaves it, the
    board's side 0 and a motion board of zeros.  call(): one fleet call, its
    neighbours' circles moving with them if `predict` (DeviceFleet(predict=))."""

    def __init__(self, cfgs, n_steps, integ, clearance, reach, static=(), predict=False):
        self.static = [tuple(float(v) for v in c) for c in static]
        self.keep = MPC_MAX_OBSTACLES - len(self.static)
        assert self.keep >= 0
        self.clearance, self.reach = float(clearance), float(reach)
        self.predict = bool(predict)
        robot = MotionRobotModel if self.predict else OM.ObstacleRobotModel
        self.models = [robot(c, n_steps, integ, self.static) for c in cfgs]
        self.recs = [[] for _ in cfgs]
        self.boards = [self.positions()]     # [c]: the positions at the start of call c
        self.motions = [[(0.0, 0.0)] * len(self.models)]     # [c]: what call c - 1 moved them by
        self.picks = []                      # per call, per robot: (within, chosen) or None
        self.edge = math.inf
        self.gap = math.inf

    def positions(self):
        return [(M.x, M.y) for M in self.models]

    def call(self, device):
        pos, mot = self.boards[-1], self.motions[-1]
        live = [(r, M) for r, M in enumerate(self.models) if not M.stop]
        row = [None] * len(self.models)
        if live:
            betas = np.unique(np.concatenate([np.array(M.grids()[1], dtype=np.float64)
                                              for _, M in live]))
            with harness.estimates_installed(betas, device) as misses:
                for r, M in live:
                    within, chosen, edge, gap = select(d2_row(pos, r), r, self.reach, self.keep)
                    self.edge, self.gap = min(self.edge, edge), min(self.gap, gap)
                    row[r] = (within, chosen)
                    if self.predict:
                        M.moving = [(*pos[q], *mot[q], self.clearance) for q in chosen]
                    else:
                        M.circles = self.static + [(*pos[q], self.clearance) for q in chosen]
                    self.recs[r].append(M.mpc_step())
                assert misses() == 0, "a denominator without its device estimate"
        self.picks.append(row)
        after = self.positions()
        self.boards.append(after)
        # a robot that goes on: one subtraction each; everyone else stands
        self.motions.append([(after[r][0] - pos[r][0], after[r][1] - pos[r][1])
                             if row[r] is not None and not M.stop else (0.0, 0.0)
                             for r, M in enumerate(self.models)])

    def run(self, n_calls, device):
        for _ in range(n_calls):
            self.call(device)
        return self

    @property
    def calls(self):
        return len(self.picks)

    def margin(self):
        """The smallest |distance - r| of any state and any circle, static or robot."""
        return min(M.margin for M in self.models)

    def neighbours(self, c=None):
        """neighbours_out after c fleet calls (None: all so far): int32 [R][17]
        of call c - 1."""
        c = self.calls if c is None else c
        out = np.full((len(self.models), ROW), -1, dtype=np.int32)
        out[:, 0] = 0
        for r, pick in enumerate(self.picks[c - 1] if c > 0 else ()):
            if pick is not None:
                out[r, 0] = pick[0]
                out[r, 1:1 + len(pick[1])] = pick[1]
        return out

    def board(self, c=None):
        """The board's bytes after c fleet calls (None: all so far): side c & 1
        holds the positions then, the other side those at the start of call
        c - 1 (after no call: side 0 the start positions, side 1 untouched
        zeros)."""
        return self._sides(self.boards, c)

    def motion(self, c=None):
        """The motion board's bytes after c predicted fleet calls (None: all so
        far), as board(c): side c & 1 holds what call c - 1 wrote, the other
        side what it read (side 0 zeroed before call 0)."""
        return self._sides(self.motions, c)

    def _sides(self, history, c):
        n = len(self.models)
        sides = [np.zeros((n, 2)), np.zeros((n, 2))]
        c = self.calls if c is None else c
        sides[c & 1] = np.array(history[c], dtype=np.float64).reshape(n, 2)
        if c > 0:
            sides[(c - 1) & 1] = np.array(history[c - 1], dtype=np.float64).reshape(n, 2)
        return np.concatenate(sides).tobytes()


def launch_counts(fleet, launches):
    """Per run(k) of `launches` the per-robot n_blocked_out: the blocked
    candidates of the steps that run's fleet calls made for the robot."""
    return OM.launch_counts(fleet.models, launches)


def expected(fleet, cfgs, cap, launches):
    """robots_model.expected for the fleet's robots."""
    case = dict(cfgs=cfgs, cap=cap, launches=launches)
    return RM.expected(case, fleet.models, fleet.recs)
