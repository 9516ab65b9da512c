"""A fleet of predicted fleet calls (mpc_episodes_fleet_run_predicted,
FleetMotionObs of csrc/mpc_episodes_fleet.h) restated on the host:
fleet_model.Fleet with a motion list beside `boards`, and robots whose `score`
masks the state after horizon step j with step j's circles only — the static
ones, unmoved, and each chosen neighbour's at (x_q + j * dx_q, y_q + j * dy_q),
the centres from the host build of the device's fleet_predict
(tests/fleet_motion_harness.cpp), so a last bit on the device is a last bit
here.

Beside what robots_obstacle_model keeps (margin — here over the moving rims —
blocked_steps, masks, free), a robot keeps per MPC step which (horizon step,
table entry) hits which candidate, the candidates' beta, and the blocked count,
winner and mask under each WRONG MULTIPLIER of the displacement: 0 (the circle
stands), j - 1, j + 1, N and 1.  A GPU test asserts on these that a kernel
which used any of them would have been caught.  Test infrastructure only."""
import ctypes
import math
import os

import numpy as np

import fleet_model as FM
import harness
import robots_model as RM
import robots_obstacle_model as OM

_P = ctypes.c_void_p
WRONG = {"0": lambda j, n: 0, "j-1": lambda j, n: j - 1, "j+1": lambda j, n: j + 1,
         "N": lambda j, n: n, "1": lambda j, n: 1}


def _lib():
    L = harness._build("fleet_motion_harness", ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17",
                                                "-ffp-contract=off", "-fPIC", "-shared",
                                                "--cuda-host-only", "-x", "hip", "-I",
                                                os.path.join(harness.REPO, "include")])
    L.fleet_predict_row.argtypes = [_P, _P, ctypes.c_int64, ctypes.c_int64, _P]
    L.fleet_predict_row.restype = None
    return L


def centres(x, d, j):
    """fleet_predict(x[q], d[q], j) for every q: the device function's host build."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    out = np.empty(len(x))
    _lib().fleet_predict_row(x.ctypes.data_as(_P), d.ctypes.data_as(_P), len(x), int(j),
                             out.ctypes.data_as(_P))
    return out


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
        self.poses.append((self.x, self.y))
        self.states.append(states)
        self.betas.append(np.array(b[0], dtype=np.float64) if n_grid else np.zeros(0))
        if n_grid:
            hit, margin = self._hits(states, lambda j, n: j)
            self.margin = min(self.margin, margin)
            mask = hit.any(axis=(0, 1))
            early = hit[:-1].any(axis=(0, 1))
        else:
            hit = np.zeros((self.n_steps, 0, 0), dtype=bool)
            mask = early = np.zeros(0, dtype=bool)
        for name, mult in WRONG.items():
            wm = self._hits(states, mult)[0].any(axis=(0, 1)) if n_grid else mask
            self.wrong[name].append((int(wm.sum()),
                                     RM.winner(states, np.where(wm, math.inf, costs), v, b).index,
                                     wm))
        self.hits.append(hit)
        self.free.append(RM.winner(states, costs, v, b).index)
        self.masks.append((mask, early))
        self.blocked_steps.append(int(mask.sum()))
        return np.where(mask, math.inf, costs)


class MotionFleet(FM.Fleet):
    """fleet_model.Fleet in lockstep with `motions` beside `boards`:
    motions[c][r] is robot r's entry of the motion board's in side of call c."""

    def __init__(self, cfgs, n_steps, integ, clearance, reach, static=()):
        super().__init__(cfgs, n_steps, integ, clearance, reach, static)
        self.models = [MotionRobotModel(c, n_steps, integ, self.static) for c in cfgs]
        self.boards = [self.positions()]
        self.motions = [[(0.0, 0.0)] * len(self.models)]

    def call(self, device):
        pos, mot = self.boards[-1], self.motions[-1]
        live = [(r, M) for r, M in enumerate(self.models) if not M.stop]
        row = [None] * len(self.models)
        if live:
            betas = np.unique(np.concatenate([np.array(M.grids()[1], dtype=np.float64)
                                              for _, M in live]))
            with harness.estimates_installed(betas, device) as misses:
                for r, M in live:
                    within, chosen, edge, gap = FM.select(FM.d2_row(pos, r), r, self.reach,
                                                          self.keep)
                    self.edge, self.gap = min(self.edge, edge), min(self.gap, gap)
                    row[r] = (within, chosen)
                    M.moving = [(pos[q][0], pos[q][1], mot[q][0], mot[q][1], self.clearance)
                                for q in chosen]
                    self.recs[r].append(M.mpc_step())
                assert misses() == 0, "a denominator without its device estimate"
        self.picks.append(row)
        after = self.positions()
        self.boards.append(after)
        # a robot that goes on: one subtraction each; everyone else stands
        self.motions.append([(after[r][0] - pos[r][0], after[r][1] - pos[r][1])
                             if row[r] is not None and not M.stop else (0.0, 0.0)
                             for r, M in enumerate(self.models)])

    def motion(self, c=None):
        """The motion board's bytes after c predicted fleet calls (None: all so
        far), as board(c): side c & 1 holds what call c - 1 wrote, the other
        side what it read (side 0 zeroed before call 0)."""
        n = len(self.models)
        sides = [np.zeros((n, 2)), np.zeros((n, 2))]
        c = self.calls if c is None else c
        sides[c & 1] = np.array(self.motions[c], dtype=np.float64).reshape(n, 2)
        if c > 0:
            sides[(c - 1) & 1] = np.array(self.motions[c - 1], dtype=np.float64).reshape(n, 2)
        return np.concatenate(sides).tobytes()
