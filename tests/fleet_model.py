"""A fleet of the batched device episodes (mpc_episodes_fleet_run,
csrc/mpc_episodes_fleet.h) restated on the host: R
robots_obstacle_model.ObstacleRobotModels in lockstep.  Per fleet call a
snapshot of every robot's position is taken; each still-running robot's
circles become the static ones and one (x_q, y_q, clearance) per chosen
neighbour; then its mpc_step() runs.  Ended robots take no step, keep their
position and stay in the snapshot.

The neighbours are chosen by a brute-force restatement of the header's rule:
of the robots q != r with d2 < reach * reach the K = 16 - len(static) smallest
by (d2, q).  d2 is the host build of the device's fleet_d2
(tests/fleet_harness.cpp: numpy has no fused multiply-add), so a tie on the
device is a tie here.

The fleet keeps, beside what the robots' models keep (the blocked count per
step, the margin between any state and any rim): per call and robot the
(within reach, chosen) pair, the smallest |sqrt(d2) - reach| over every pair a
running robot looked at, and the smallest d2 gap between the K-th and the
(K+1)-th neighbour of a capped selection.  A GPU test asserts these margins
before it looks at a kernel, unless exact ties are what it is about.  Test
infrastructure only."""
import ctypes
import math
import os

import numpy as np

import harness
import robots_model as RM
import robots_obstacle_model as OM
from diplomjourney_amd.abi import MPC_MAX_OBSTACLES

_P = ctypes.c_void_p
CAP_GAP = 1e-12          # the d2 gap a capped selection must have at its boundary
ROW = 1 + MPC_MAX_OBSTACLES


def _lib():
    L = harness._build("fleet_harness", ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17",
                                         "-ffp-contract=off", "-fPIC", "-shared",
                                         "--cuda-host-only", "-x", "hip", "-I",
                                         os.path.join(harness.REPO, "include")])
    L.fleet_d2_row.argtypes = [_P, _P, ctypes.c_int64, ctypes.c_int64, _P]
    L.fleet_d2_row.restype = None
    return L


def d2_row(pos, r):
    """fleet_d2(robot r, robot q) for every q: the device function's host build."""
    x = np.ascontiguousarray([p[0] for p in pos], dtype=np.float64)
    y = np.ascontiguousarray([p[1] for p in pos], dtype=np.float64)
    out = np.empty(len(pos))
    _lib().fleet_d2_row(x.ctypes.data_as(_P), y.ctypes.data_as(_P), len(pos), int(r),
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


class Fleet:
    """After the constructor: every robot as k_episodes_reset leaves it and the
    board's side 0.  call(): one fleet call."""

    def __init__(self, cfgs, n_steps, integ, clearance, reach, static=()):
        self.static = [tuple(float(v) for v in c) for c in static]
        self.keep = MPC_MAX_OBSTACLES - len(self.static)
        assert self.keep >= 0
        self.clearance, self.reach = float(clearance), float(reach)
        self.models = [OM.ObstacleRobotModel(c, n_steps, integ, self.static) for c in cfgs]
        self.recs = [[] for _ in cfgs]
        self.boards = [self.positions()]     # [c]: the positions at the start of call c
        self.picks = []                      # per call, per robot: (within, chosen) or None
        self.edge = math.inf
        self.gap = math.inf

    def positions(self):
        return [(M.x, M.y) for M in self.models]

    def call(self, device):
        pos = self.boards[-1]
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
                    M.circles = self.static + [(pos[q][0], pos[q][1], self.clearance)
                                               for q in chosen]
                    self.recs[r].append(M.mpc_step())
                assert misses() == 0, "a denominator without its device estimate"
        self.picks.append(row)
        self.boards.append(self.positions())

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
        n = len(self.models)
        sides = [np.zeros((n, 2)), np.zeros((n, 2))]
        c = self.calls if c is None else c
        sides[c & 1] = np.array(self.boards[c], dtype=np.float64).reshape(n, 2)
        if c > 0:
            sides[(c - 1) & 1] = np.array(self.boards[c - 1], dtype=np.float64).reshape(n, 2)
        return np.concatenate(sides).tobytes()


def launch_counts(fleet, launches):
    """Per run(k) of `launches` the per-robot n_blocked_out: the blocked
    candidates of the steps that run's fleet calls made for the robot."""
    return OM.launch_counts(fleet.models, launches)


def expected(fleet, cfgs, cap, launches):
    """robots_model.expected for the fleet's robots."""
    case = dict(cfgs=cfgs, cap=cap, launches=launches)
    return RM.expected(case, fleet.models, fleet.recs)
