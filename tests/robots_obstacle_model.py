"""One robot of the batched device episodes with keep-out circles
(k_episodes_run with an obstacle hook, csrc/mpc_episodes.h) restated on the
host: robots_model.RobotModel with its `score` step overridden.  The step's
states are the replica's; the mask is ranking.blocked of them (the header's formula
in world coordinates: any step-end state 1..N strictly inside any circle, a
NaN state inside nothing); blocked costs become +inf, and robots_model.winner
and the update run unchanged, so an all-blocked step is the step without a
finite cost.  The model sums the mask into the robot's blocked count, step by
step, and keeps the smallest |distance - r| over every state of every
candidate of every step: a test asserts that it exceeds ranking.MARGIN before
it looks at a kernel, and the mask then depends neither on last bits nor on
the rect+cum frame rotation.  `fillers`: circles that must block nothing
(asserted per step, their margin kept too), so that runs with different
numbers of them share one model run.  Test infrastructure only."""
import math

import numpy as np

import ranking
import robots_model as RM


class ObstacleRobotModel(RM.RobotModel):
    def __init__(self, cfg, n_steps, integ, circles, fillers=()):
        super().__init__(cfg, n_steps, integ)
        self.circles, self.fillers = list(circles), list(fillers)
        self.margin = math.inf
        self.blocked_steps = []   # per step: blocked candidates
        self.masks = []           # per step: (mask, mask of the states before the last alone)
        self.free = []            # per step: the winner without circles (index; -1: none)
        self.poses = []           # per step: the pose it started from

    def score(self, states, costs, v, b):
        """The blocked candidates' costs +inf (RobotModel.mpc_step calls this
        between the rollout and the winner, before the pose moves)."""
        n_grid = len(costs)
        mask = early = np.zeros(0, dtype=bool)
        margin = math.inf
        if n_grid:
            mask, margin = ranking.blocked(states, self.circles)
            early = (ranking.blocked(states[:-1], self.circles)[0] if self.n_steps > 1
                     else np.zeros(n_grid, dtype=bool))
            if self.fillers:
                none, far = ranking.blocked(states, self.fillers)
                assert not none.any(), "a filler circle blocks a candidate"
                margin = min(margin, far)
        return self.scored(states, costs, v, b, mask, early, margin)

    def scored(self, states, costs, v, b, mask, early, margin):
        """The bookkeeping of a scored step, whatever formed its masks (`mask`:
        the blocked candidates, `early`: those blocked before the last state
        alone, `margin`: the step's smallest |distance - r|); the blocked
        candidates' costs +inf."""
        self.poses.append((self.x, self.y))
        if margin == margin:                      # (NaN: no finite state at all)
            self.margin = min(self.margin, margin)
        self.free.append(RM.winner(states, costs, v, b).index)
        self.masks.append((mask, early))
        self.blocked_steps.append(int(mask.sum()))
        return np.where(mask, math.inf, costs)

    def blocked_in(self, first, last):
        """The blocked candidates of steps [first, last)."""
        return sum(self.blocked_steps[first:last])


def run(cfgs, n_steps, integ, max_calls, circles, fillers=(), device=False):
    """robots_model.run with ObstacleRobotModel (one table for all robots).
    Returns (models, records per robot, first-step (costs, Result) per robot)."""
    return RM.run(cfgs, n_steps, integ, max_calls, device=device,
                  model=lambda c, n, i: ObstacleRobotModel(c, n, i, circles, fillers))


def launch_counts(models, launches):
    """Per launch the per-robot n_blocked_out the entry must write: the blocked
    candidates of the steps that launch ran for the robot."""
    out, done = [], [0] * len(models)
    for k in launches:
        row = []
        for r, M in enumerate(models):
            upto = min(done[r] + k, M.calls)
            row.append(M.blocked_in(done[r], upto))
            done[r] = upto
        out.append(np.array(row, dtype=np.int64))
    return out
