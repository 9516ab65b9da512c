"""A fleet of planned fleet calls (mpc_episodes_fleet_run_planned,
FleetPlanObs of csrc/mpc_episodes_fleet.h) restated on the host:
fleet_model.Fleet with a plan board.  Every robot publishes two points
(a1, a2) of its plan on exit; a chosen neighbour's circle stands at a1 for
horizon step 1, at a2 for step 2 and at fleet_predict(a2, a2 - a1, j - 2) for
step j >= 3, per coordinate, through the host build of the device's function
(fleet_model.centres).

What a robot publishes after a call (PlanFleet.call): if it took a step in the
call, goes on after it and the step was not stale, the layers min(k + 1, 2) and
min(k + 2, 2) of its model's `ot` after the update, k the layer the update
returned (episode_model's trace: 0, or 1 / 2 while the robot finishes);
everyone else its position twice.  PlanRobotModel keeps (k, stale) per step.

Beside the true rule the model scores every step under WRONG rules, on the
true run's states (as MotionRobotModel does with its multipliers), and keeps
per step the blocked count, the winner and the mask of each:

  standing   the neighbour's circle where the pose board has it, every step
  moved      the constant displacement of predict=True: x_q + j * dx_q
  early      the plan one layer early: (ot[k], ot[min(k + 1, 2)]) published
  hold       a2 for every j >= 3
  j-1, j-3   the extrapolation's multiplier j - 1 and j - 3 for j - 2
  ot         a robot that stepped publishes its ot whether it goes on or not
             and whether its step was stale or not

A test asserts that a kernel which followed any of them would have been
caught.  Test infrastructure only."""
import math

import numpy as np

import fleet_model as FM
import harness
import robots_model as RM
from diplomjourney_amd.abi import MPC_EP_STALE

WRONG = ("standing", "moved", "early", "hold", "j-1", "j-3", "ot")


def stand(p):
    return (p[0], p[1], p[0], p[1])


def plan_centres(entries, j, mult=lambda j: j - 2, hold=False):
    """The step-j centres [(x, y)] of the neighbours whose plan board entries
    are `entries` [(x1, y1, x2, y2)]."""
    if not len(entries):
        return []
    a = np.array(entries, dtype=np.float64)
    if j == 1:
        return [(float(x), float(y)) for x, y in a[:, 0:2]]
    if j == 2 or hold:
        return [(float(x), float(y)) for x, y in a[:, 2:4]]
    cx = FM.centres(a[:, 2], a[:, 2] - a[:, 0], mult(j))
    cy = FM.centres(a[:, 3], a[:, 3] - a[:, 1], mult(j))
    return [(float(x), float(y)) for x, y in zip(cx, cy)]


class PlanRobotModel(FM.MotionRobotModel):
    """MotionRobotModel whose neighbours' circles come from plan board
    entries.  `near`, set per call: for the chosen neighbours, in order, their
    `pos` (x, y), `mot` (dx, dy), `plan`, `early` and `ot` entries (the true
    board's and the two wrong boards'), and the radius `r`."""

    def __init__(self, cfg, n_steps, integ, circles):
        super().__init__(cfg, n_steps, integ, circles)
        self.near = dict(pos=[], mot=[], plan=[], early=[], ot=[], r=0.0)
        self.wrong = {k: [] for k in WRONG}
        self.layers = []    # per MPC step: (the layer k the update returned, the step was stale)
        self.ots = []       # per MPC step: the (x, y) of ot's three layers after the update

    def rule_centres(self, rule, j):
        N = self.near
        if rule == "true":
            return plan_centres(N["plan"], j)
        if rule == "standing":
            return list(N["pos"])
        if rule == "moved":
            if not N["pos"]:
                return []
            p, d = np.array(N["pos"]), np.array(N["mot"])
            return list(zip(FM.centres(p[:, 0], d[:, 0], j).tolist(),
                            FM.centres(p[:, 1], d[:, 1], j).tolist()))
        if rule == "early":
            return plan_centres(N["early"], j)
        if rule == "ot":
            return plan_centres(N["ot"], j)
        if rule == "hold":
            return plan_centres(N["plan"], j, hold=True)
        return plan_centres(N["plan"], j, mult={"j-1": lambda j: j - 1, "j-3": lambda j: j - 3}[rule])

    def circles_of(self, rule, j):
        """Step j's table under `rule`: the static circles, then the neighbours'."""
        return list(self.circles) + [(x, y, self.near["r"]) for x, y in self.rule_centres(rule, j)]

    def _hits(self, states, rule):
        """bool [N, circles, candidates] and the smallest |distance - r|: the
        state after step j against step j's table under `rule` (the header's
        formula, a NaN state inside nothing)."""
        n = self.n_steps
        n_circ = len(self.circles) + len(self.near["plan"])
        hit = np.zeros((n, n_circ, states.shape[2]), dtype=bool)
        margin = math.inf
        if not n_circ:
            return hit, margin
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(1, n + 1):
                x, y = states[j - 1, 0, :][None, :], states[j - 1, 1, :][None, :]
                cx, cy, r = (np.array(col)[:, None] for col in zip(*self.circles_of(rule, j)))
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
            hit, margin = self._hits(states, "true")
        else:
            hit, margin = np.zeros((self.n_steps, 0, 0), dtype=bool), math.inf
        mask, early = hit.any(axis=(0, 1)), hit[:-1].any(axis=(0, 1))
        for name in WRONG:
            wm = self._hits(states, name)[0].any(axis=(0, 1)) if n_grid else mask
            self.wrong[name].append((int(wm.sum()),
                                     RM.winner(states, np.where(wm, math.inf, costs), v, b).index,
                                     wm))
        self.hits.append(hit)
        return self.scored(states, costs, v, b, mask, early, margin)

    def mpc_step(self):
        rec = super().mpc_step()
        if rec is not None:
            self.layers.append((int(self.trace["k"]), bool(rec["status"] & MPC_EP_STALE)))
            self.ots.append([(layer[0], layer[1]) for layer in self.ot])
        return rec

    def layer_points(self, first):
        """(ot[first], ot[first + 1]), clamped to layer 2: a plan board entry."""
        a, b = self.ot[min(first, 2)], self.ot[min(first + 1, 2)]
        return (a[0], a[1], b[0], b[1])


class PlanFleet(FM.Fleet):
    """After the constructor: every robot as k_episodes_reset leaves it, the
    pose board's side 0 and a plan board on which everybody stands.  call():
    one planned fleet call.  `plans[c]`: what call c reads (what call c - 1
    published); `plans_early`, `plans_ot`: the same under the wrong rules
    `early` and `ot`; `motions` as Fleet keeps them, for the wrong rule `moved`."""

    def __init__(self, cfgs, n_steps, integ, clearance, reach, static=()):
        super().__init__(cfgs, n_steps, integ, clearance, reach, static, predict=True)
        self.predict = "plan"
        self.models = [PlanRobotModel(c, n_steps, integ, self.static) for c in cfgs]
        standing = [stand(p) for p in self.boards[0]]
        self.plans, self.plans_early, self.plans_ot = [standing], [standing], [standing]

    def call(self, device):
        pos, mot = self.boards[-1], self.motions[-1]
        boards = dict(plan=self.plans[-1], early=self.plans_early[-1], ot=self.plans_ot[-1])
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
                    M.near = dict(pos=[pos[q] for q in chosen], mot=[mot[q] for q in chosen],
                                  r=self.clearance,
                                  **{k: [b[q] for q in chosen] for k, b in boards.items()})
                    self.recs[r].append(M.mpc_step())
                assert misses() == 0, "a denominator without its device estimate"
        self.picks.append(row)
        after = self.positions()
        self.boards.append(after)
        self.motions.append([(after[r][0] - pos[r][0], after[r][1] - pos[r][1])
                             if row[r] is not None and not M.stop else (0.0, 0.0)
                             for r, M in enumerate(self.models)])
        true, early, ot = [], [], []
        for r, M in enumerate(self.models):
            stepped = row[r] is not None
            k = M.layers[-1][0] if stepped else 0
            plans = stepped and not M.stop and not M.layers[-1][1]
            true.append(M.layer_points(k + 1) if plans else stand(after[r]))
            early.append(M.layer_points(k) if plans else stand(after[r]))
            ot.append(M.layer_points(k + 1) if stepped else stand(after[r]))
        self.plans.append(true)
        self.plans_early.append(early)
        self.plans_ot.append(ot)

    def motion(self, c=None):
        """A planned fleet has no motion board (robots_bench.fleet_against
        compares it with the launch's, which is None too)."""
        return None

    def plan(self, c=None):
        """The plan board's bytes after c >= 1 planned fleet calls (None: all so
        far): side c & 1 holds what call c - 1 published, the other side what
        it read (side 0 before call 0: everybody standing at the start)."""
        n = len(self.models)
        c = self.calls if c is None else c
        assert c >= 1, "before the first call the board is whatever the caller left in it"
        sides = [None, None]
        sides[c & 1] = np.array(self.plans[c], dtype=np.float64).reshape(n, 4)
        sides[(c - 1) & 1] = np.array(self.plans[c - 1], dtype=np.float64).reshape(n, 4)
        return np.concatenate(sides).tobytes()

    def separated(self, rules=WRONG):
        """Per wrong rule: (the steps whose blocked count differs from the true
        rule's, the steps whose winner differs)."""
        out = {}
        for name in rules:
            counts = sum(w[0] != n for M in self.models
                         for w, n in zip(M.wrong[name], M.blocked_steps))
            wins = sum(w[1] != rec["index"] for M, rr in zip(self.models, self.recs)
                       for w, rec in zip(M.wrong[name], rr))
            out[name] = (counts, wins)
        return out
