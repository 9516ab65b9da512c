"""The case table of the directly driven episode update (mpc_episode_advance,
tests/test_episode_update_gpu.py layer 1): every case is a cfg, a model-made
self-consistent EpisodeState, fabricated mpc_result_t rows and a log ring.

The table is the full product of (m, winner, has_traj, n_steps) repeated REPS
times; in each repetition the other axes (layer-2 probe, stuck rule and pose,
event, heading, end, restart incumbent, log ring, wheelbase) are drawn from a
fixed-seed generator, so that every value of every axis meets every core
combination often.  What a case then DOES — its status bits, sector, layer,
m transition, restart cause — is decided by the model alone
(tests/episode_model.py); coverage() counts it, and
tests/test_episode_model_cpu.py requires every outcome at least 8 times before
any GPU is involved.  Test infrastructure only."""
import functools
import itertools
import math

import numpy as np

import harness
from diplomjourney_amd.episode import reference_episode_config
from episode_model import EpisodeModel, Result
from oracle import parity as P

EPS = 0.25                 # squares of the probe offsets below are exact against it
REPS = 13
POISON = -7.0e77           # layers at or past n_steps: never read by the update
PI = math.pi

M_VALUES = (0, 1, 2)
N_STEPS = (1, 2, 3, 10)
HAS_TRAJ = (0, 1)
WINNERS = ("found1", "last_of_2", "last_of_3", "last_of_4", "tie_by_index", "lower_cost_no_index",
           "zero_cost_tie", "nan_beside_found", "eq_incumbent", "all_nan", "inf", "no_index")
PROBES = ("far", "inside", "exact", "above")
STUCK = ("moved", "repeat", "x_only", "neg_zero")
RULES = ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2))          # (stop_rule, recursive)
EVENTS = ("none", "right", "left", "new", "right+left", "left+new", "right+new", "all",
          "disabled")
HEADINGS = (("s0", 2.0), ("s1", 4.0), ("s2", 5.5), ("s3", 7.0), ("pi/2", PI / 2), ("pi", PI),
            ("3pi/2", 3 * PI / 2), ("2pi", 2 * PI), ("negative", -0.75), ("small", 0.5))
ENDS = ("none", "arrived", "limit", "both")
RESTARTS = ("given", "origin")
LOGS = ("cap1", "cap3", "null", "cap0")
WHEELBASES = (0.5, 0.45)
FOUND_WINNERS = WINNERS[:8]


def _rows(kind, n_steps, incumbent, win_traj, rng):
    """(results, number of the winning row or None) of one winner case.  Losing
    rows carry other horizons and poses, so taking a field from the wrong row
    shows."""
    def lose(cost, index):
        ns = int(rng.choice(N_STEPS))
        return Result(cost, index, ns, 0.9, -0.3,
                      [[100.0 + index, 200.0 + k, 3.0] for k in range(min(ns, 3))])

    def win(cost, index):
        return Result(cost, index, n_steps, 0.45, 0.125, win_traj)

    if kind == "found1":
        return [win(10.0, 17)], 0
    if kind in ("last_of_2", "last_of_3", "last_of_4"):
        n = int(kind[-1])
        return [lose(20.0 + r, r) for r in range(n - 1)] + [win(10.0, 1000 + n)], n - 1
    if kind == "tie_by_index":
        return [lose(10.0, 7), win(10.0, 3), lose(20.0, 1)], 1
    if kind == "lower_cost_no_index":        # index < 0 never wins, whatever its cost
        return [lose(1.0, -1), win(10.0, 5)], 1
    if kind == "zero_cost_tie":
        return [lose(0.0, 9), win(0.0, 8)], 1
    if kind == "nan_beside_found":
        return [lose(math.nan, 0), win(10.0, 4), lose(math.inf, 1)], 1
    if kind == "eq_incumbent":               # strict <: not found
        return [lose(incumbent + 5.0, 2), win(incumbent, 6)], None
    if kind == "all_nan":
        return [lose(math.nan, 4), win(math.nan, 2)], None
    if kind == "inf":
        return [win(math.inf, 0)], None
    if kind == "no_index":
        return [win(5.0, -1), lose(3.0, -1), lose(math.inf, -1)], None
    raise ValueError(kind)


def build_case(m, winner, has_traj, n_steps, rng):
    probe = PROBES[rng.integers(len(PROBES))]
    stuck = STUCK[rng.integers(len(STUCK))]
    stop_rule, recursive = RULES[rng.integers(len(RULES))]
    event = EVENTS[rng.integers(len(EVENTS))]
    hname, heading = HEADINGS[rng.integers(len(HEADINGS))]
    end = ENDS[rng.integers(len(ENDS))]
    restart = RESTARTS[rng.integers(len(RESTARTS))]
    logk = LOGS[rng.integers(len(LOGS))]
    L = WHEELBASES[rng.integers(len(WHEELBASES))]
    coords = dict(m=m, winner=winner, has_traj=has_traj, n_steps=n_steps, probe=probe,
                  stuck=stuck, stop_rule=stop_rule, recursive=recursive, event=event,
                  heading=hname, end=end, restart=restart, log=logk, L=L)
    p = 7
    fires = event not in ("none", "disabled")
    arrive = end in ("arrived", "both")

    # geometry, all binary fractions: R the returned pose, T the target the
    # probe sees (before an event), E what an event makes the target
    rx = -0.0 if stuck == "neg_zero" else 1.5
    ry = 2.25
    near, far = (0.25, -0.25), (3.0, 1.0)
    # with an event the old target is the opposite of the new one, so an arrival
    # test against the wrong target shows
    off_t = (far if arrive else near) if fires else (near if arrive else far)
    T = (rx + off_t[0], ry + off_t[1])
    off_e = near if arrive else far
    probe_off = {"far": (4.0, 4.0), "inside": (0.25, 0.25), "exact": (0.5, 0.0),
                 "above": (0.5, 0.0)}[probe]
    Q = [T[0] - probe_off[0], T[1] - probe_off[1]]
    while probe == "above" and T[0] - Q[0] <= 0.5:  # the first pose whose offset exceeds 0.5
        Q[0] = math.nextafter(Q[0], -math.inf)
    k_ret = m                                        # the finishing layer of this m

    def layers(n):
        """n layer states whose clamped layer k_ret is R and whose clamped
        layer 2 (when another one) is Q; every other layer is somewhere else."""
        out = [[10.0 + k, 20.0 + k, heading + 1.0] for k in range(n)]
        if min(2, n - 1) != min(k_ret, n - 1):
            out[min(2, n - 1)] = [Q[0], Q[1], heading + 1.0]
        out[min(k_ret, n - 1)] = [rx, ry, heading]
        return out

    cfg = reference_episode_config(start=(0.5, -1.0, 0.3, 0.2, 0.1), target=(2.0, 3.0),
                                   seed=20261015 + int(rng.integers(1000)),
                                   incumbent0=12345.5 if restart == "given" else 0.0)
    cfg.eps, cfg.L, cfg.stop_rule = EPS, L, stop_rule
    # no limit: none set, or one the step just does not pass (p + 1 > max_steps is false)
    cfg.max_steps = p if end in ("limit", "both") else int(rng.choice((0, p + 1, p + 5)))
    cfg.p_turn_right = p if event in ("right", "right+left", "right+new", "all") else 60
    cfg.p_turn_left = p if event in ("left", "right+left", "left+new", "all") else 90
    cfg.p_new_target = p if event in ("new", "left+new", "right+new", "all") else 110
    if event == "disabled":
        cfg.p_turn_right, cfg.p_turn_left, cfg.p_new_target = 0, -3, 0
    cfg.event_target_x, cfg.event_target_y = rx + off_e[0], ry + off_e[1]
    if arrive:                      # a U-turn target within eps of the pose
        cfg.turn_distance, cfg.radius_u_turn = 0.25, 0.25
    cfg.slow_turn, cfg.slow_new_target = 20, 10

    M = EpisodeModel(cfg)
    M.m, M.has_traj, M.recursive, M.p = m, has_traj, recursive, p
    M.episodes = int(rng.choice((1, 3)))
    M.step = {"cap1": 9, "cap3": int(rng.choice((4, 5, 3000000000))), "null": 2,
              "cap0": 6}[logk]
    M.slowing = int(rng.choice((0, 1, 5)))
    M.incumbent = 1000.0
    M.xt, M.yt = T
    M.phi, M.v, M.beta = heading, 0.3, -0.0625
    stale = layers(3)
    applied_is_pose = winner not in FOUND_WINNERS and not has_traj
    if stuck in ("repeat", "neg_zero"):
        M.x, M.y = (0.0 if stuck == "neg_zero" else rx), ry
    elif stuck == "x_only":
        M.x, M.y = rx, ry - 1.0
    else:
        M.x, M.y = rx - 1.0, ry - 1.0
    if applied_is_pose:             # the pose itself is returned: let it be R
        M.x, M.y = rx, ry
    M.x0, M.y0 = M.x - 2.0, M.y - 3.0
    if has_traj:
        M.ot, M.ot_v, M.ot_beta = stale, 0.625, -0.1875
    M.t = 0.0
    for _ in range(p - 1):
        M.t = M.t + cfg.delta_t
    M.prepare()                     # t, K and seed as episode_prepare leaves them
    M.early = M.early_prepare()
    M.nv, M.nb = 3, 5
    M.grid_v = [0.125 * i for i in range(64)]
    M.grid_b = [-0.5 + 0.015625 * i for i in range(64)]
    M.done, M.chain_error, M.p2p_seq, M.gathered_tag = 3, 0, 5, 0x1234567800000009
    M.chain_pub = [((0xABC00000 + i) << 32) | 77 for i in range(len(M.chain_pub))]

    win_traj = layers(n_steps)[:3]
    results, _ = _rows(winner, n_steps, M.incumbent, win_traj, rng)
    cap = {"cap1": 1, "cap3": 3, "null": 3, "cap0": 0}[logk]
    return dict(coords=coords, cfg=cfg, model=M, results=results, cap=cap,
                log_null=logk == "null")


def case_table():
    """[case]: the (m, winner, has_traj, n_steps) product, REPS times."""
    rng = np.random.default_rng(20261020)
    core = list(itertools.product(M_VALUES, WINNERS, HAS_TRAJ, N_STEPS))
    return [build_case(*c, rng) for _ in range(REPS) for c in core]


def run_model(case):
    """The model's update of one case: (post-state model, log record, trace).
    The case's own model is left as it is (the pre-state)."""
    import copy
    M = copy.copy(case["model"])
    M.ot = [list(r) for r in M.ot]
    M.grid_v, M.grid_b, M.chain_pub = list(M.grid_v), list(M.grid_b), list(M.chain_pub)
    rec = M.advance(case["results"])
    return M, rec, M.trace


def coverage(table):
    """Counts of what the model does over the table, by kind of outcome."""
    from collections import Counter
    cov = {k: Counter() for k in ("status", "bit", "sector", "layer", "m_transition", "restart",
                                  "m_found_traj", "log_slot")}
    for case in table:
        M, rec, tr = run_model(case)
        cov["status"][tr["status"]] += 1
        for bit in (P.STALE, P.STUCK, P.BREAK, P.EVENT, P.ARRIVED, P.LIMIT):
            if tr["status"] & bit:
                cov["bit"][bit] += 1
        for s in tr.get("sectors", ()):
            cov["sector"][s] += 1
        cov["layer"][tr["k"]] += 1
        cov["m_transition"][(tr["m0"], tr["m1"])] += 1
        if tr["ended"]:
            cov["restart"][tr["ended"]] += 1
        cov["m_found_traj"][(tr["m0"], tr["found"], tr["had_traj"])] += 1
        cov["log_slot"][(case["coords"]["log"], rec["step"] % case["cap"] if case["cap"] else
                         None)] += 1
    return cov


def possible_statuses():
    """Every status word episode_advance can produce: STALE or not, times a
    break (BREAK alone under math_mpc's rule, STUCK|BREAK under the script's)
    or [STUCK] [EVENT] [ARRIVED or LIMIT]."""
    tails = [P.BREAK, P.STUCK | P.BREAK]
    for stuck, event, end in itertools.product((0, P.STUCK), (0, P.EVENT),
                                               (0, P.ARRIVED, P.LIMIT)):
        tails.append(stuck | event | end)
    return sorted({s | t for s in (0, P.STALE) for t in tails})


# ----------------------------------------------------------------------------
# layer 3: episodes steered by the cfg alone, from reset()
# ----------------------------------------------------------------------------
STEERED_STEPS = 6
STEERED_N_CAND = 1026      # ranking.N_CAND: two full tiles plus one lane pair


def steered_cfgs():
    """[(name, cfg, n_steps)]: about ten episodes whose cfg alone walks the
    update's branches within STEERED_STEPS steps of a reset."""
    def make(start, target, n_steps, **mods):
        inc0 = mods.pop("incumbent0", 0.0)
        cfg = reference_episode_config(start=start, target=target, incumbent0=inc0)
        cfg.p_turn_right = cfg.p_turn_left = cfg.p_new_target = 0
        for k, v in mods.items():
            setattr(cfg, k, v)
        return cfg, n_steps

    ahead = (0.1 * math.cos(0.6), 0.1 * math.sin(0.6))     # two steps ahead of heading 0.6
    out = [
        # the three events at once, one heading per sector of turn_target
        ("events, sector 0", *make((0.0, 0.0, 2.0, 0.5, 0.0), (-1.0, 3.0), 3,
                                   p_turn_right=1, p_turn_left=2, p_new_target=3)),
        ("events, sector 1, L 0.45", *make((1.0, -2.0, 4.0, 0.5, 0.1), (-2.0, -3.0), 10, L=0.45,
                                           p_turn_right=1, p_turn_left=2, p_new_target=3)),
        ("events, sector 2", *make((0.5, 0.5, 5.5, 0.3, -0.1), (3.0, -2.0), 2,
                                   p_turn_left=1, p_turn_right=2, p_new_target=3)),
        ("two events on p = 1, sector 3", *make((0.0, 0.0, 7.0, 0.5, 0.0), (2.0, 2.0), 3,
                                                p_turn_left=1, p_new_target=1, p_turn_right=2)),
        # m walks 0 -> 1 -> 2 and the episode arrives
        ("arrival", *make((0.0, 0.0, 0.6, 0.5, 0.0), ahead, 3, eps=0.004)),
        ("arrival, horizon 10, L 0.45", *make((0.0, 0.0, 0.6, 0.5, 0.0), ahead, 10, eps=0.004,
                                              L=0.45)),
        # a stale first step without trajectory (stuck), a break, then a stale
        # step WITH the trajectory that carried over the restart
        ("stale without, then with a trajectory", *make((0.0, 0.0, 0.3, 0.4, 0.0), (2.0, 3.0), 3,
                                                        incumbent0=1.0)),
        # the target behind the robot: it stops, is stuck, and breaks
        ("stuck then break", *make((0.0, 0.0, 0.0, 0.0, 0.0), (-2.0, 0.0), 3)),
        ("stuck then break, the script's rule", *make((0.0, 0.0, 0.0, 0.0, 0.0), (-2.0, 0.0), 2,
                                                      stop_rule=1)),
        ("step limit 2", *make((0.0, 0.0, 1.0, 0.5, 0.0), (2.0, 3.0), 10, max_steps=2, L=0.45,
                               p_turn_right=2)),
    ]
    return [(name, cfg, ns) for name, cfg, ns in out]


@functools.lru_cache(maxsize=None)
def steered_batch(n_steps, j):
    """Step j's fixed candidates of a horizon (every form but the generated
    one): seeded uniform controls; candidate 0 stands still."""
    rng = np.random.default_rng(7000 + 100 * n_steps + j)
    v = rng.uniform(0.0, 1.0, (n_steps, STEERED_N_CAND))
    b = rng.uniform(-0.6, 0.6, (n_steps, STEERED_N_CAND))
    v[:, 0] = b[:, 0] = 0.0
    return v, b


def best_row(states, costs, v, b, index=None):
    """The Result of candidate `index` of a replica rollout (None: of its
    lexicographic (cost, index) minimum over the finite costs)."""
    n_steps = v.shape[0]
    if index is None:
        ok = np.flatnonzero(costs < math.inf)
        if not len(ok):
            return Result(math.inf, -1, n_steps, 0.0, 0.0, [[0.0] * 3] * min(n_steps, 3))
        index = int(ok[np.lexsort((ok, costs[ok]))[0]])
    return Result(float(costs[index]), int(index), n_steps, float(v[0, index]),
                  float(b[0, index]),
                  [[float(states[s, q, index]) for q in range(3)] for s in range(min(n_steps, 3))])


def walk(cfg, n_steps, integ, generated, logged=None, early_after=(), oracle=None):
    """STEERED_STEPS steps of the model from reset: per step the model's
    problem, the host replica's rollout of the step's batch (the device's
    reciprocal estimates when a device log is given, the host's quotient in a
    dry run) and the model's update with the winner's row — the logged index
    when the log says found, the replica's minimum otherwise.  early_after:
    the steps after whose update the form writes the early-publication record.
    Returns (model, records, traces, replica costs of the rows)."""
    M = EpisodeModel(cfg)
    recs, traces, costs_of = [], [], []
    for j in range(STEERED_STEPS):
        if generated:
            V, B, seed = M.sample()
            v, b = oracle.sample_controls(V, B, STEERED_N_CAND, n_steps, seed, index_base=0)
        else:
            v, b = steered_batch(n_steps, j)
        prob, _ = M.begin_step()
        states, costs = harness.replica_rollout(prob, v, b, integ,
                                                device_estimates=logged is not None,
                                                device_consts=True)
        index = None
        if logged is not None and logged[j].found and 0 <= logged[j].index < STEERED_N_CAND:
            index = logged[j].index
        row = best_row(states, costs, v, b, index)
        recs.append(M.advance([row]))
        traces.append(M.trace)
        costs_of.append(row.cost)
        if j in early_after:
            M.early = M.early_prepare()
    return M, recs, traces, costs_of
