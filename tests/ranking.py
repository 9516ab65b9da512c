"""Candidate ranking by peeling (tests/test_ranking_gpu.py, test_ranking_cpu.py).

An arg-min launch reports one candidate.  Launching again after the winner's
step-0 speed has been overwritten with NaN (a NaN cost never wins,
include/mpc_rollout.h) reports the next one, and so on until the result is
index -1, found 0: the sequence of winners is the kernel's complete ordering of
its candidates by (cost, index).  It must equal the host replica's costs sorted
by (cost, index) element for element, `==` on the doubles: one wrong cost,
index, tie or mask bit anywhere in the launch changes the sequence, and the
first mismatch names the candidate, hence its tile, wave, lane and pair slot.

peel() is the driver (public ABI and production binaries only, no host
synchronisation per peel), check_ranking() the comparison, controls() the fixed
seeded input of a horizon, check_preconditions() what is asserted of the
replica's numbers before a kernel is looked at.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from diplomjourney_amd.abi import MPC_TILE, RESULT_BYTES, make_problem

N_CAND = 1026          # two full 512-candidate tiles plus one lane pair
HORIZONS = (1, 2, 3, 4, 7, 32)
# start pose (x, y, phi, v, beta) and target of every ranked problem: the target
# lies 4 m ahead, slightly left of the heading, so that progress ranks a candidate
START = (0.2, -0.1, 0.7, 0.5, 0.0)
TARGET = (2.7, 3.0)
SEED = 100             # + n_steps; a seed that misses a precondition is replaced
RESULT_WORDS = RESULT_BYTES // 8
# words of one mpc_result_t that a peel records: cost, index, found | n_steps << 32,
# v, beta, traj[0] = (x, y, phi)
REC_WORDS = 8


def where(c):
    """Where candidate c runs in the streaming kernels (512-candidate tiles of
    four waves, two candidates per lane)."""
    c = int(c)
    if c < 0:
        return "no candidate"
    return (f"candidate {c}: tile {c // MPC_TILE}, wave {(c % MPC_TILE) // 128}, "
            f"lane {(c % 128) // 2}, pair slot {c % 2}")


# ----------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------
def result_words(buf, n=1):
    """[n, REC_WORDS] int64 view of the leading words of n mpc_result_t."""
    return buf.view(torch.int64).view(n, RESULT_WORDS)[:, :REC_WORDS]


def soa_offset(ld=0):
    """Flat offset of candidate c's step-0 v in an SoA tensor [N, C]: c itself;
    robot r of a batched [N, R * ld] tensor: r * ld + c."""
    def off(c):
        if ld:
            return c + ld * torch.arange(c.numel(), device=c.device)
        return c
    return off


def tiled_offset(n_steps):
    """The same in a tiled tensor (mpc_tiled_index at s = 0)."""
    def off(c):
        return (c // MPC_TILE) * (2 * MPC_TILE * n_steps) + c % MPC_TILE
    return off


def peel(launch, v, offset, n_peels):
    """launch() enqueues the kernel under test and returns an int64 tensor
    [R, W] (R problems; word 0 the winner's cost bits, word 1 its index, the
    rest whatever the case wants logged) on v's device.  After every launch the
    winner's step-0 v in `v` (any layout: offset(index tensor) -> flat offsets)
    is overwritten with NaN, an index of -1 leaving the tensor as it is.
    Nothing synchronises: the records go to a device log that is copied once.
    Returns the log, numpy int64 [n_peels, R, W]."""
    flat = v.view(-1)
    nan = torch.full((), math.nan, dtype=torch.float64, device=flat.device)
    log = None
    for i in range(n_peels):
        rec = launch()
        if log is None:
            log = torch.zeros((n_peels,) + tuple(rec.shape), dtype=torch.int64,
                              device=rec.device)
        log[i].copy_(rec)
        idx = rec[:, 1]
        ok = idx >= 0
        at = offset(torch.where(ok, idx, torch.zeros_like(idx)))
        ok = ok & (at < flat.numel())        # a wild index is logged, never written through
        at = torch.where(ok, at, torch.zeros_like(at))
        flat[at] = torch.where(ok, nan, flat[at])
    return log.cpu().numpy()


def _f64(words):
    return np.ascontiguousarray(words).view(np.float64)


def expected_order(costs, excluded=None):
    """Indices of the candidates with a finite cost (and not excluded), sorted
    by (cost, index)."""
    costs = np.asarray(costs)
    order = np.lexsort((np.arange(len(costs)), costs))
    keep = np.isfinite(costs)
    if excluded is not None:
        keep &= ~excluded
    return order[keep[order]]


def check_ranking(got, costs, excluded=None, states=None, top=None, what=""):
    """got: one problem's peel log [n_peels, W >= 3] (W >= 8 with states: words
    5..7 the winner's first state).  The peeled sequence must be
    expected_order() with bitwise-equal costs, every entry found, then index
    -1 / found 0 to the end of the log, which must hold at least one such
    record.  top: compare the first `top` only (no end-of-sequence check).
    Returns the number of ranked candidates."""
    order = expected_order(costs, excluded)
    n = len(order) if top is None else top
    assert top is None or len(order) >= top
    assert len(got) >= n + (top is None), f"{what}: {len(got)} peels for {n} candidates"
    g_idx, g_cost = got[:, 1], _f64(got[:, 0])
    g_found = got[:, 2] & 0xFFFFFFFF
    want_idx, want_cost = order[:n], np.asarray(costs)[order[:n]]
    bad = (g_idx[:n] != want_idx) | ~(g_cost[:n] == want_cost) | (g_found[:n] != 1)
    if bad.any():
        k = int(np.argmax(bad))
        c = int(want_idx[k])
        raise AssertionError(
            f"{what}: rank {k} of {n}: expected {where(c)} cost {want_cost[k]!r}; the kernel "
            f"reported {where(g_idx[k])} cost {g_cost[k]!r} found {g_found[k]} "
            f"({int(bad.sum())} of {n} ranks differ)")
    if states is not None:
        first = np.stack([_f64(got[:n, 5 + k]) for k in range(3)], axis=1)   # [n, 3]
        want = states[0][:, want_idx].T
        diff = ~(first == want).all(axis=1)
        if diff.any():
            k = int(np.argmax(diff))
            raise AssertionError(f"{what}: rank {k}: the reported first state of "
                                 f"{where(want_idx[k])} is {first[k]!r}, the replica's {want[k]!r}")
    if top is None:
        tail = (g_idx[n:] != -1) | (g_found[n:] != 0)
        if tail.any():
            k = n + int(np.argmax(tail))
            raise AssertionError(f"{what}: after the {n} finite candidates the kernel reported "
                                 f"{where(g_idx[k])} cost {g_cost[k]!r} found {g_found[k]}")
    return n


# ----------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------
def problem(L, pose=START[:3], t_a=0.05, t_b=0.05 + 0.05):
    """The ranked problem: an episode's first step from START (t = delta_t)."""
    return make_problem(pose[0], pose[1], pose[2], TARGET[0], TARGET[1], START[0], START[1], L,
                        t_a, t_b)


def grid_batch(n, n_steps, seed):
    """Reference-grid controls drawn as tests/test_replica.py's _case draws them."""
    from oracle import oracle as O
    from diplomjourney_amd import math_model_tree as mmt
    V = mmt.vector_of_velocities(0.5)
    B = mmt.vector_of_beta_angles(0.0)
    return O.sample_controls(V, B, n, n_steps, seed)


@functools.lru_cache(maxsize=None)
def controls(n_steps, n=N_CAND):
    """The fixed input of a horizon (read-only arrays): grid controls, then
    * every column whose whole control sequence repeats an earlier column's gets
      an off-grid step-0 speed of its own (the grid has 451 entries: at N = 1
      most of 1026 draws repeat one), so that costs tie only where meant to;
    * irregular candidates (|beta| > 1.1, |dphi| > 0.2): four with |beta| in
      (1.1, 1.25) at some step, two with a speed that makes |dphi| > 0.2, two
      with a steering angle around 1e8.  One sits in tile 2 (the last tile's
      only pair, or only candidate for n = 1025), one is the second candidate
      of a pair whose first is regular, several sit in tile 1.  Candidate 1024
      (|beta| = 1.15 at step 0) also drives faster than any grid candidate, so
      it ranks near the top in every mode;
    * two candidates with a NaN steering angle and one with v = +inf;
    * three pairs of exact duplicates (dst := src): within one lane pair,
      across two waves of a tile, across two tiles."""
    N, last = n_steps, n_steps - 1
    v, b = grid_batch(n, N, SEED + N)
    seen = set()
    for c in range(n):
        key = v[:, c].tobytes() + b[:, c].tobytes()
        if key in seen:
            v[0, c] = 0.476 + 0.048 * (c + 0.37) / n
            key = v[:, c].tobytes() + b[:, c].tobytes()
        seen.add(key)
    odd = 1025 if n > 1025 else 1023          # second of a pair whose first is regular
    # (candidate, step, v or None, beta or None)
    edits = [(1024, 0, 1.2, 1.15), (201, 0, None, -1.15), (813, N // 2, None, 1.22),
             (390, last, None, -1.24),
             (odd, min(1, last), 40.0, 0.06), (589, 0, 36.0, -0.07),
             (47, 0, None, 1e8), (950, last, None, -1.3e8),
             (5, 0, None, math.nan), (700, last, None, math.nan),
             (513, last, math.inf, None)]
    if N >= 2:
        edits.append((1024, 1, 30.0, 0.05))
    for c, s, vv, bb in edits:
        if vv is not None:
            v[s, c] = vv
        if bb is not None:
            b[s, c] = bb
    dup = ((10, 11), (30, 300), (100, 712))
    for src, dst in dup:
        v[:, dst], b[:, dst] = v[:, src], b[:, src]
    v.flags.writeable = b.flags.writeable = False
    return SimpleNamespace(n=n, n_steps=N, v=v, b=b, dup=dup,
                           beta_irregular=(1024, 201, 813, 390, 47, 950),
                           dphi_irregular=(odd, 589), nonfinite=(5, 700, 513))


def check_preconditions(inp, costs):
    """What must hold of the replica's costs of an input before a kernel is
    looked at.  Returns the number of finite costs."""
    costs = np.asarray(costs)
    fin = np.isfinite(costs)
    assert not fin[list(inp.nonfinite)].any()
    dst = [d for _, d in inp.dup]
    for s, d in inp.dup:
        assert fin[s] and costs[s] == costs[d], (s, d, costs[s], costs[d])
    rest = fin.copy()
    rest[dst] = False
    assert len(np.unique(costs[rest])) == int(rest.sum()), "an unintended tie"
    first = set(expected_order(costs)[:20].tolist())
    assert first & set(inp.beta_irregular), "no |beta| > 1.1 candidate among the first 20"
    assert int(fin.sum()) >= inp.n - 3 - 8
    return int(fin.sum())


# ----------------------------------------------------------------------------
# keep-out circles
# ----------------------------------------------------------------------------
def circles(states, winner, n_steps):
    """The three circles of obstacle_cases.case around this input: (a) on the
    unconstrained winner's final state, r = 0.10 reach; (b) at 0.45 reach ahead
    of the start pose, 0.1 rad right of its heading, r = 0.05 reach; (c) (5, 5,
    0.5), never reached; reach = 0.05 N."""
    reach = 0.05 * n_steps
    h = START[2] - 0.1
    return [(float(states[-1, 0, winner]), float(states[-1, 1, winner]), 0.10 * reach),
            (START[0] + 0.45 * reach * math.cos(h), START[1] + 0.45 * reach * math.sin(h),
             0.05 * reach),
            (5.0, 5.0, 0.5)]


def blocked(states, circ):
    """(mask, min |distance - r|) from the replica's states with the header's
    formula: any step, any circle, (x_k - x)^2 + (y_k - y)^2 < r^2; a NaN state
    is inside no circle."""
    x, y = states[:, 0, :], states[:, 1, :]
    m = np.zeros(states.shape[2], dtype=bool)
    margin = math.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for cx, cy, r in circ:
            d2 = (x - cx) ** 2 + (y - cy) ** 2
            m |= (d2 < r * r).any(axis=0)
            margin = min(margin, float(np.nanmin(np.abs(np.sqrt(d2) - r))))
    return m, margin


# ----------------------------------------------------------------------------
# the workload's grid shape: a top-K case
# ----------------------------------------------------------------------------
BIG_N = 2 * 2048 * 512 + N_CAND     # blocks stride over three rounds of tiles
BIG_STEPS = 4
BIG_TOP = 96


def big_positions():
    """Where the 96 best candidates are put.  The launch has 2048 tile blocks and
    4099 tiles; block k takes tiles k, 2048 + k, 4096 + k.  The first and last lane
    pair of rounds 0, 1, 2 of the first block (tiles 0, 2048, 4096) and of rounds
    0, 1 of the last block (tiles 2047, 4095: it has no third round); the lone
    pair of the final partial tile 4098; the rest over other blocks' second rounds
    and the only other third-round tile, 4097."""
    pos = []
    for t in (0, 2048, 4096, 2047, 4095):
        pos += [t * 512, t * 512 + 1, t * 512 + 510, t * 512 + 511]
    pos += [4098 * 512, 4098 * 512 + 1]
    k = 0
    while len(pos) < BIG_TOP:
        t = 4097 if k % 5 == 0 else 2048 + 1 + (k * 397) % 2046
        pos.append(t * 512 + (k * 131) % 512)
        k += 1
    assert len(set(pos)) == BIG_TOP and max(pos) < BIG_N
    return pos


def place_best(v, b, costs, positions):
    """Swap whole columns so that the len(positions) best candidates by (cost,
    index) sit at `positions`, best first (the multiset of costs is kept).
    Returns (v, b, costs) of the permuted input."""
    n = len(costs)
    best = expected_order(costs)[:len(positions)]
    perm = np.arange(n)                       # new column -> original column
    for orig, pos in zip(best, positions):
        cur = int(np.flatnonzero(perm == orig)[0])
        perm[cur], perm[pos] = perm[pos], perm[cur]
    return np.ascontiguousarray(v[:, perm]), np.ascontiguousarray(b[:, perm]), costs[perm]


# ----------------------------------------------------------------------------
# the cases' problems (shared by the CPU preconditions and the GPU cases)
# ----------------------------------------------------------------------------
MODES = ("qk21", "rect", "qk21+rot", "rect+rot", "rect+cum")
WHEELBASES = (0.5, 0.45)      # the power-of-two and the divided form
MARGIN = 1e-9                 # obstacle_cases.MARGIN
# the batched entry's robots: three poses over the same columns
BATCH_POSES = (START[:3], (0.25, -0.05, 0.8), (0.1, -0.2, 0.6))
DT = 0.05                     # config.py's delta_t


def chain_batch_a(n_steps, n=N_CAND):
    """The chained cases' first batch A: a grid batch of the ranked batch's
    shape that is never edited."""
    v, b = grid_batch(n, n_steps, 900 + n_steps)
    v.flags.writeable = b.flags.writeable = False
    return v, b


def problem_after(pose, L):
    """The second step's problem of an episode whose first step moved to `pose`
    (episode.logged_step_problems: t += delta_t per step)."""
    t = (0.0 + DT) + DT
    return problem(L, pose, t, t + DT)
