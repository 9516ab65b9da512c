"""The cases of the device-resident episode's keep-out-circle tests
(tests/test_episode_obstacles_abi.py checks their preconditions with the IEEE
replica on the CPU, tests/test_episode_obstacles_gpu.py runs them).

Every expectation is the host replica's (harness.replica_rollout with the
device's constants): its states give the blocked mask (ranking.blocked, the
header's formula), its costs the ranking of the candidates the mask leaves.
"""
import numpy as np

import ranking as R
from harness import replica_rollout

# (mode, L, n_steps, n): the first step of an episode from ranking.START
# (heading 0.7: the frame transform of rect+cum is not trivial); 1025 columns:
# the scalar path
FIRST_STEP = ([("rect+cum", L, N, R.N_CAND) for L in R.WHEELBASES for N in (1, 3, 10)] +
              [("rect+rot", 0.5, 3, R.N_CAND), ("qk21", 0.5, 3, R.N_CAND),
               ("rect+cum", 0.5, 3, 1025)])
# the chained second step: (L, n_steps)
SECOND_STEP = [(L, N) for L in R.WHEELBASES for N in (1, 3, 10)]
# circles no candidate comes near: they fill a table up to the count of an instantiation
FAR = tuple((6.0 + 0.7 * i, -4.0, 0.3) for i in range(13))


def with_far(circ, count):
    """`count` circles: the first of ranking.circles alone (count 1), or all
    three plus far ones."""
    if count == 1:
        return list(circ[:1])
    assert count >= len(circ)
    return list(circ) + list(FAR[:count - len(circ)])


def counts_of(n):
    """The circle counts a case runs with: every streaming instantiation (1, 4,
    16) on the aligned path; the scalar path has one."""
    return (1, 4, 16) if n % 2 == 0 else (4,)


def masked(st, costs, n_steps, counts, circ=None):
    """{count: (circles, mask)} around the unconstrained winner of (st, costs)
    (circ: ranking.circles unless given), with the preconditions of a ranked
    obstacle case asserted: the mask is the same in every arithmetic (margin),
    the unconstrained winner is blocked, some but not all candidates are."""
    winner = int(R.expected_order(costs)[0])
    if circ is None:
        circ = R.circles(st, winner, n_steps)
    out = {}
    for k in counts:
        c = with_far(circ, k)
        mask, margin = R.blocked(st, c)
        assert margin > R.MARGIN, (k, margin)
        assert mask[winner], "the unconstrained winner is not blocked"
        assert 0 < mask.sum() < len(costs), int(mask.sum())
        out[k] = (c, mask)
    return out


def first_step(mode, L, n_steps, n, device):
    """(input, states, costs) of a first-step case; device: with the GPU's
    reciprocal estimates (exact), else the IEEE replica (the preconditions do
    not depend on last bits)."""
    inp = R.controls(n_steps, n)
    st, costs = replica_rollout(R.problem(L), inp.v, inp.b, mode, device_estimates=device,
                                device_consts=True)
    return inp, st, costs


BIG_SEEDS = (4243, 4244)      # the grid-shape case's batches A and B


def big_circles(st, costs):
    """The grid-shape case's circle.  Its two million grid candidates end within
    centimetres of each other, so ranking.circles' radius would block them all:
    the circle sits on the unconstrained winner's final state and takes in its
    500 to 2000 nearest final states, the rim in the widest gap between two
    consecutive distances there (every earlier state is a step's length away)."""
    w = int(R.expected_order(costs)[0])
    fx, fy = st[-1, 0, :], st[-1, 1, :]
    d = np.sort(np.hypot(fx - fx[w], fy - fy[w])[np.isfinite(costs)])[500:2001]
    k = int(np.argmax(np.diff(d)))
    return [(float(fx[w]), float(fy[w]), float(0.5 * (d[k] + d[k + 1])))]


def batch_a_winner(L, n_steps, device, batch=None):
    """Step A of the chained cases on the replica: (winner's states [N, 3],
    the pose step B starts from = its first layer, the target being far)."""
    va, ba = batch if batch is not None else R.chain_batch_a(n_steps)
    st, costs = replica_rollout(R.problem(L), va, ba, "rect+cum", device_estimates=device,
                                device_consts=True)
    w = int(R.expected_order(costs)[0])
    return st[:, :, w], tuple(float(q) for q in st[0, :, w])


def a_unblocked(traj_a, circ):
    """Step A runs under step B's circles too (the chain is not broken between
    them): its winner must stay its winner, clear of every circle."""
    mask, margin = R.blocked(np.ascontiguousarray(traj_a[:, :, None]), circ)
    assert not mask[0] and margin > R.MARGIN, (bool(mask[0]), margin)
