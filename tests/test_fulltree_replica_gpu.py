"""Every shard's winner of the full-tree kernels (csrc/mpc_fulltree.h) against
the host replica, bit for bit (tests/fulltree_cases.py; its index maps,
prediction and inputs are checked without a GPU in test_fulltree_replica_cpu.py).

Production library, public ABI.  A case sweeps n_shards over every Fibonacci
number below the tree's unit count and the unit count itself; every shard of
every split must report the replica's finite-cost leaf with the smallest (cost,
leaf) of its unit range: leaf, cost bits, found, s1, k[], v[], beta[] and the
three layer states.  The cases are the smallest trees at which each index edge
of k_ft_leaves exists; each prints its launches, the shards whose minimum was
tied, and its wall time."""
import math
import time

import numpy as np
import pytest

import fulltree_cases as F

pytestmark = pytest.mark.gpu


def _sweep(engine, s1, name, mode, L=F.WHEELBASE, nan_v=None):
    c = F.case(s1, name, mode, L, nan_v, True)
    n_list = F.sweep(s1)
    what = f"S1 {s1} {name} {mode}" + (f" L {L}" if L != F.WHEELBASE else "") + \
        (f" V[{nan_v}] = NaN" if nan_v is not None else "")
    t0 = time.perf_counter()
    log, rows = F.run_sweep(engine, c, n_list)
    t1 = time.perf_counter()
    n, tied = F.check_sweep(log, rows, c, n_list, what=what)
    assert n == sum(n_list)
    print(f"{what}: {n} launches, {tied} tied shards, {int((log[:, 1] < 0).sum())} without a "
          f"finite leaf, {t1 - t0:.2f} s on the device, {time.perf_counter() - t1:.2f} s checking")
    return c, log


@pytest.mark.parametrize("name", F.PROBLEMS)
@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("s1", [5, 9, 14, 35])
def test_every_shard_small_trees(engine, s1, mode, name):
    """S1 = 5 (1 x 5) and 9 (3 x 3): fewer units than waves (empty shares,
    every piece a quad of one, 39 and 47 clamped lanes).  S1 = 14 (2 x 7):
    S1 = 2 mod 4, 196 pairs (the last group is 4 lanes full).  S1 = 35 (5 x 7):
    S1 odd, every group boundary mid-row."""
    _sweep(engine, s1, name, mode)


@pytest.mark.parametrize("nan_v", [None, 1, 0])
@pytest.mark.parametrize("mode", ["qk21", "rect+rot"])
def test_every_shard_workload_grid(engine, mode, nan_v):
    """S1 = 65 (5 x 13, workload G's grid), as it is and with a NaN speed:
    V[1] = NaN puts NaN costs inside quads next to finite ones (the v = 0 ties
    stay), V[0] = NaN makes all of the first groups NaN (shards without a
    finite leaf: leaf -1, found 0, cost +inf)."""
    c, log = _sweep(engine, 65, "move", mode, nan_v=nan_v)
    assert (log[:, 1] < 0).any() == (nan_v is not None)
    assert c.no_rot == (nan_v is not None)      # a NaN dphi is not <= kRotMax


@pytest.mark.parametrize("mode", ["qk21", "rect+rot"])
def test_every_shard_no_clamped_lane(engine, mode):
    """S1 = 72 (8 x 9): S1 a multiple of 4 and S1^2 of 64, no clamped lane, no tail."""
    _sweep(engine, 72, "move", mode)


@pytest.mark.parametrize("mode", ["rect+rot", "qk21+rot"])
def test_rotation_fallback(engine, mode):
    """L = 0.25 makes some |dphi| > kRotMax: the launch-wide flag is raised and
    the rotation modes evaluate directly -- the replica's direct numbers, and
    record for record what a launch in the direct mode reports."""
    c, log = _sweep(engine, 35, "move", mode, L=F.WHEELBASE_NO_ROT)
    assert c.no_rot == 1
    direct, _ = F.run_sweep(engine, c, F.sweep(35), mode=mode.split("+")[0])
    assert np.array_equal(log, direct)


@pytest.mark.parametrize("mode", F.MODES)
def test_incumbent_at_the_winners_cost(engine, mode):
    """found is cost < incumbent, strictly: 0 with the incumbent at the
    winner's cost (leaf and cost still reported), 1 one ulp above it."""
    c = F.case(14, "move", mode, F.WHEELBASE, None, True)
    leaf, cost, _ = F.expected_records(c.minima, 1)
    states = F.layer_states(c, leaf)
    for inc, found in ((float(cost[0]), 0), (math.nextafter(float(cost[0]), math.inf), 1)):
        log, _ = F.run_sweep(engine, c, [1], incumbent=inc)
        F.check_records(log, 14, c.V, c.B, leaf, cost, [found], states,
                        lambda i: f"incumbent {inc!r}", f"S1 14 move {mode}")


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("n_robots", [1, 5, 1500])
def test_batched_entry(engine, n_robots, mode):
    """mpc_fulltree_argmin_batched at S1 = 35 against the replica with the
    device's constants: R = 1 (6 blocks per robot), R = 5 (the three problems
    and two seeded random ones), R = 1500 (cycling through those five: 2 blocks
    per robot, another wave split).  Robot r's incumbent is its winner's cost
    (found 0) for even r, one ulp above (found 1) for odd r."""
    s1 = 35
    cases = [F.case(s1, name, mode, F.WHEELBASE, None, True, True)
             for name in F.BATCH_PROBLEMS[:min(n_robots, 5)]]
    win = [F.expected_records(c.minima, 1) for c in cases]
    st = [F.layer_states(c, w[0]) for c, w in zip(cases, win)]
    which = np.arange(n_robots) % len(cases)
    leaf = np.array([win[k][0][0] for k in which])
    cost = np.array([win[k][1][0] for k in which])
    states = np.stack([st[k][0] for k in which])
    found = np.arange(n_robots) % 2
    inc = np.where(found == 1, np.nextafter(cost, math.inf), cost)
    t0 = time.perf_counter()
    log = F.run_batched(engine, [cases[k].problem for k in which], inc, cases[0].V, cases[0].B,
                        mode)
    F.check_records(log, s1, cases[0].V, cases[0].B, leaf, cost, found, states,
                    lambda i: f"robot {i} (problem {F.BATCH_PROBLEMS[which[i]]})",
                    f"batched R {n_robots} {mode}")
    print(f"batched R {n_robots} {mode}: {time.perf_counter() - t0:.2f} s")
