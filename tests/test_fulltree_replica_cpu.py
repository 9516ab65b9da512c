"""The full-tree replica, the shard sweep's index maps and prediction, and the
inputs' preconditions, without a GPU (tests/fulltree_cases.py; the GPU side is
tests/test_fulltree_replica_gpu.py).

* The replica (harness.replica_fulltree with the host's reciprocals) against
  oracle.fulltree_argmin on every case input: the same winner, cost and states
  within test_fulltree_gpu.py's bars.
* unit_of() / shard_range(): the shards partition the units, every leaf lies in
  exactly one unit, for every S1 and every n_shards of the sweeps.
* expected_records() against a plain per-shard scan of the replica's costs.
* What keeps the sweeps from being vacuous, on the replica's numbers alone.
"""
import math

import numpy as np
import pytest

import fulltree_cases as F

STATE_TOL = 1e-9        # tests/test_fulltree_gpu.py
COST_RTOL = 1e-12


def _inputs():
    """(s1, problem, mode, L, nan_v) of every input the GPU cases run."""
    out = []
    for s1 in (5, 9, 14, 35):
        out += [(s1, name, mode, F.WHEELBASE, None) for name in F.PROBLEMS for mode in F.MODES]
    out += [(35, name, mode, F.WHEELBASE, None) for name in F.RANDOM_SEEDS for mode in F.MODES]
    out += [(65, "move", mode, F.WHEELBASE, nan) for mode in ("qk21", "rect+rot")
            for nan in (None, 1, 0)]
    out += [(72, "move", mode, F.WHEELBASE, None) for mode in ("qk21", "rect+rot")]
    out += [(35, "move", mode, F.WHEELBASE_NO_ROT, None) for mode in ("rect+rot", "qk21+rot")]
    return out


def test_sweep_sizes():
    assert [F.n_units(s) for s in (5, 9, 14, 35, 65, 72)] == [5, 18, 56, 700, 4355, 5832]
    assert F.sweep(14) == [1, 2, 3, 5, 8, 13, 21, 34, 55, 56]
    assert sum(F.sweep(14)) == 198 and sum(F.sweep(35)) == 2295
    assert F.sweep(5) == [1, 2, 3, 5] and F.sweep(65)[-2:] == [4181, 4355]
    assert F.where(322, 35) == ("leaf 322 = (k0 0, k1 9, k2 7): group 0, lane 9, k2 % 4 = 3, "
                                "unit 7")


@pytest.mark.parametrize("s1", sorted(F.SHAPES))
def test_units_and_shards_partition(s1):
    nu = F.n_units(s1)
    u = F.unit_of(np.arange(s1 ** 3), s1)
    assert u.min() == 0 and u.max() == nu - 1
    # a unit holds one leaf per pair of its group: 64, fewer in the last group
    per_unit = np.bincount(u, minlength=nu).reshape(-1, s1)
    last = s1 * s1 - 64 * (per_unit.shape[0] - 1)
    assert (per_unit[:-1] == 64).all() and (per_unit[-1] == last).all()
    for n in F.sweep(s1):
        r = [F.shard_range(s, n, s1) for s in (range(n) if n <= 100 else
                                               (0, 1, nu % n, max(nu % n - 1, 0), n - 2, n - 1))]
        if n <= 100:
            assert r[0][0] == 0 and r[-1][1] == nu
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(hi - lo in (nu // n, nu // n + 1) and hi > lo for lo, hi in r)
        # the vector form of expected_records is the same split
        minima = (np.zeros(nu), np.arange(nu), np.ones(nu, dtype=np.int64))
        _, _, size = F.expected_records(minima, n)
        lo = np.concatenate([[0], np.cumsum(size)[:-1]])
        for s in (0, n // 2, n - 1):
            assert (int(lo[s]), int(lo[s] + size[s])) == F.shard_range(s, n, s1)


@pytest.mark.parametrize("s1, name, mode, L, nan_v", _inputs())
def test_replica_vs_oracle(oracle, s1, name, mode, L, nan_v):
    """The same winner (these inputs are chosen so that it is), cost and states."""
    c = F.case(s1, name, mode, L, nan_v)
    ref = F.oracle_winner(oracle, c.problem, c.V, c.B, mode)
    leaf, cost, _ = F.expected_records(c.minima, 1)
    assert int(leaf[0]) == ref["leaf"] and ref["found"]
    assert math.isclose(cost[0], ref["cost"], rel_tol=COST_RTOL)
    st = F.layer_states(c, leaf)[0]
    assert np.abs(st - np.array(ref["traj"])).max() <= STATE_TOL


@pytest.mark.parametrize("s1, name, mode, nan_v", [
    (5, "move", "rect", None), (9, "near", "qk21+rot", None), (14, "move", "rect+rot", None),
    (14, "stay", "qk21", None), (35, "move", "rect+rot", None), (35, "near", "qk21", None),
    (65, "move", "qk21", 0), (65, "move", "rect+rot", 1)])
def test_expected_records_equal_a_plain_scan(s1, name, mode, nan_v):
    """expected_records (unit minima, reduced per shard) == the script's scan
    over the shard's leaves, the scan standing in for the kernel; and
    check_records notices one wrong leaf, cost bit or found."""
    c = F.case(s1, name, mode, F.WHEELBASE, nan_v)
    n_list = F.sweep(s1)
    if s1 > 35:     # the scan costs S1^3 per shard: the two ends and a middle of the sweep
        n_list = [1, 2, 3, 55, 4355]
    rng = np.random.default_rng(s1)
    rows, log = [], []
    for n in n_list:
        # (unit 0 is NaN with V[0] = NaN, unit 13 = (group 0, k2 13) with V[1] = NaN)
        shards = range(n) if n <= 100 else sorted({0, 13} | set(rng.choice(n, 40, replace=False)))
        leaf, cost, _ = F.expected_records(c.minima, n)
        for s in shards:
            j, cj = F.scan_shard(c.costs, s1, s, n)
            assert (j, cj) == (int(leaf[s]), float(cost[s])), (n, s)
            rows.append((n, s))
            log.append((j, cj))
    assert any(j < 0 for j, _ in log) == (nan_v is not None)
    if s1 != 14 or name != "move":
        return
    # the scan's records as a device log, through the comparison
    n_list = F.sweep(s1)
    words = np.zeros((sum(n_list), F.REC_WORDS), dtype=np.int64)
    i = 0
    rows = []
    for n in n_list:
        for s in range(n):
            j, cj = F.scan_shard(c.costs, s1, s, n)
            k = np.array([j // (s1 * s1), (j // s1) % s1, j % s1])
            words[i, 0] = np.float64(cj).view(np.int64)
            words[i, 1] = j
            words[i, 2] = 1 | (s1 << 32)
            words[i, 3:6] = k
            words[i, 6:9] = c.V[k // len(c.B)].view(np.int64)
            words[i, 9:12] = c.B[k % len(c.B)].view(np.int64)
            words[i, 12:21] = F.layer_states(c, [j])[0].ravel().view(np.int64)
            rows.append((n, s))
            i += 1
    assert F.check_sweep(words, rows, c, n_list) == (198, 65)
    for col, delta, text in ((1, 1, "expected leaf"), (0, 1, "expected leaf"),
                             (2, -1, "expected leaf"), (5, 1, r"k\[\]"), (7, 1, r"v\[\]"),
                             (10, 1, r"beta\[\]"), (20, 1, "layer states")):
        wrong = words.copy()
        wrong[87 + 8, col] += delta
        with pytest.raises(AssertionError, match=f"n_shards 55, shard 8 .*{text}"):
            F.check_sweep(wrong, rows, c, n_list)


def _ties_at_minimum(c):
    leaf, _, ties = F.expected_records(c.minima, 1)
    return int(leaf[0]), int(ties[0])


@pytest.mark.parametrize("mode", F.MODES)
def test_preconditions_ties(mode):
    """The sweeps meet ties: structural ones (v = 0 makes beta irrelevant), so
    they do not depend on the reciprocal estimates."""
    for s1 in (5, 9, 14, 35):
        nb = F.SHAPES[s1][1]
        assert _ties_at_minimum(F.case(s1, "stay", mode)) == (0, nb ** 3)
    leaf, ties = _ties_at_minimum(F.case(35, "near", mode))
    assert leaf != 0 and ties >= 2
    for s1 in (14, 35):
        shards, tied = F.tied_shards(F.case(s1, "move", mode))
        assert shards == sum(F.sweep(s1)) and tied * 10 >= shards
    if mode == "rect+rot":      # the figures this file was written with
        assert (leaf, ties) == (322, 21)
        assert F.tied_shards(F.case(14, "move", mode)) == (198, 65)
        assert F.tied_shards(F.case(35, "move", mode)) == (2295, 400)
        assert len(np.unique(F.case(35, "move", mode).costs)) < 23000


@pytest.mark.parametrize("mode", ("qk21", "rect+rot"))
def test_preconditions_non_finite(mode):
    """V[1] = NaN: NaN costs next to finite ones, the v = 0 ties stay.  V[0] =
    NaN: shards without a finite leaf and shards with one."""
    c = F.case(65, "move", mode, nan_v=1)
    nan = np.isnan(c.costs).reshape(-1, 65)[:, :64].reshape(-1, 4)      # the rows' quads
    assert (nan.any(axis=1) & ~nan.all(axis=1)).any()
    assert F.tied_shards(c)[1] > 0
    c = F.case(65, "move", mode, nan_v=0)
    assert np.isnan(c.costs[:64 * 65]).all()                 # all of group 0
    empty = sum(int((F.expected_records(c.minima, n)[0] < 0).sum()) for n in F.sweep(65))
    assert 0 < empty < sum(F.sweep(65))
    assert np.isfinite(F.case(65, "move", mode).costs).all()


def test_preconditions_rotation_flag():
    for mode in ("rect+rot", "qk21+rot"):
        assert F.case(35, "move", mode, F.WHEELBASE_NO_ROT).no_rot == 1
        assert F.case(35, "move", mode).no_rot == 0
        # with the flag raised the rotation modes compute the direct modes' numbers
        direct = F.case(35, "move", mode.split("+")[0], F.WHEELBASE_NO_ROT)
        assert direct.no_rot == 1
        assert np.array_equal(direct.costs, F.case(35, "move", mode, F.WHEELBASE_NO_ROT).costs)
        assert not np.array_equal(F.case(35, "move", mode.split("+")[0]).costs,
                                  F.case(35, "move", mode).costs)


@pytest.mark.parametrize("s1, name, mode, L, nan_v", _inputs())
def test_preconditions_crit_sqrt_range(s1, name, mode, L, nan_v):
    """The device's crit_sqrt is exact for 0 and from 2^-767 up: no leaf of a
    case comes closer to its target than that, except `stay`'s exact 0."""
    c = F.case(s1, name, mode, L, nan_v)
    st = F.layer_states(c, np.arange(s1 ** 3))[:, 2]          # the leaves' states
    d2 = (c.problem.x_t - st[:, 0]) ** 2 + (c.problem.y_t - st[:, 1]) ** 2
    fin = np.isfinite(c.costs)
    assert np.isfinite(d2[fin]).all()
    small = fin & (d2 < 2.0 ** -767)
    assert (d2[small] == 0.0).all() and (small.any() == (name == "stay"))
