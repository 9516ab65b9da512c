"""The ranking driver's self-check and the inputs' preconditions, without a GPU.

* tests/ranking.py's peel() driven with oracle.rollout_argmin as the "kernel"
  must reproduce the oracle's own per-candidate costs sorted by (cost, index).
* What tests/test_ranking_gpu.py requires of its inputs holds of the host
  replica's costs (replica_rollout without device estimates): ties only where
  duplicates were planted, a |beta| > 1.1 candidate among the first 20, circles
  whose mask does not depend on the arithmetic.
"""
import math
import sys

import numpy as np
import pytest
import torch

import ranking as R
from harness import replica_rollout

INC_MAX = float(sys.maxsize)


def _oracle_case():
    n, N = 130, 3
    v, b = R.grid_batch(n, N, 7)
    b[0, 5] = math.nan
    v[2, 77] = math.nan
    v[2, 40], b[2, 40] = 1e300, 0.0          # a +inf cost: the squared distance overflows
    for dst in (20, 60, 129):                # three exact duplicates of column 3
        v[:, dst], b[:, dst] = v[:, 3], b[:, 3]
    return v, b


def test_driver_ranks_the_oracle(oracle):
    v, b = _oracle_case()
    n = v.shape[1]
    p = R.problem(0.5)
    _, costs, states = oracle.rollout_argmin(p, v, b, integ="rect", want_costs=True,
                                             want_states=True)
    assert np.isnan(costs[[5, 77]]).all() and costs[40] == math.inf
    assert costs[3] == costs[20] == costs[60] == costs[129]

    def launch():
        res, _, _ = oracle.rollout_argmin(p, v, b, incumbent=INC_MAX, integ="rect")
        return R.result_words(torch.frombuffer(bytearray(bytes(res)), dtype=torch.uint8))

    got = R.peel(launch, torch.from_numpy(v), R.soa_offset(), n)[:, 0]
    assert R.check_ranking(got, costs, states=states, what="oracle") == n - 3
    assert int(np.isnan(v[0]).sum()) == n - 3          # one NaN per peeled candidate
    # the comparison notices one wrong index, one wrong cost, one entry too many
    for col, row in ((1, 17), (0, 90)):
        wrong = got.copy()
        wrong[row, col] = wrong[row + 1, col]
        with pytest.raises(AssertionError, match=f"rank {row} of"):
            R.check_ranking(wrong, costs, what="oracle")
    wrong = got.copy()
    wrong[n - 3, 1:3] = (7, 1)
    with pytest.raises(AssertionError, match="after the 127 finite"):
        R.check_ranking(wrong, costs, what="oracle")
    with pytest.raises(AssertionError, match="peels for"):
        R.check_ranking(got[:n - 3], costs, what="oracle")


def test_driver_top_k_and_batched_offsets():
    """top=: only a prefix is compared; soa_offset(ld) addresses robot r's columns."""
    costs = np.array([3.0, 1.0, math.nan, 1.0, 2.0])
    got = np.zeros((3, 3), dtype=np.int64)
    got[:, 0] = np.array([1.0, 1.0, 2.0]).view(np.int64)
    got[:, 1] = (1, 3, 4)
    got[:, 2] = 1
    assert R.check_ranking(got, costs, top=3) == 3
    with pytest.raises(AssertionError):
        R.check_ranking(got, costs)
    assert R.soa_offset(10)(torch.tensor([4, 0, 9])).tolist() == [4, 10, 29]
    assert R.tiled_offset(3)(torch.tensor([0, 511, 512, 1025])).tolist() == [0, 511, 3072, 6145]
    assert R.where(1025) == "candidate 1025: tile 2, wave 0, lane 0, pair slot 1"


def test_big_positions_are_distinct_lane_pairs():
    pos = R.big_positions()
    assert len(pos) == R.BIG_TOP and pos[:4] == [0, 1, 510, 511]
    assert R.BIG_N - 2 in pos and R.BIG_N - 1 in pos
    v = np.arange(24.0).reshape(2, 12)
    costs = np.array([5, 4, 9, 1, 7, 3, 8, 2, 6, 0, 11, 10], dtype=np.float64)
    v2, _, c2 = R.place_best(v, v, costs, [11, 0, 5])
    assert list(R.expected_order(c2)[:3]) == [11, 0, 5]
    assert sorted(c2) == sorted(costs) and sorted(v2[0]) == sorted(v[0])


def _polygon_cases():
    """Every case of tests/test_ranking_polygons_gpu.py, as polygon_case's arguments."""
    import polygon_cases as pc
    cases = [dict(name="start", mode=m, n_steps=N, plant=N == 3)
             for m in R.MODES for N in (1, 3, 10)]
    cases += [dict(name=name, mode=m, n_steps=3) for name in pc.PLACEMENTS if name != "start"
              for m in ("rect", "rect+cum", "qk21+rot")]
    cases += [dict(name=name, mode=m, n_steps=3, mixed=True) for name in ("start", "ten-II")
              for m in ("rect", "rect+cum", "qk21")]
    cases += [dict(name="start", mode=m, n_steps=N, n=n) for n in (1025, R.N_CAND)
              for m in ("rect", "rect+cum") for N in (1, 3)]
    cases += [dict(name="ten-III", mode="rect+cum", n_steps=3, n_poly=k) for k in (1, 2, 3)]
    return cases


def test_polygon_case_preconditions(oracle):
    """What the keep-out polygon ranking cases assert of their reference before
    a launch holds of the host replica without the device's estimates: the
    scene's conditions, the host-built mask against the exact rule, and how few
    states the header's bound leaves out (ranking.check_polygon_scene)."""
    cases = _polygon_cases()
    assert len(cases) == 15 + 18 + 6 + 8 + 3
    total = 0
    for kw in cases:
        c = R.polygon_case(**kw)
        assert 0 < c.n_free < c.n_fin
        if c.through is not None:
            assert c.through[0] not in c.inp.beta_irregular + c.inp.dphi_irregular
        total += c.n_free
    print(f"{len(cases)} cases, {total} candidates to rank")


@pytest.mark.parametrize("n_steps", R.HORIZONS + (10,))
def test_input_preconditions(oracle, n_steps):
    """Every problem the GPU cases rank, on the host replica."""
    for n in (R.N_CAND, 1025):
        inp = R.controls(n_steps, n)
        assert inp.v.shape == (n_steps, n)
        assert (np.abs(inp.b[:, list(inp.beta_irregular)]) > 1.1).any(axis=0).all()
        assert np.isnan(inp.b).any(axis=0).sum() == 2 and np.isinf(inp.v).any(axis=0).sum() == 1
        for L in R.WHEELBASES:
            for mode in R.MODES:
                if n == 1025 and mode not in ("rect", "rect+cum"):
                    continue
                for consts in (False, True):            # one-shot / episode constants
                    _, costs = replica_rollout(R.problem(L), inp.v, inp.b, mode,
                                               device_consts=consts)
                    assert R.check_preconditions(inp, costs) == n - 3
    inp = R.controls(n_steps)
    # the batched robots' poses
    for pose in R.BATCH_POSES:
        for mode in ("rect+rot", "rect+cum"):
            _, costs = replica_rollout(R.problem(0.5, pose), inp.v, inp.b, mode,
                                       device_consts=True)
            R.check_preconditions(inp, costs)
    # the chained cases: B after the first step of A's winner
    va, ba = R.chain_batch_a(n_steps)
    for L in R.WHEELBASES:
        st, costs = replica_rollout(R.problem(L), va, ba, "rect+cum", device_consts=True)
        w = int(R.expected_order(costs)[0])
        _, costs = replica_rollout(R.problem_after(st[0, :, w], L), inp.v, inp.b, "rect+cum",
                                   device_consts=True)
        R.check_preconditions(inp, costs)
    # the circles
    if n_steps in (1, 3, 10):
        for mode in R.MODES:
            st, costs = replica_rollout(R.problem(0.5), inp.v, inp.b, mode)
            w = int(R.expected_order(costs)[0])
            circ = R.circles(st, w, n_steps)
            mask, margin = R.blocked(st, circ)
            assert margin > R.MARGIN and mask[w] and 0 < mask.sum() < inp.n
