"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the
reference's recorded outputs.

Bar (BASELINE.json north_star): chosen control identical; predicted
(x, y, phi) within 1e-6 abs.  Observed differences are ulp-level: the device
fp64 tan/sincos are faithfully rounded like glibc's but differ from them in
the last bit for a few % of arguments, so costs agree to ~1e-16 relative;
tests assert 1e-12 on costs and 1e-9 on states (far inside 1e-6), and an
identical arg-min index.  Where a test draws >= 1e5 random candidates, an
index disagreement is tolerated ONLY when the oracle's own costs of the two
candidates are within 1e-13 relative (a genuine near-tie below the ulp noise);
none has been observed.
"""
import math
import sys

import numpy as np
import pytest
import torch

from conftest import call_controls, call_problem

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-9
COST_RTOL = 1e-12
INC_MAX = float(sys.maxsize)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _same_choice(got, ref, costs=None):
    if got.index == ref.index:
        return True
    assert costs is not None, (got.as_dict(), ref.as_dict())
    gap = abs(costs[got.index] - costs[ref.index]) / abs(costs[ref.index])
    assert gap < 1e-13, f"index {got.index} vs {ref.index}, oracle cost gap {gap}"
    return False


def _threads():
    import os
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 8


def _report(name, **kv):
    """Append a parity record to $MPC_PARITY_REPORT (JSON lines), if set, and
    print it (pytest -s / the captured log)."""
    import json
    import os
    rec = dict(test=name, **kv)
    print("PARITY", json.dumps(rec))
    path = os.environ.get("MPC_PARITY_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _close_traj(got, ref, n_steps, tol=STATE_TOL):
    d = max(abs(got.traj[s][k] - ref.traj[s][k]) for s in range(n_steps) for k in range(3))
    assert d <= tol, d
    return d


def _grid451():
    from diplomjourney_amd import math_model_tree as mmt
    return mmt.vector_of_velocities(0.5), mmt.vector_of_beta_angles(0.0)


def _sampled(engine, n_cand, n_steps, seed=20261015, base=0):
    V, B = _grid451()
    v, b = engine.sample_controls(_dev(V), _dev(B), n_cand, n_steps, seed, index_base=base)
    return V, B, v, b


# --------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ["qk21", "rect", "rect+rot", "rect+cum"])
def test_scenario_replay_through_c_abi(engine, scenario, integ):
    """All 349 recorded predictive_control calls: identical (v, beta) and
    index; states within 1e-9 of the reference's own — for the reference's
    arithmetic (qk21) and for the bench's (rect+cum, the chained step's
    recurrence; rect+rot, the two-launch default of config E)."""
    worst = 0.0
    for rec in scenario["calls"]:
        v_sc, b_sc = call_controls(rec)
        engine.rollout_argmin(call_problem(rec), _dev(v_sc), _dev(b_sc),
                              incumbent=rec["pre"]["optimal_criterion"], integrator=integ)
        got = engine.fetch()
        assert got.found == rec["found"]
        assert (got.v, got.beta) == (rec["post"]["result_v"], rec["post"]["result_beta"])
        for s, ref in zip(got.trajectory(), rec["traj"]):
            worst = max(worst, max(abs(a - b) for a, b in zip(s, ref[:3])))
    assert worst <= STATE_TOL


def test_coordinate_tree_states(engine, scenario, candidates):
    """The kernel-filled CoordinateTree (states_out) against the reference's
    per-candidate layer states of 6 calls."""
    calls = {r["call"]: r for r in scenario["calls"]}
    for det in candidates["calls"]:
        rec = calls[det["call"]]
        v_sc, b_sc = call_controls(rec)
        n = v_sc.shape[1]
        states = torch.empty((3, 3, n), dtype=torch.float64, device="cuda")
        engine.rollout_argmin(call_problem(rec), _dev(v_sc), _dev(b_sc), integrator="qk21",
                              states=states)
        got = states.cpu().numpy()
        for layer in range(3):
            ref = np.array(det["layers"][layer]).T
            assert np.abs(got[layer] - ref).max() <= STATE_TOL


@pytest.mark.parametrize("integ", ["qk21", "rect+cum"])
def test_drop_in_scenario_end_to_end(engine, scenario, integ, monkeypatch):
    """The whole reference scenario (math_model_tree.py:736-738) through the
    drop-in predictive_control/math_mpc: every call's chosen control and
    returned state, the operator events and the episode trajectories — with
    the reference's arithmetic and with the bench's."""
    from diplomjourney_amd import math_model_tree as mmt
    monkeypatch.setattr(mmt, "INTEGRATOR", integ)
    seen = []
    orig = mmt.predictive_control

    def rec_pc(*a):
        ret = orig(*a)
        seen.append(ret)
        return ret
    mmt.predictive_control = rec_pc
    try:
        mmt.run_reference_scenario(seed=0)
    finally:
        mmt.predictive_control = orig
    ref = [c["ret"] for c in scenario["calls"]]
    assert len(seen) == len(ref) == 349
    for got, want in zip(seen, ref):
        assert got[3:] == want[3:]                       # chosen (v, beta): identical
        assert max(abs(a - b) for a, b in zip(got[:3], want[:3])) <= 1e-6
    for name, want in scenario["trajectories"].items():
        got = getattr(mmt, name)
        assert len(got) == len(want), name
        assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-6, name
    mmt.reset_state()


@pytest.mark.parametrize("n_cand,n_steps,integ", [
    (100_000, 3, "qk21"), (100_000, 3, "rect"), (200_000, 10, "rect"), (100_000, 12, "rect"),
    (50_000, 8, "qk21"), (30_001, 5, "rect"), (1000, 1, "rect"), (4096, 32, "qk21"),
    (200_000, 11, "rect"), (1, 3, "rect"), (257, 10, "rect"),
])
def test_synthetic_vs_oracle(engine, oracle, n_cand, n_steps, integ):
    V, B, v, b = _sampled(engine, n_cand, n_steps)
    vh, bh = v.cpu().numpy(), b.cpu().numpy()
    ov, ob = oracle.sample_controls(V, B, n_cand, n_steps, 20261015)
    assert np.array_equal(vh, ov) and np.array_equal(bh, ob)       # sampler: bitwise
    from diplomjourney_amd.abi import make_problem
    prob = make_problem(0.1, -0.2, 0.3, 2, 3, 0, 0, 0.5, 0.05, 0.1)
    engine.rollout_argmin(prob, v, b, incumbent=INC_MAX, integrator=integ)
    got = engine.fetch()
    ref, costs, _ = oracle.rollout_argmin(prob, vh, bh, incumbent=INC_MAX, integ=integ,
                                          want_costs=True)
    if _same_choice(got, ref, costs):
        _close_traj(got, ref, n_steps)
        assert math.isclose(got.cost, ref.cost, rel_tol=COST_RTOL)
        assert (got.v, got.beta, got.found) == (ref.v, ref.beta, ref.found)


def test_full_size_config_c(engine, oracle):
    """Config C size (N=10, 1e6 candidates) against the full oracle scan."""
    n_cand, n_steps = 1_000_000, 10
    V, B, v, b = _sampled(engine, n_cand, n_steps, seed=7)
    from diplomjourney_amd.abi import make_problem
    prob = make_problem(0.5, 0.2, 1.1, 2, 3, 0.1, -0.1, 0.5, 0.35, 0.4)
    engine.rollout_argmin(prob, v, b, incumbent=INC_MAX, integrator="rect")
    got = engine.fetch()
    ref, costs, _ = oracle.rollout_argmin(prob, v.cpu().numpy(), b.cpu().numpy(),
                                          incumbent=INC_MAX, integ="rect", want_costs=True)
    if _same_choice(got, ref, costs):
        _close_traj(got, ref, n_steps)


def test_chained_config_c_steps_vs_oracle(engine, oracle):
    """The bench's default step at config C's size: chained rect+cum launches
    of the device episode (1e6 candidates, N = 10, distinct resident batches
    drawn as bench.make_pool draws them).  Every logged step's winner is the
    oracle's full scan (reference arithmetic, glibc trig) of the same batch on
    the problem rebuilt on the host from the previous log record: chosen
    index, (v, beta) identical, returned pose within 1e-9, cost within 1e-12."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.abi import make_problem
    from diplomjourney_amd.episode import DeviceEpisode
    n, ns, steps = 1_000_000, 10, 6
    pool = _pool(engine, n, ns, steps, 0x5EED0000)
    ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", chain=True, log_capacity=64)
    for c in pool:
        ep.step(controls=c)
    ep.flush()
    log = ep.read_log()
    assert len(log) == steps and ep.chain_error() == 0
    x = y = phi = 0.0
    t = 0.0
    for i, (rec, (v, b)) in enumerate(zip(log, pool)):
        t = t + mmt.delta_t
        prob = make_problem(x, y, phi, 2, 3, 0, 0, mmt.L, t, t + mmt.delta_t)
        inc = 10000 * math.sqrt(13) + 10000 * 1000 ** 2 if i == 0 else INC_MAX
        ref, costs, _ = oracle.rollout_argmin(prob, v.cpu().numpy(), b.cpu().numpy(),
                                              incumbent=inc, integ="rect", want_costs=True)
        assert (rec.p, rec.found, ref.found) == (i + 1, 1, 1)
        if rec.index == ref.index:
            assert (rec.v, rec.beta) == (ref.v, ref.beta)
            assert math.isclose(rec.cost, ref.cost, rel_tol=COST_RTOL)
            d = max(abs(a - c) for a, c in zip((rec.x, rec.y, rec.phi), ref.traj[0]))
            assert d <= STATE_TOL, (i, d)
        else:   # only a near-tie below the ulp noise of the two recurrences
            gap = abs(costs[rec.index] - costs[ref.index]) / abs(costs[ref.index])
            assert gap < 1e-13, (i, rec.index, ref.index, gap)
        x, y, phi = rec.x, rec.y, rec.phi


def test_chained_config_c_events_and_restart_vs_oracle(engine, oracle):
    """The bench's default step at config C's size through a whole episode:
    130 chained rect+cum launches at 1e6 candidates x N = 10 with max_steps =
    115, so the operator events at p = 60 / 90 / 110 (turn_right, turn_left,
    new_target: math_model_tree.py:564-569) and an episode restart happen
    inside.  Every step's problem is rebuilt on the host with the drop-in's
    own event helpers (_turn_target, new target + line origin at the pose,
    t += dt, reset on a restart, the first incumbent of each episode from its
    line origin) from the previous log record — and must equal
    episode.logged_step_problems (the bench's parity leg) — and each batch is
    scanned in full by the oracle twice:
      * qk21, the reference's own arithmetic (scipy quad, math_model_tree.py
        :91-96): the logged winner IS its winner on every step (identity, no
        tolerance; SURVEY §7 hard part 2) and the costs agree within 1e-12;
      * rect, the kernel's integrator restated: same index and (v, beta), the
        returned pose one of the winner's layer states within 1e-9
        (finishing logic), or an index disagreement only below 1e-13 relative
        — every use of that branch is counted and reported (MPC_PARITY_REPORT)."""
    from concurrent.futures import ThreadPoolExecutor
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.abi import (MPC_EP_ARRIVED, MPC_EP_BREAK, MPC_EP_EVENT, MPC_EP_LIMIT,
                                       make_problem)
    from diplomjourney_amd.episode import DeviceEpisode
    n, ns, steps, max_steps, nb = 1_000_000, 10, 130, 115, 8
    pool = _pool(engine, n, ns, nb, 0x5EED0100)
    ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", chain=True, log_capacity=256,
                       max_steps=max_steps)
    for i in range(steps):
        ep.step(controls=pool[i % nb])
    ep.flush()
    log = ep.read_log()                      # raises on a nonzero chain_error
    assert len(log) == steps
    host = [(v.cpu().numpy(), b.cpu().numpy()) for v, b in pool]
    ended = MPC_EP_ARRIVED | MPC_EP_LIMIT | MPC_EP_BREAK

    def criterion0(xt, yt, x0, y0):
        return 10000 * math.sqrt((xt - x0) ** 2 + (yt - y0) ** 2) + 10000 * 1000 ** 2

    # the host's rebuild of every step's problem from the log so far
    probs = []
    x = y = phi = t = 0.0
    xt, yt, x0, y0 = 2.0, 3.0, 0.0, 0.0
    inc = criterion0(xt, yt, x0, y0)
    for rec in log:
        t = t + mmt.delta_t
        probs.append((make_problem(x, y, phi, xt, yt, x0, y0, mmt.L, t, t + mmt.delta_t), inc))
        inc = INC_MAX
        x, y, phi = rec.x, rec.y, rec.phi
        if rec.status & ended:
            x = y = phi = t = 0.0
            xt, yt, x0, y0 = 2.0, 3.0, 0.0, 0.0
            inc = criterion0(xt, yt, x0, y0)
            continue
        if rec.p == 60:
            xt, yt = mmt._turn_target(x, y, phi, 2, -1)
            x0, y0 = x, y
        elif rec.p == 90:
            xt, yt = mmt._turn_target(x, y, phi, 2, +1)
            x0, y0 = x, y
        elif rec.p == 110:
            xt, yt, x0, y0 = 2.0, 3.0, x, y
    events = sorted(r.p for r in log if r.status & MPC_EP_EVENT)
    assert events[:3] == [60, 90, 110], events
    assert len({r.episode for r in log}) >= 2                  # a restart inside
    from diplomjourney_amd.episode import logged_step_problems
    helper = logged_step_problems(log, ep.cfg)
    for (pa, ia), (pb, ib) in zip(probs, helper):
        assert [getattr(pa, f) for f, _ in pa._fields_] == \
            [getattr(pb, f) for f, _ in pb._fields_] and ia == ib
    with ThreadPoolExecutor(max_workers=_threads()) as ex:
        futs = [ex.submit(oracle.rollout_argmin, probs[i][0], *host[i % nb], incumbent=probs[i][1],
                          integ="rect", want_costs=True) for i in range(steps)]
        futq = [ex.submit(oracle.rollout_argmin, probs[i][0], *host[i % nb], incumbent=probs[i][1],
                          integ="qk21") for i in range(steps)]
        refs = [f.result() for f in futs]
        refq = [f.result()[0] for f in futq]
    near_ties, q_noise = [], 0.0
    for i, (rec, q) in enumerate(zip(log, refq)):     # the reference's arithmetic
        assert q.found == 1 and rec.index == q.index, (i, rec.index, q.index)
        assert (rec.v, rec.beta) == (q.v, q.beta), i
        q_noise = max(q_noise, abs(rec.cost - q.cost) / abs(q.cost))
    assert q_noise < COST_RTOL, q_noise
    for i, (rec, (ref, costs, _)) in enumerate(zip(log, refs)):
        assert rec.found == ref.found == 1, i
        if rec.index == ref.index:
            assert (rec.v, rec.beta) == (ref.v, ref.beta), i
            assert math.isclose(rec.cost, ref.cost, rel_tol=COST_RTOL), i
            d = min(max(abs(a - c) for a, c in zip((rec.x, rec.y, rec.phi), ref.traj[k]))
                    for k in range(3))
            assert d <= STATE_TOL, (i, d)
        else:   # only a near-tie below the ulp noise of the two recurrences
            gap = abs(costs[rec.index] - costs[ref.index]) / abs(costs[ref.index])
            assert gap < 1e-13, (i, rec.index, ref.index, gap)
            near_ties.append((i, gap))
    _report("chained_config_c_events_and_restart", steps=steps, candidates=n, horizon=ns,
            identity_vs_qk21=steps, max_rel_cost_diff_vs_qk21=q_noise,
            near_tie_branch_vs_rect=len(near_ties), near_ties=near_ties)


@pytest.mark.parametrize("integ", ["qk21", "rect+cum"])
def test_near_tie_candidates_vs_oracle(engine, oracle, integ):
    """Near ties below the two arithmetics' noise (the device's
    steering tangent starts from the non-IEEE v_rcp_f64 estimate): 4096
    candidates whose steering angles climb one ulp at a time from the same
    control (costs within ~1e-15 of each other), in 4 groups, each followed
    by exact duplicates of its first candidate.  The chosen index equals the
    oracle's (reference arithmetic, glibc trig) or, only where the oracle's
    own costs of the two differ by < 1e-13 relative, another member of the
    near tie; an exact duplicate never beats the lowest index."""
    from diplomjourney_amd.abi import make_problem
    n, ns = 4096, 10
    beta = np.empty(n)
    b0 = 0.31
    for g in range(4):
        blk = np.arange(1024)
        base = np.nextafter(b0, 1.0) if g else b0
        vals = [base]
        for _ in range(767):
            vals.append(np.nextafter(vals[-1], 1.0))
        vals += [vals[0]] * 256                      # exact duplicates of the group's first
        beta[g * 1024 + blk] = vals
        b0 = vals[766]
    vh = np.full((ns, n), 0.55)
    bh = np.tile(beta, (ns, 1))
    v = torch.from_numpy(vh).cuda()
    b = torch.from_numpy(bh).cuda()
    prob = make_problem(0.2, -0.1, 0.4, 2, 3, 0, 0, 0.5, 0.35, 0.4)
    engine.rollout_argmin(prob, v, b, incumbent=INC_MAX, integrator=integ)
    got = engine.fetch()
    ref, costs, _ = oracle.rollout_argmin(prob, vh, bh, incumbent=INC_MAX,
                                          integ="qk21" if integ == "qk21" else "rect",
                                          want_costs=True)
    _same_choice(got, ref, costs)
    # an exact duplicate of an earlier candidate is never the winner
    first = {}
    for k in range(n):
        first.setdefault(bh[0, k], k)
    assert first[bh[0, got.index]] == got.index


def test_sharded_exchange_equals_single_launch(engine):
    """Config D emulated on one device: 8 contiguous shards (index_base) +
    the device all-reduce(min+index) selection == one launch over all."""
    from diplomjourney_amd.abi import RESULT_BYTES, make_problem
    from diplomjourney_amd.distributed import select_winner_host, shard_range
    from diplomjourney_amd.expansion import results_from_device
    n_cand, n_steps, world = 2_000_000, 12, 8
    V, B, v, b = _sampled(engine, n_cand, n_steps, seed=11)
    prob = make_problem(-0.3, 0.4, 2.0, 2, 3, 0, 0, 0.5, 1.0, 1.05)
    engine.rollout_argmin(prob, v, b, incumbent=INC_MAX, integrator="rect")
    single = engine.fetch()
    gathered = torch.empty(world * RESULT_BYTES, dtype=torch.uint8, device="cuda")
    for r in range(world):
        lo, hi = shard_range(n_cand, r, world)
        _, _, vs, bs = _sampled(engine, hi - lo, n_steps, seed=11, base=lo)
        engine.rollout_argmin(prob, vs, bs, index_base=lo, incumbent=INC_MAX, integrator="rect",
                              out=gathered[r * RESULT_BYTES:(r + 1) * RESULT_BYTES])
    out = torch.empty(RESULT_BYTES, dtype=torch.uint8, device="cuda")
    engine.select_winner(gathered, incumbent=INC_MAX, out=out)
    dev = engine.fetch(out)
    host = select_winner_host(results_from_device(gathered), incumbent=INC_MAX)
    assert dev.index == single.index == host.index
    assert dev.cost == single.cost and dev.trajectory() == single.trajectory()


def test_config_d_full_size_sharded_vs_oracle(engine, oracle):
    """Config D at its full size on one GPU: N = 12, 1e7 candidates in the 8
    contiguous shards of 8 ranks (index_base), each shard's winner from the
    bench's arithmetic (rect+cum), then the device all-reduce(min+index)
    selection over the 8 records — against the oracle's scan of every shard
    (reference arithmetic, glibc trig, 8 host threads) and its lexicographic
    minimum: same global index and control, states within 1e-9 — and the
    same global index as the oracle's scan in qk21, the reference's own
    arithmetic (identity, no tolerance; SURVEY §7 hard part 2)."""
    from concurrent.futures import ThreadPoolExecutor
    from diplomjourney_amd.abi import RESULT_BYTES, make_problem
    from diplomjourney_amd.distributed import shard_range
    n, ns, world = 10_000_000, 12, 8
    prob = make_problem(-0.3, 0.4, 2.0, 2, 3, 0, 0, 0.5, 1.0, 1.05)
    gathered = torch.empty(world * RESULT_BYTES, dtype=torch.uint8, device="cuda")
    futs, futq = [], []
    with ThreadPoolExecutor(max_workers=_threads()) as pool:
        for r in range(world):
            lo, hi = shard_range(n, r, world)
            _, _, vs, bs = _sampled(engine, hi - lo, ns, seed=13, base=lo)
            engine.rollout_argmin(prob, vs, bs, index_base=lo, incumbent=INC_MAX,
                                  integrator="rect+cum",
                                  out=gathered[r * RESULT_BYTES:(r + 1) * RESULT_BYTES])
            vh, bh = vs.cpu().numpy(), bs.cpu().numpy()
            del vs, bs
            futs.append(pool.submit(oracle.rollout_argmin, prob, vh, bh, index_base=lo,
                                    incumbent=INC_MAX, integ="rect", want_costs=True))
            futq.append(pool.submit(oracle.rollout_argmin, prob, vh, bh, index_base=lo,
                                    incumbent=INC_MAX, integ="qk21"))
        refs = [f.result() for f in futs]
        refq = [f.result()[0] for f in futq]
    out = torch.empty(RESULT_BYTES, dtype=torch.uint8, device="cuda")
    engine.select_winner(gathered, incumbent=INC_MAX, out=out)
    got = engine.fetch(out)
    q = min(refq, key=lambda x: (x.cost, x.index))
    assert got.index == q.index and (got.v, got.beta) == (q.v, q.beta), (got.index, q.index)
    assert math.isclose(got.cost, q.cost, rel_tol=COST_RTOL)
    best = min(range(world), key=lambda r: (refs[r][0].cost, refs[r][0].index))
    ref = refs[best][0]
    _report("config_d_full_size_sharded", candidates=n, horizon=ns, shards=world,
            identity_vs_qk21=1, rel_cost_diff_vs_qk21=abs(got.cost - q.cost) / abs(q.cost),
            near_tie_branch_vs_rect=int(got.index != ref.index))
    if got.index != ref.index:           # only a near-tie below the ulp noise
        lo_g = shard_range(n, 0, world)[1]
        costs = {r: refs[r][1] for r in range(world)}
        r_got = next(r for r in range(world) if shard_range(n, r, world)[0] <= got.index
                     < shard_range(n, r, world)[1])
        c_got = costs[r_got][got.index - shard_range(n, r_got, world)[0]]
        gap = abs(c_got - ref.cost) / abs(ref.cost)
        assert gap < 1e-13, (got.index, ref.index, gap, lo_g)
    else:
        assert (got.v, got.beta, got.found) == (ref.v, ref.beta, 1)
        _close_traj(got, ref, ns)
        assert math.isclose(got.cost, ref.cost, rel_tol=COST_RTOL)


def test_exchange_chain_two_ranks_on_one_gpu(engine, tmp_path):
    """The multi-GPU chained exchange (mpc_episode_exchange_step: one launch
    per rank and step + one all_gather of the 536-B candidates; flush by
    mpc_episode_exchange_flush) rehearsed with 2 gloo ranks sharing this GPU
    (two child processes): both ranks log exactly the steps of one rank
    running the single-GPU chained episode over all the candidates, restarts
    and the final global winner included."""
    _run_two_ranks(engine, tmp_path, "gather")


def _run_two_ranks(engine, tmp_path, mode, delay_s=0.0):
    import json
    import os
    import socket
    import subprocess
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    n_total, ns, steps, world = 60_000, 10, 70, 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    logs = [open(tmp_path / f"rank{r}.log", "wb") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(repo, "tests", "dist_rank.py"),
                               str(r), str(world), str(port), str(n_total), str(ns), str(steps),
                               str(tmp_path / f"rank{r}.json"), mode, str(delay_s)], env=env,
                              stdout=logs[r], stderr=subprocess.STDOUT)
             for r in range(world)]
    import time
    t_end = time.time() + 150
    while time.time() < t_end and any(p.poll() is None for p in procs):
        time.sleep(0.2)
    hung = [r for r, p in enumerate(procs) if p.poll() is None]
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
    for fh in logs:
        fh.close()
    outs = [open(tmp_path / f"rank{r}.log", "rb").read() for r in range(world)]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert not hung and p.returncode == 0, (f"rank {r} rc {p.returncode} hung {hung}:\n"
                                               + o.decode(errors="replace")[-3000:])
    ranks = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n_total, ns, 4100 + i) for i in range(4)]
    one = DeviceEpisode(engine, n_total, ns, integrator="rect+cum", chain=True, log_capacity=256,
                        max_steps=40)
    for i in range(steps):
        one.step(controls=pool[i % 4])
    one.flush()
    want = [[r.step, r.index, r.cost, r.x, r.y, r.phi, r.v, r.beta, r.p, r.episode, r.status]
            for r in one.read_log()]
    assert len(want) == steps and len({w[9] for w in want}) >= 2      # a restart inside
    for rk in ranks:
        assert rk["chain_error"] == 0
        assert rk["log"] == want
    assert ranks[0]["winner"] == ranks[1]["winner"] == one.local.cpu().tolist()
    return ranks


def test_c_host_exchange_episode(engine, tmp_path):
    """A C++ host with no Python (tests/c_host/exchange_episode.cpp): one
    process, an RCCL clique of the visible GPUs (here 1) from
    mpc_comm_init_all, per MPC step mpc_episode_exchange_step on every GPU and
    one grouped all_gather (mpc_exchange_allgather_group); flushed by
    mpc_episode_exchange_flush.  Its episode log and final winner equal, byte
    for byte, the single-GPU chained episode driven from Python."""
    import ctypes
    import os
    import struct
    import subprocess
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import native
    from diplomjourney_amd.abi import LOG_BYTES, RESULT_BYTES
    from diplomjourney_amd.episode import DeviceEpisode, reference_episode_config
    n_total, ns, steps, seed0 = 40_000, 10, 60, 4200
    cfg = reference_episode_config(max_steps=40)
    V, B = mmt.vector_of_velocities(0.5), mmt.vector_of_beta_angles(0.0)
    blob = (struct.pack("<6i", 1, ns, steps, len(V), len(B), 0) + struct.pack("<qQ", n_total, seed0)
            + bytes(cfg) + struct.pack(f"<{len(V)}d", *V) + struct.pack(f"<{len(B)}d", *B))
    (tmp_path / "in.bin").write_bytes(blob)
    assert os.path.exists(native.C_HOST_BIN), "built by __graft_entry__.build()"
    r = subprocess.run([native.C_HOST_BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = (tmp_path / "out.bin").read_bytes()
    Vd = torch.tensor(V, dtype=torch.float64, device="cuda")
    Bd = torch.tensor(B, dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(Vd, Bd, n_total, ns, seed0 + k) for k in range(4)]
    one = DeviceEpisode(engine, n_total, ns, integrator="rect+cum", chain=True, log_capacity=256,
                        max_steps=40)
    for i in range(steps):
        one.step(controls=pool[i % 4])
    one.flush()
    want = b"".join(bytes(rec) for rec in one.read_log())
    assert len(want) == steps * LOG_BYTES
    assert len({rec.episode for rec in one.read_log()}) >= 2         # a restart inside
    assert out[:steps * LOG_BYTES] == want
    assert out[steps * LOG_BYTES:steps * LOG_BYTES + RESULT_BYTES] == bytes(one.local.cpu().numpy())


def test_ties_resolve_to_lowest_index(engine):
    from diplomjourney_amd.abi import make_problem
    prob = make_problem(0, 0, 0, 2, 3, 0, 0, 0.5, 0.05, 0.1)
    n, ns = 700_000, 4
    v = torch.full((ns, n), 0.6, dtype=torch.float64, device="cuda")
    b = torch.full((ns, n), 0.2, dtype=torch.float64, device="cuda")
    engine.rollout_argmin(prob, v, b, incumbent=INC_MAX, integrator="rect")
    assert engine.fetch().index == 0                     # all identical -> first
    gen = torch.Generator(device="cpu").manual_seed(3)
    v = (torch.rand((ns, n), generator=gen, dtype=torch.float64) * 0.9).cuda()
    b = ((torch.rand((ns, n), generator=gen, dtype=torch.float64) - 0.5) * 2).cuda()
    engine.rollout_argmin(prob, v, b, incumbent=INC_MAX, integrator="rect")
    best = engine.fetch().index
    # positions across lane pairs, wave tiles (128), block tiles (512) and
    # the launch's last, partial tile (700_000 = 1367 full tiles + 96)
    for dup_at in (best + 1 if best + 1 < n else best - 1, 1, 127, 128, 129, 255, 256, 511, 512,
                   1023, 1024, 699_391, 699_392, 699_393, n - 1, 0):
        v2, b2 = v.clone(), b.clone()
        v2[:, dup_at], b2[:, dup_at] = v[:, best], b[:, best]
        engine.rollout_argmin(prob, v2, b2, incumbent=INC_MAX, integrator="rect")
        assert engine.fetch().index == min(best, dup_at)


def test_nonfinite_and_incumbent(engine):
    from diplomjourney_amd.abi import make_problem
    prob = make_problem(0, 0, 0, 2, 3, 0, 0, 0.5, 0.05, 0.1)
    n, ns = 10_000, 3
    gen = torch.Generator(device="cpu").manual_seed(5)
    v = (torch.rand((ns, n), generator=gen, dtype=torch.float64)).cuda()
    b = ((torch.rand((ns, n), generator=gen, dtype=torch.float64) - 0.5) * 2).cuda()
    engine.rollout_argmin(prob, v, b, integrator="rect")
    base = engine.fetch()
    v2 = v.clone()
    v2[1, base.index] = float("nan")                      # the best turns NaN: never wins
    engine.rollout_argmin(prob, v2, b, integrator="rect")
    assert engine.fetch().index != base.index
    engine.rollout_argmin(prob, torch.full_like(v, float("nan")), b, integrator="rect")
    none = engine.fetch()
    assert (none.index, none.found) == (-1, 0) and none.cost == math.inf
    engine.rollout_argmin(prob, v, b, incumbent=base.cost, integrator="rect")   # strict <
    same = engine.fetch()
    assert (same.found, same.index, same.cost) == (0, base.index, base.cost)
    engine.rollout_argmin(prob, v, b, incumbent=math.nextafter(base.cost, math.inf),
                          integrator="rect")
    assert engine.fetch().found == 1


def test_batched_robots_vs_oracle(engine, oracle):
    """Config E shape at test size: R robots, segmented per-robot arg-min."""
    from diplomjourney_amd.abi import make_problem
    from diplomjourney_amd.expansion import problems_to_device, results_from_device
    rng = np.random.default_rng(20261015)
    for R, cand, ns in ((64, 2000, 8), (7, 1001, 3), (3, 5000, 12)):
        probs = []
        for _ in range(R):
            x0, y0 = rng.uniform(-10, 10, 2)
            probs.append(make_problem(x0, y0, rng.uniform(-math.pi, math.pi),
                                      x0 + rng.uniform(-10, 10), y0 + rng.uniform(-10, 10),
                                      x0, y0, 0.5, 0.05, 0.1))
        V, B = _grid451()
        v = torch.empty((ns, R * cand), dtype=torch.float64, device="cuda")
        b = torch.empty_like(v)
        for r in range(R):
            engine.sample_controls(_dev(V), _dev(B), cand, ns, 20261015 + r,
                                   v_out=v[:, r * cand:], beta_out=b[:, r * cand:], ld=R * cand)
        inc = rng.uniform(1e3, 1e9, R)
        out = engine.rollout_argmin_batched(problems_to_device(probs, "cuda"), v, b, cand,
                                            incumbents_dev=_dev(inc), integrator="rect")
        got = results_from_device(out)
        ref = oracle.rollout_argmin_batched(probs, v.cpu().numpy(), b.cpu().numpy(), cand,
                                            incumbents=inc, integ="rect")
        for g, o in zip(got, ref):
            assert (g.index, g.found) == (o.index, o.found)
            assert math.isclose(g.cost, o.cost, rel_tol=COST_RTOL)
            _close_traj(g, o, ns)


def test_full_size_config_e_batched(engine, oracle):
    """Config E at its full size, built as bench.py builds it (1024 robots x
    1e4 candidates, N=8, per-robot PCG64 problems and sampler seeds), in the
    bench's rect+rot mode: every robot's winner equals the host replica of the
    kernel's arithmetic, its cost and trajectory to within ulps; and for a
    sample of robots the oracle (reference arithmetic, rect) picks the same
    candidate.  (Not bitwise: the batched kernel derives each robot's
    constants on the device — sin/cos of the start heading with the kernel's
    own sincos, squares as x*x — where the replica, like the single-problem
    host path, takes libm's; robot 527's winner, for one, lands 1 ulp apart
    in one coordinate.)"""
    from harness import replica_rollout
    from diplomjourney_amd.abi import make_problem
    from diplomjourney_amd.expansion import problems_to_device, results_from_device
    R, cand, ns = 1024, 10_000, 8
    probs = []
    for r in range(R):
        g = np.random.default_rng(20261015 + r)
        x0, y0 = g.uniform(-10, 10, 2)
        phi0 = g.uniform(-math.pi, math.pi)
        xt, yt = g.uniform(x0 - 10, x0 + 10), g.uniform(y0 - 10, y0 + 10)
        probs.append(make_problem(x0, y0, phi0, xt, yt, x0, y0, 0.5, 0.05, 0.1))
    V, B = _grid451()
    v = torch.empty((ns, R * cand), dtype=torch.float64, device="cuda")
    b = torch.empty_like(v)
    for r in range(R):
        engine.sample_controls(_dev(V), _dev(B), cand, ns, 20261015 + r,
                               v_out=v[:, r * cand:], beta_out=b[:, r * cand:], ld=R * cand)
    out = engine.rollout_argmin_batched(problems_to_device(probs, "cuda"), v, b, cand,
                                        integrator="rect+rot")
    got = results_from_device(out)
    vh, bh = v.cpu().numpy(), b.cpu().numpy()
    exact = 0
    for r in range(R):
        cols = slice(r * cand, (r + 1) * cand)
        st, costs = replica_rollout(probs[r], vh[:, cols], bh[:, cols], "rect+rot",
                                    device_estimates=True)
        k = int(np.argmin(costs))
        g = got[r]
        if g.index != k:     # only a near-tie below the constants' ulp noise
            assert abs(costs[g.index] - costs[k]) <= 1e-13 * abs(costs[k]), r
            continue
        assert math.isclose(g.cost, costs[k], rel_tol=1e-14), r
        d = np.abs(np.array(g.trajectory()) - st[:, :, k]).max()
        assert d <= 1e-13, (r, d)
        exact += g.trajectory() == [list(st[s, :, k]) for s in range(ns)]
    assert exact >= R // 2       # most winners still bit-identical to the replica
    sample = list(range(0, R, 64))
    ref = oracle.rollout_argmin_batched([probs[r] for r in sample],
                                        np.concatenate([vh[:, r * cand:(r + 1) * cand]
                                                        for r in sample], axis=1),
                                        np.concatenate([bh[:, r * cand:(r + 1) * cand]
                                                        for r in sample], axis=1),
                                        cand, integ="rect")
    for r, o in zip(sample, ref):
        assert got[r].index == o.index, r
        _close_traj(got[r], o, ns)


def test_states_out_vs_oracle(engine, oracle):
    from diplomjourney_amd.abi import make_problem
    n, ns = 5003, 6
    V, B, v, b = _sampled(engine, n, ns, seed=3)
    prob = make_problem(1.0, 2.0, -0.7, 2, 3, 0.5, 0.5, 0.5, 0.05, 0.1)
    states = torch.empty((ns, 3, n), dtype=torch.float64, device="cuda")
    engine.rollout_argmin(prob, v, b, integrator="qk21", states=states)
    _, _, ref = oracle.rollout_argmin(prob, v.cpu().numpy(), b.cpu().numpy(), integ="qk21",
                                      want_states=True)
    assert np.abs(states.cpu().numpy() - ref).max() <= STATE_TOL


def test_two_phase_api_matches(engine):
    from diplomjourney_amd.abi import make_problem
    V, B, v, b = _sampled(engine, 300_000, 10, seed=21)
    prob = make_problem(0, 0, 0.2, 2, 3, 0, 0, 0.5, 0.05, 0.1)
    engine.rollout_argmin(prob, v, b, integrator="rect")
    one = engine.fetch()
    engine.partials(prob, v, b, integrator="rect")
    engine.finalize(prob, v, b, integrator="rect")
    two = engine.fetch()
    assert bytes(one) == bytes(two)


@pytest.mark.parametrize("split", [False, True])
def test_device_episode_matches_host_episode(engine, split):
    """The device-resident episode (mpc_episode_*: grid, sampler, problem,
    finishing logic, stuck detector and operator events in HBM, no host sync)
    makes the same choices as the host-driven episode over 200 MPC steps incl.
    the p = 60 / 90 / 110 operator events — with the selection run by the last
    block of the rollout launch (fused) or by its own kernel (split)."""
    from diplomjourney_amd.episode import DeviceEpisode, Episode
    n, ns, steps = 20_000, 10, 200
    host = Episode(engine, n, ns)
    want = []
    for _ in range(steps):
        host.step()
        want.append(host.last_log)
    dev = DeviceEpisode(engine, n, ns, log_capacity=512, split=split)
    for _ in range(steps):
        dev.step()
    got = dev.read_log()
    assert len(got) == steps
    for g, w in zip(got, want):
        assert (g.index, g.p, g.found, g.status) == (w[0], w[2], w[8], w[9])
        assert math.isclose(g.cost, w[1], rel_tol=COST_RTOL)
        assert max(abs(a - b) for a, b in zip((g.x, g.y, g.phi, g.v, g.beta), w[3:8])) <= STATE_TOL
    assert max(w[2] for w in want) > 110          # the operator events were exercised


def _scenario_episode_log(engine, calls, integrator, n_cand=452):
    """The device loop in the reference's configuration, one step per call."""
    from diplomjourney_amd.episode import DeviceEpisode
    ep = DeviceEpisode(engine, n_cand, 3, integrator=integrator, log_capacity=512,
                       enumerate=True, incumbent0=10000050990.195135)
    for _ in range(calls):
        ep.step()
    return ep.read_log()


@pytest.mark.parametrize("integ", ["qk21", "rect+rot"])
def test_device_episode_replays_reference_scenario(engine, scenario, integ):
    """The device-resident math_mpc loop (mpc_episode_*: grids, slow-down,
    enumeration, rollout, selection, finishing logic, stuck detector, operator
    events, all in HBM, no host round trip) in the reference's configuration
    — N = 3, the step's |V| x |B| constant sequences as the candidate set
    (padding to 452 masked), the first incumbent of :676 — reproduces the
    reference's model run (math_model_tree.py:736, calls 0-150): every
    chosen (v, beta) identical, every returned pose within 1e-6, the events at
    p = 60 / 90 / 110 and the arrival after call 150."""
    from diplomjourney_amd.abi import MPC_EP_ARRIVED, MPC_EP_EVENT
    calls = [c for c in scenario["calls"] if not c["isActual"]]
    assert len(calls) == 151
    log = _scenario_episode_log(engine, len(calls), integ)
    assert len(log) == len(calls)
    worst = 0.0
    for i, (rec, g) in enumerate(zip(calls, log)):
        assert (g.p, g.episode, g.found) == (i + 1, 1, int(rec["found"]))
        assert (g.v, g.beta) == tuple(rec["ret"][3:5]), i
        worst = max(worst, max(abs(a - b) for a, b in zip((g.x, g.y, g.phi), rec["ret"][:3])))
        V, B = rec["V"], rec["B"]
        if rec["pre"]["steps_for_slowing"] > 0:                 # :312-316
            V = [min(V) if min(V) > 0.4 else 0.4] * len(V)
        first = next(k for k in range(len(V) * len(B))          # lowest index of the control
                     if (V[k // len(B)], B[k % len(B)]) == (g.v, g.beta))
        assert g.index == first, i
        want = MPC_EP_EVENT if g.p in (60, 90, 110) else 0
        want |= MPC_EP_ARRIVED if i == len(calls) - 1 else 0
        assert g.status == want, (i, g.status)
    assert worst <= 1e-6, worst
def test_device_episode_stuck_detector_vs_drop_in(engine):
    """A target behind the robot: after one forced move (the line-origin
    sentinel makes staying at the start cost 1e10) staying still is optimal,
    the pose repeats (recursive = True, :562-563) and the next step ends the
    episode with "Recursive error" (:559-561).  The device loop logs the same
    three steps as the drop-in math_mpc (chosen control, pose, p), marks them
    stuck / break, and restarts the episode after the break."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.abi import MPC_EP_BREAK, MPC_EP_STUCK
    from diplomjourney_amd.episode import DeviceEpisode
    mmt.reset_state()
    inc0 = mmt.optimal_criterion
    seen = []
    try:
        mmt.math_mpc([0, 0, 0, 0, 0], [-2, 0], False, on_step=lambda p, c: seen.append((p, c)))
        assert mmt.recursive
    finally:
        mmt.reset_state()
    assert [p for p, _ in seen] == [1, 2, 3]
    ep = DeviceEpisode(engine, 452, 3, integrator="qk21", log_capacity=16, target=(-2, 0),
                       enumerate=True, incumbent0=inc0)
    for _ in range(4):
        ep.step()
    log = ep.read_log()
    for (p, c), g, st in zip(seen, log, (0, MPC_EP_STUCK, MPC_EP_BREAK)):
        assert (g.p, g.episode, g.status, g.found) == (p, 1, st, 1)
        assert (g.v, g.beta) == (c[3], c[4])
        assert max(abs(a - b) for a, b in zip((g.x, g.y, g.phi), c[:3])) <= 1e-6
    assert (log[3].p, log[3].episode) == (1, 2)        # the ended episode restarted


def test_device_episode_stale_without_winner(engine):
    """No candidate beats the incumbent (incumbent0 below every cost): the
    step keeps the stale optimal_trajectory — before any winner, the pose
    itself (the reference's [[[0]]] has no layers to return) — so the pose
    repeats (stuck); the next step finds a winner but ends the episode
    (recursive was set).  The host-driven Episode applies the same update."""
    from diplomjourney_amd.abi import MPC_EP_BREAK, MPC_EP_STALE, MPC_EP_STUCK
    from diplomjourney_amd.episode import DeviceEpisode
    ep = DeviceEpisode(engine, 452, 3, integrator="qk21", log_capacity=16, enumerate=True,
                       incumbent0=1.0)
    for _ in range(3):
        ep.step()
    a, b, c = ep.read_log()
    assert (a.found, a.index, a.status, a.p) == (0, -1, MPC_EP_STALE | MPC_EP_STUCK, 1)
    assert (a.x, a.y, a.phi, a.v, a.beta) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert (b.found, b.status, b.p, b.episode) == (1, MPC_EP_BREAK, 2, 1)
    assert (c.p, c.episode) == (1, 2)


@pytest.mark.parametrize("integ", ["rect+rot", "qk21", "rect", "qk21+rot"])
def test_device_episode_resident_controls(engine, integ):
    """Device episode over caller-resident candidate batches (the bench's
    default input mode: no sampler launch, the step's problem prepared by the
    previous advance).  Every step's winner equals the plain C-ABI arg-min of
    the same batch on the problem rebuilt on the host from the previous
    logged state, and the partial records of the device-constants (KDEV)
    kernel equal those of the by-value kernel."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.abi import make_problem
    from diplomjourney_amd.episode import DeviceEpisode
    n, ns, steps = 50_000, 10, 6
    dev = DeviceEpisode(engine, n, ns, integrator=integ, log_capacity=64)
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 77 + i) for i in range(steps)]
    x = y = phi = 0.0
    t, dt = 0.0, mmt.delta_t
    for i in range(steps):
        t = t + dt
        prob = make_problem(x, y, phi, 2, 3, 0, 0, mmt.L, t, t + dt)
        inc = 10000 * math.sqrt(13) + 10000 * 1000 ** 2 if i == 0 else INC_MAX
        dev.cur = pool[i]
        dev.partials()                               # KDEV records of this batch ...
        kdev = dev.ws.clone()
        dev.step(controls=pool[i])
        ref = engine.fetch(engine.rollout_argmin(prob, *pool[i], incumbent=inc,
                                                 integrator=integ))
        log = dev.read_log()[-1]
        assert log.index == ref.index and ref.found == 1
        assert math.isclose(log.cost, ref.cost, rel_tol=COST_RTOL)
        engine.partials(prob, *pool[i], integ)       # ... equal the by-value kernel's
        n_rec = -(-n // 512)                         # blocks of the CPL = 2 launch
        a = kdev.view(torch.int64)[:2 * n_rec].cpu()
        b = engine._workspace(engine.lib.mpc_workspace_bytes(n, ns)).view(torch.int64)[:2 * n_rec].cpu()
        idx_a, idx_b = a[1::2], b[1::2]
        assert torch.equal(idx_a, idx_b)
        x, y, phi = log.x, log.y, log.phi


def test_device_episode_exchange_path_and_graph_capture(engine):
    """The multi-GPU step structure (finalize -> RCCL all_gather -> advance)
    over a 1-rank nccl group, launched eagerly and replayed from a HIP graph
    that captures the collective, logs exactly the steps of the single-GPU
    episode (finalize applies the update itself) on the same resident batches."""
    import torch.distributed as dist
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    n, ns, steps = 40_000, 10, 12
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 900 + i) for i in range(steps)]
    ref = DeviceEpisode(engine, n, ns, log_capacity=64)
    for i in range(steps):
        ref.step(controls=pool[i])
    want = [(r.step, r.index, r.cost, r.x, r.y, r.phi, r.v, r.beta) for r in ref.read_log()]
    own = not dist.is_initialized()
    if own:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                                world_size=1, device_id=torch.device("cuda", 0))
    try:
        eager = DeviceEpisode(engine, n, ns, log_capacity=64, exchange=True)
        half = steps // 2
        for i in range(half):                      # eager (also creates the communicator)
            eager.step(controls=pool[i])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                  # the rest captured, collective included
            for i in range(half, steps):
                eager.step(controls=pool[i])
        g.replay()
        torch.cuda.synchronize()
        got = [(r.step, r.index, r.cost, r.x, r.y, r.phi, r.v, r.beta) for r in eager.read_log()]
        assert got == want
    finally:
        if own:
            dist.destroy_process_group()


def _episode_log(ep):
    return [(r.step, r.index, r.cost, r.x, r.y, r.phi, r.v, r.beta, r.p, r.episode)
            for r in ep.read_log()]


@pytest.mark.parametrize("wheelbase,n,ns", [(0.5, 50_000, 10), (0.45, 50_000, 10),
                                            (0.5, 100_000, 3), (0.45, 100_000, 3)])
def test_chained_episode_matches_separate_launches(engine, wheelbase, n, ns):
    """Chained steps (mpc_episode_chain_step: step k's rollout and step k-1's
    finalize + episode update in ONE launch, the tile blocks waiting on device
    for block 0's published constants) log exactly the steps of the
    two-launch device episode over 130 steps of resident batches — operator
    events at p = 60/90/110 included — eagerly and replayed from a HIP graph
    whose last launch is the flush; a launch whose last tile is partial
    (50_000 = 97 tiles of 512 + 336).  Both wheelbase forms of the chained
    kernel: L = 0.5 (a power of two, PL2) and L = 0.45 (v / L divided);
    N = 10 at 5e4 candidates and config B's shape (N = 3, 1e5)."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    integ = "rect+cum"
    steps = 130
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 500 + i) for i in range(8)]
    ref = DeviceEpisode(engine, n, ns, integrator=integ, log_capacity=256, L=wheelbase)
    for i in range(steps):
        ref.step(controls=pool[i % 8])
    want = _episode_log(ref)
    assert len(want) == steps and {r[8] for r in want} >= {60, 90, 110}
    ch = DeviceEpisode(engine, n, ns, integrator=integ, log_capacity=256, chain=True,
                       L=wheelbase)
    half = steps // 2
    for i in range(half):
        ch.step(controls=pool[i % 8])
    ch.flush()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    n0 = ch.steps_enqueued
    with torch.cuda.graph(g):
        for i in range(half, steps):
            ch.step(controls=pool[i % 8])
        ch.flush()
    ch.steps_enqueued = n0
    g.replay()
    ch.steps_enqueued += steps - half
    assert _episode_log(ch) == want
    assert ch.chain_error() == 0


def test_chained_episode_multi_tile_blocks(engine):
    """Chained steps when blocks stride over several tiles (1.1e6 candidates
    > 2048 blocks x 512) equal the two-launch episode."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    n, ns, steps = 1_100_000, 6, 5
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 700 + i) for i in range(steps)]
    ref = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=16)
    ch = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=16, chain=True)
    for i in range(steps):
        ref.step(controls=pool[i])
        ch.step(controls=pool[i])
    assert _episode_log(ch) == _episode_log(ref)
    assert ch.chain_error() == 0


@pytest.mark.parametrize("ns", [10, 3])
def test_chained_wheelbase_mismatch_is_flagged(engine, ns):
    """A chained launch whose cfg wheelbase form (power of two or not)
    differs from the state's constants sets chain error 2 instead of
    returning wrong costs silently."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    n = 20_000
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 40 + i) for i in range(2)]
    ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=16, chain=True)
    ep.step(controls=pool[0])
    ep.flush()
    assert ep.chain_error() == 0
    ep.cfg.L = 0.45                      # state reset with L = 0.5
    ep.step(controls=pool[1])
    ep.flush()
    assert ep.chain_error() == 2


@pytest.mark.parametrize("wheelbase,n,cap,overlap", [(0.5, 40_000, 6, False),
                                                     (0.45, 40_000, 6, False),
                                                     (0.5, 1_000_000, 1, False),
                                                     (0.5, 40_000, 6, True),
                                                     (0.5, 1_000_000, 3, True)])
def test_chained_exchange_path_and_graph_capture(engine, wheelbase, n, cap, overlap):
    """The chained multi-GPU step (launch: rollout of step k + selection over
    step k-1's gathered winners; then step k's local finalize and the RCCL
    all_gather) over a 1-rank nccl group, eager and graph-captured, logs the
    steps of the single-GPU episode; both wheelbase forms.  The graph (CAP
    captured steps) is replayed three times: a replay repeats its launches'
    epochs, so with one captured step the next replay passes only if no tagged
    record of the last one survives its consumption."""
    import torch.distributed as dist
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode, cu_reserved_stream
    ns, steps = 10, 12
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 900 + i) for i in range(steps)]
    half, reps = steps - cap, 3
    ref = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64, L=wheelbase)
    for i in list(range(steps)) + list(range(half, steps)) * (reps - 1):
        ref.step(controls=pool[i])
    want = _episode_log(ref)
    own = not dist.is_initialized()
    if own:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                                world_size=1, device_id=torch.device("cuda", 0))
    # the overlapped form launches (and replays) on a CU-reserved stream: the
    # collective beside each launch needs free CUs (1M candidates: the launch
    # is larger than one resident round)
    launch = cu_reserved_stream(torch.device("cuda", 0)) if overlap else torch.cuda.current_stream()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(launch):
            ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64,
                               exchange=True, chain=True, L=wheelbase, overlap=overlap)
            for i in range(half):
                ep.step(controls=pool[i])
            ep.flush()
        torch.cuda.synchronize()
        if overlap:
            # eager only: a replayed graph's branches lose the CU mask
            with pytest.raises(ValueError, match="eager"):
                with torch.cuda.graph(torch.cuda.CUDAGraph()):
                    ep.step(controls=pool[half])
            with torch.cuda.stream(launch):
                for i in list(range(half, steps)) * reps:
                    ep.step(controls=pool[i])
                    if i == steps - 1:
                        ep.flush()
        else:
            g = torch.cuda.CUDAGraph()
            n0 = ep.steps_enqueued
            with torch.cuda.graph(g):
                for i in range(half, steps):
                    ep.step(controls=pool[i])
                ep.flush()
            ep.steps_enqueued = n0
            for _ in range(reps):
                g.replay()
                ep.steps_enqueued += steps - half
        torch.cuda.synchronize()
        assert _episode_log(ep) == want
        assert ep.chain_error() == 0
    finally:
        if own:
            dist.destroy_process_group()


@pytest.mark.parametrize("wheelbase,n,cap", [(0.5, 40_000, 6), (0.45, 40_000, 6),
                                             (0.5, 1_000_000, 3)])
def test_p2p_exchange_one_rank_eager_and_graph(engine, wheelbase, n, cap):
    """The collective-free exchange (mpc_episode_p2p_step: block 0 posts the
    rank's candidate into every rank's mailbox and the next launch's block 0
    waits for them in its own) on one rank: eager steps, then a captured
    sequence (ending with mpc_episode_p2p_flush) replayed three times, log the
    steps of the single-GPU episode.  A replay repeats its launches' epochs,
    so it passes only if every consumed mailbox tag was cleared."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    ns, steps, reps = 10, 12, 3
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 1900 + i) for i in range(steps)]
    half = steps - cap
    ref = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64, L=wheelbase)
    for i in list(range(steps)) + list(range(half, steps)) * (reps - 1):
        ref.step(controls=pool[i])
    want = _episode_log(ref)
    ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64, exchange=True,
                       chain=True, L=wheelbase, p2p=True)
    try:
        for i in range(half):
            ep.step(controls=pool[i])
        ep.flush()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        n0 = ep.steps_enqueued
        with torch.cuda.graph(g):
            for i in range(half, steps):
                ep.step(controls=pool[i])
            ep.flush()
        ep.steps_enqueued = n0
        for _ in range(reps):
            g.replay()
            ep.steps_enqueued += steps - half
        torch.cuda.synchronize()
        assert _episode_log(ep) == want
        assert ep.chain_error() == 0
    finally:
        ep.close()


@pytest.mark.parametrize("wheelbase,n,ns", [(0.5, 100_000, 3), (0.45, 60_000, 10),
                                            (0.5, 1_000_000, 10), (0.5, 1_250_000, 12)])
def test_tiled_chained_episode_matches_soa(engine, wheelbase, n, ns):
    """MPC_LAYOUT_TILED (the bench's resident layout): the tiled sampler's
    candidates are the SoA sampler's, and the chained episode over tiled
    batches logs exactly the chained episode over the same SoA batches —
    70 steps with max_steps = 40 (a restart inside), both wheelbase forms, a
    ragged last tile (n % 512 != 0), config C's and D's sizes — with the same
    final result record."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    from diplomjourney_amd.expansion import tiled_to_soa
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    soa = [engine.sample_controls(V, B, n, ns, 900 + i) for i in range(4)]
    til = [engine.sample_controls_tiled(V, B, n, ns, 900 + i) for i in range(4)]
    for (v, b), t in zip(soa, til):
        v2, b2 = tiled_to_soa(t, n)
        assert torch.equal(v, v2) and torch.equal(b, b2)
    eps = [DeviceEpisode(engine, n, ns, integrator="rect+cum", chain=True, log_capacity=128,
                         max_steps=40, L=wheelbase) for _ in range(2)]
    for i in range(70):
        eps[0].step(controls=soa[i % 4])
        eps[1].step(controls=til[i % 4])
    logs = [_episode_log(e) for e in eps]
    assert logs[0] == logs[1] and len(logs[0]) == 70
    assert len({r[9] for r in logs[0]}) >= 2                     # a restart inside
    assert torch.equal(eps[0].local, eps[1].local)
    assert eps[1].chain_error() == 0


def test_tiled_p2p_one_rank_and_probe(engine):
    """Tiled controls through the P2P exchange form (one rank: eager steps,
    then a captured sequence of odd length replayed three times) log the
    single-GPU SoA episode; the tiled stream probe runs on the same batches."""
    import ctypes
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    from diplomjourney_amd.expansion import tiled_to_soa
    n, ns, steps, cap, reps = 300_000, 10, 12, 5, 3
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    til = [engine.sample_controls_tiled(V, B, n, ns, 2900 + i) for i in range(steps)]
    soa = [tiled_to_soa(t, n) for t in til]
    half = steps - cap
    ref = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64)
    for i in list(range(steps)) + list(range(half, steps)) * (reps - 1):
        ref.step(controls=soa[i])
    want = _episode_log(ref)
    ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64, exchange=True,
                       chain=True, p2p=True)
    try:
        for i in range(half):
            ep.step(controls=til[i])
        ep.flush()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        n0 = ep.steps_enqueued
        with torch.cuda.graph(g):
            for i in range(half, steps):
                ep.step(controls=til[i])
            ep.flush()
        ep.steps_enqueued = n0
        for _ in range(reps):
            g.replay()
            ep.steps_enqueued += steps - half
        torch.cuda.synchronize()
        assert _episode_log(ep) == want
        assert ep.chain_error() == 0
    finally:
        ep.close()
    sink = torch.empty(2048 * 256, dtype=torch.int64, device="cuda")
    from diplomjourney_amd import native
    native.check(native.lib().mpc_stream_probe_tiled(
        til[0].data_ptr(), n, ns, sink.data_ptr(), sink.numel() * 8,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mpc_stream_probe_tiled")
    torch.cuda.synchronize()


def test_p2p_exchange_two_ranks_on_one_gpu(engine, tmp_path):
    """The collective-free exchange with 2 ranks (two processes sharing this
    GPU; the mailboxes' IPC handles exchanged once over gloo, every step's
    candidates by the launches' own peer stores): both ranks log exactly the
    steps of one rank running the single-GPU chained episode over all the
    candidates, restarts and the final global winner included."""
    _run_two_ranks(engine, tmp_path, "p2p")


def test_p2p_exchange_with_a_lagging_rank(engine, tmp_path):
    """A rank that runs late (ranks are not barrier-aligned between
    steps): rank 1 holds its stream back ~0.3 s (a spinning kernel) before
    its 10th step, so rank 0's launches wait in block 0 for its candidate while
    their tile blocks wait for block 0.  The tiles' bound (3 s) outlasts block
    0's peer wait (2 s), so the lag is absorbed: both ranks log exactly the
    single-rank episode, chain_error 0 on both."""
    ranks = _run_two_ranks(engine, tmp_path, "p2p", delay_s=0.3)
    assert ranks[1]["held_ms"] > 200, ranks[1]["held_ms"]


def test_overlapped_exchange_with_a_late_collective(engine):
    """The overlapped exchange step (mpc_episode_exchange_step2): the
    all_gather of step k runs on a side stream beside launch k+1, whose block
    0 waits for the device-side mark.  Here every collective is held back ~1 ms
    (a spinning kernel in front of it on the side stream), so each launch's
    block 0 waits for the mark while its tiles stream: the episode still logs
    exactly the single-GPU chained episode, chain_error 0."""
    import torch.distributed as dist
    from diplomjourney_amd import distributed as D
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode, cu_reserved_stream
    n, ns, steps = 200_000, 10, 10
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    pool = [engine.sample_controls(V, B, n, ns, 1300 + i) for i in range(steps)]
    ref = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64, chain=True)
    for i in range(steps):
        ref.step(controls=pool[i])
    want = _episode_log(ref)
    own = not dist.is_initialized()
    if own:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                                world_size=1, device_id=torch.device("cuda", 0))
    orig = D.gather_into

    def late(out, local, group=None):
        torch.cuda._sleep(2_000_000)          # ~1 ms on the side stream, before the collective
        return orig(out, local, group)
    try:
        import diplomjourney_amd.device_episode as E
        E.gather_into = late
        torch.cuda.synchronize()
        with torch.cuda.stream(cu_reserved_stream(torch.device("cuda", 0))):
            ep = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=64,
                               exchange=True, chain=True, overlap=True)
            for i in range(steps):
                ep.step(controls=pool[i])
            ep.flush()
        torch.cuda.synchronize()
        assert _episode_log(ep) == want
        assert ep.chain_error() == 0
    finally:
        E.gather_into = orig
        if own:
            dist.destroy_process_group()


@pytest.mark.parametrize("extra", [[], ["--integrator", "rect+rot"]])
def test_bench_contract(extra):
    """bench.py --full (a short run, no CPU leg) prints ONE JSON line with the
    driver's contract keys; the default step is the chained rect+cum launch
    and its roofline is the chained kernel's, with the committed PMC traffic
    of that kernel; two-launch rect+rot reports the rollout kernel."""
    import json
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--steps", "8",
                        "--warmup", "2", "--cpu-seconds", "0", "--no-second-pass"] + extra,
                       capture_output=True, text=True, timeout=200, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2 and d["value"] > 0
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] < 1
    assert rf["algorithmic_bytes_per_launch"] == 16.0 * 10 * 1_000_000
    # the measured read ceiling of the kernel's own access
    # pattern beside the spec peak, the host-visible step latency, and the
    # kernel's VALU issue share from the committed PMC counters
    assert 2000 < rf["stream_ceiling_GBs"] < 9000 and 0 < rf["frac_of_stream_ceiling"] < 1.5
    assert 0 < d["p50_host_ms"] < 5
    assert 0 < rf["valu"]["fp64_issue_share"] < 1.5
    if extra:
        assert d["config"]["integrator"] == "rect+rot"
        assert rf["kernel"] == "k_rollout_argmin_stream"
    else:
        assert d["config"]["integrator"] == "rect+cum"
        assert rf["kernel"] == "k_episode_chain"
        assert d["config"]["step_launches"].startswith("chained")
        ro = d["roofline_rollout_only"]
        assert ro["kernel"] == "k_rollout_argmin_stream" and 0 < ro["frac"] < 1
        # every checker leg against the reference arithmetic (oracle qk21):
        # the episode through the reference's events and a restart, the
        # samplers, the S1 = 451 full tree, the device episode drivers
        par = d["parity"]
        assert par["pass"] and all(par["checks"].values()), par["checks"]
        assert par["steps"] == 116 and par["identity_rate"] == 1.0, par
        assert par["episode"]["events_at_p"] == [60, 90, 110] and par["episode"]["restarts"] >= 1
        assert par["max_abs_pose_diff"] <= 1e-9
        cd = d["config_d"]      # BASELINE config D's one-GPU share in the same run
        assert cd["chain_error"] == 0 and cd["config"]["candidates_per_gpu"] == 1_250_000
        assert cd["roofline"]["kernel"] == "k_episode_chain"
        assert cd["roofline"]["algorithmic_bytes_per_launch"] == 16.0 * 12 * 1_250_000
        ct = d["config_d_total"]   # config D as written: 1e7 in total (all on one GPU)
        assert ct["chain_error"] == 0 and ct["config"]["candidates_total"] == 10_000_000
        assert ct["roofline"]["algorithmic_bytes_per_launch"] == 16.0 * 12 * 10_000_000
        assert ct["scaling"] == "strong" and 0 < ct["roofline"]["frac"] < 1
        assert d["ramp"]["steps"] >= 300
    assert rf["traffic"] is not None and abs(rf["traffic"] / 160e6 - 1) < 0.01


@pytest.mark.parametrize("mode", ["p2p", "rccl"])
def test_bench_two_ranks_spawned(mode):
    """`python bench.py --gpus 2` with no launcher (the driver's own command
    form) runs TWO ranks — spawned by the GPU-free parent, here rehearsed
    with gloo on the one GPU — and rank 0's line says so: n_gpus 2, the
    exchange step, chain_error 0, and the roofline of the exchange form of the
    chained kernel (the launch that carries an N > 1 step)."""
    import json
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    # the driver's --full form (--steps 20 --warmup 5, second input pass, parity
    # check and config-D sub-result included); gloo and a smaller config-C
    # shard only because both ranks share this one GPU
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--full",
                        "--dist-backend", "gloo", "--candidates-per-gpu", "100000", "--steps", "20",
                        "--warmup", "5", "--exchange-mode", mode],
                       capture_output=True, text=True, timeout=300, cwd=repo, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["chain_error"] == 0 and d["value"] > 0
    assert d["config"]["candidates_total"] == 200_000 and d["scaling"] == "weak"
    if mode == "p2p":   # the mailboxes' self-test passed: no fallback
        assert "peer stores" in d["config"]["parallelism"]
        assert d["exchange"] == "mailbox peer stores"
    else:
        assert "all_gather(536 B candidates)" in d["config"]["parallelism"]
    rf = d["roofline"]
    kern = "k_episode_chain[p2p]" if mode == "p2p" else "k_episode_chain[exchange]"
    assert rf["kernel"] == kern and 0 < rf["frac"] < 1
    assert rf["algorithmic_bytes_per_launch"] == 16.0 * 10 * 100_000
    # the sampled second pass (expand + advance: the 808-B all_gather) ran
    assert d["other_inputs"]["inputs"] == "sampled" and d["other_inputs"]["value"] > 0
    # every checker leg against the reference arithmetic (oracle qk21), the
    # episode leg with the N > 1 schedule (events at p = 6 / 12 / 16, a restart)
    assert d["parity"]["pass"] and d["parity"]["identity_rate"] == 1.0, d["parity"]["checks"]
    assert d["parity"]["episode"]["events_at_p"] == [6, 12, 16]
    # config D as written: 1e7 candidates in total over the two ranks
    ct = d["config_d_total"]
    assert ct["chain_error"] == 0 and ct["value"] > 0
    assert ct["config"]["candidates_total"] == 10_000_000
    assert ct["config"]["candidates_per_gpu"] == 5_000_000
    # BASELINE config D in the same run: N=12, 1.25e6 per GPU, same step form
    cd = d["config_d"]
    assert cd["chain_error"] == 0 and cd["value"] > 0
    assert cd["config"]["n_steps"] == 12 and cd["config"]["candidates_total"] == 2_500_000
    assert cd["roofline"]["kernel"] == kern
    assert cd["roofline"]["algorithmic_bytes_per_launch"] == 16.0 * 12 * 1_250_000


def test_bench_workload_a_parity():
    """bench.py --workload A --full: the reference scenario through the drop-in,
    one JSON line with every recorded call's chosen control identical."""
    import json
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--workload", "A", "--full",
                        "--steps", "1", "--warmup", "0", "--cpu-seconds", "0"],
                       capture_output=True, text=True, timeout=200, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["parity"]["calls"] == 349 == d["parity"]["chosen_control_identical"]
    assert d["parity"]["max_abs_pose_diff"] <= 1e-6 and d["p50_ms"] > 0


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) times the K steps only — the line keeps the
    headline keys, every field that needs a pass of its own is null — and
    --dump-outputs writes what the timed steps returned: per step the log
    record, and the last step's winner record, identical from run to run
    (the ramp before the timed region is as long as the clock says, the
    episode restarts a fixed number of steps before the timed ones)."""
    import json
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, n, ns = 8, 20_000, 10
    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1",
                            "--steps", str(k), "--warmup", "2", "--candidates-per-gpu", str(n),
                            "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=200, cwd=repo)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["full"] is False and d["steps"] == k and d["dtype"] == "f64"
        assert d["unit"] == "rollouts/s" and d["higher_is_better"] is True
        assert d["ms_per_step"] > 0
        assert abs(d["value"] / (n / (d["ms_per_step"] * 1e-3)) - 1) < 1e-9
        for key in ("cpu_baseline", "roofline", "other_inputs", "generated_inputs", "p50_ms",
                    "p50_host_ms", "kernel_ms"):
            assert d[key] is None, key
        assert "parity" not in d and "config_d" not in d
        assert d["config"]["step_launches"].startswith("chained") and d["chain_error"] == 0
        dumps.append({f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == sorted(b) == ["step_cost", "step_index", "step_state", "step_status",
                                      "winner_control", "winner_cost", "winner_found",
                                      "winner_index", "winner_trajectory"]
    for name in a:
        assert a[name].dtype == np.float64
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert a["step_index"].shape == (k,) and a["step_state"].shape == (k, 5)
    assert a["winner_trajectory"].shape == (ns, 3)
    # the timed steps are steps K .. 2K-1 of the restarted episode
    assert a["step_status"][:, 0].tolist() == list(range(k, 2 * k))
    assert ((0 <= a["step_index"]) & (a["step_index"] < n)).all()
    # the winner record is the last step's: its candidate, cost and first state
    # (every step starts from the incumbent float(sys.maxsize), so a candidate
    # is found; 2K steps of at most v_max * 0.05 leave the robot far from the
    # target at distance 3.6, so the finishing logic returns layer 0)
    assert a["winner_found"][0] == 1 and a["winner_index"][0] == a["step_index"][-1]
    assert a["winner_cost"][0] == a["step_cost"][-1]
    assert np.array_equal(a["winner_control"], a["step_state"][-1, 3:])
    assert np.abs(a["winner_trajectory"][0] - a["step_state"][-1, :3]).max() <= 1e-12


@pytest.mark.parametrize("integ,n,L", [("rect+cum", 100_000, None), ("rect+rot", 100_000, None),
                                       ("qk21", 20_000, None), ("rect+cum", 1_100_000, 0.45)])
def test_generated_episode_matches_sampled(engine, integ, n, L):
    """Generated controls (mpc_episode_generate_step: grid + sampler fused into
    the rollout, candidates never in HBM) log exactly the steps of the sampled
    episode (mpc_episode_sample -> arrays -> rollout -> selection) over 150
    steps with the operator events and an episode restart, for the default
    integrators, a non-power-of-two wheelbase and several tiles per block; the
    final winner record (re-rolled trajectory included) is identical too."""
    from diplomjourney_amd.episode import DeviceEpisode
    ns, steps = 10, 150
    logs, outs = [], []
    for gen in (False, True):
        ep = DeviceEpisode(engine, n, ns, integrator=integ, log_capacity=256, L=L, generate=gen)
        ep.cfg.max_steps = 120            # forces an episode restart inside the run
        ep.reset()
        for _ in range(steps):
            ep.step()
        logs.append([bytes(r) for r in ep.read_log()])
        outs.append(ep.local.cpu().numpy().tobytes())
    assert len(logs[0]) == steps
    assert logs[1] == logs[0]
    assert outs[1] == outs[0]


def test_generated_step_arguments(engine):
    """mpc_episode_generate_step rejects odd candidate counts and a short
    workspace before launching; the largest grid (64 x 64 entries, 64 KiB of
    LDS) launches."""
    import ctypes
    from diplomjourney_amd import abi, native
    from diplomjourney_amd.episode import DeviceEpisode
    L = native.lib()
    ep = DeviceEpisode(engine, 1000, 10, integrator="rect+cum", generate=True)
    ep.step()                             # allocates the workspace
    wsb = L.mpc_episode_generate_workspace_bytes(1000, 10)
    assert wsb >= 16 and L.mpc_episode_generate_workspace_bytes(1, 10) == 0

    def call(n=1000, wsb=wsb, ratio=None):
        cfg = ep.cfg
        if ratio is not None:
            cfg = type(ep.cfg).from_buffer_copy(ep.cfg)
            cfg.ratio_v = cfg.ratio_beta = ratio
        return L.mpc_episode_generate_step(ctypes.byref(cfg), ep.state.data_ptr(), n, 10, 0,
                                           ep._integ, ep._gen_ws.data_ptr(), wsb,
                                           ep.local.data_ptr(), ep.log.data_ptr(), 16, None)

    assert call(n=999) == abi.MPC_ERR_ARG
    assert call(wsb=wsb - 1) == abi.MPC_ERR_WORKSPACE
    assert call(ratio=100.0) == abi.MPC_OK


def _pool(engine, n, ns, count, seed):
    from diplomjourney_amd import math_model_tree as mmt
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    return [engine.sample_controls(V, B, n, ns, seed + i) for i in range(count)]


def _two_launch_log(engine, n, ns, batches, wheelbase=None, cap=512, max_steps=None):
    from diplomjourney_amd.episode import DeviceEpisode
    ref = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=cap, L=wheelbase)
    if max_steps:
        ref.cfg.max_steps = max_steps
    for c in batches:
        ref.step(controls=c)
    return ref, _episode_log(ref)


@pytest.mark.parametrize("ns", [2, 3, 12])
def test_short_and_long_horizons_chain(engine, ns):
    """Horizons around the head prefetch three steps before a loop's end
    (none for N = 2, at the first step for N = 3) and the config-D length
    N = 12: the chained steps log exactly the two-launch rect+cum episode
    over 60 steps with a restart."""
    from diplomjourney_amd.episode import DeviceEpisode
    n, steps = 20_000, 60
    pool = _pool(engine, n, ns, 4, 900 + ns)
    batches = [pool[i % 4] for i in range(steps)]
    _, want = _two_launch_log(engine, n, ns, batches, max_steps=40)
    assert len({r[9] for r in want}) >= 2, "no episode restart exercised"
    ch = DeviceEpisode(engine, n, ns, integrator="rect+cum", log_capacity=512, chain=True)
    ch.cfg.max_steps = 40
    ch.reset()
    for c in batches:
        ch.step(controls=c)
    ch.flush()
    assert _episode_log(ch) == want
    assert ch.chain_error() == 0
