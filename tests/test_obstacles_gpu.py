"""Keep-out circles on the GPU (mpc_rollout_partials_obstacles /
mpc_rollout_argmin_obstacles and the Python layers over them) against the CPU
oracle: tests/obstacle_cases.py forms the blocked mask and the expected winner
from the oracle's states and costs."""
import math

import pytest

import obstacle_cases as oc
from diplomjourney_amd import abi

pytestmark = pytest.mark.gpu

_dev_cache = {}


def _dev(c):
    """The case's controls on the device (uploaded once per case)."""
    import torch
    key = id(c)
    if key not in _dev_cache:
        _dev_cache[key] = (c, torch.tensor(c.v).cuda(), torch.tensor(c.b).cuda())
    return _dev_cache[key][1:]


def _run(engine, c, mode, circles, states=None, counter=True):
    """(MpcResult, raw 808 bytes, n_blocked or None) of one obstacle call."""
    import torch
    v, b = _dev(c)
    nb = torch.full((1,), -7, dtype=torch.int64, device=engine.device) if counter else None
    out = engine.rollout_argmin(c.problem, v, b, integrator=mode, states=states,
                                obstacles=circles, n_blocked=nb)
    res = engine.fetch(out)
    raw = out.cpu().numpy().tobytes()
    return res, raw, (int(nb.item()) if counter else None)


def _check_winner(res, n_blocked, c):
    assert n_blocked == c.n_blocked                     # exactly the oracle's count
    assert res.index == c.index and res.found == 1
    assert math.isclose(res.cost, c.cost, rel_tol=1e-12), (res.cost, c.cost)


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_steps", [1, 3, 10])
@pytest.mark.parametrize("n_cand", [2178, 2177, 130])
def test_mask_and_winner(engine, oracle, n_cand, n_steps, mode):
    """2178: four blocks and a partial wave on the LDS-DMA ring path; 2177: the
    one-candidate-per-lane path; N = 10 wraps the 3-slot ring, N = 1 never
    refills it."""
    c = oc.case(n_cand, n_steps, oc.ORACLE_OF[mode])
    oc.check_preconditions(c)
    res, _, nb = _run(engine, c, mode, c.circles)
    _check_winner(res, nb, c)


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_cand", [2178, 2177])
def test_no_obstacles_is_the_plain_call(engine, oracle, n_cand, mode):
    """n_obstacles = 0, and a circle nothing reaches: mpc_rollout_argmin's
    record byte for byte, nothing blocked."""
    c = oc.case(n_cand, 3, oc.ORACLE_OF[mode])
    v, b = _dev(c)
    plain = engine.rollout_argmin(c.problem, v, b, integrator=mode).cpu().numpy().tobytes()
    assert len(plain) == 808
    _, raw0, nb0 = _run(engine, c, mode, [])
    assert raw0 == plain and nb0 == 0
    _, raw1, nb1 = _run(engine, c, mode, [c.circles[2]])
    assert raw1 == plain and nb1 == 0


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_cand", [2178, 2177])
def test_all_blocked(engine, oracle, n_cand, mode):
    c = oc.case(n_cand, 3, oc.ORACLE_OF[mode])
    res, _, nb = _run(engine, c, mode, [(oc.POSE[0], oc.POSE[1], 10.0)])
    assert res.index == -1 and res.found == 0 and nb == n_cand
    assert res.cost == math.inf


@pytest.mark.parametrize("mode", ["rect+rot", "rect+cum"])
def test_irregular_candidate(engine, oracle, mode):
    """A candidate with beta = 1.2 at step 0 is recomputed by step_safe; the
    circle on its state after step 2 must block it there as well."""
    c = oc.case(130, 3, oc.ORACLE_OF[mode], irregular=True)
    oc.check_preconditions(c)
    res, _, nb = _run(engine, c, mode, c.circles)
    _check_winner(res, nb, c)
    # without circle (d) the irregular candidate is free (and whoever else (d) blocked)
    free = oc.blocked_mask(c.states, c.circles[:3])
    assert not free[c.irr] and free.sum() < c.n_blocked
    _, _, nb3 = _run(engine, c, mode, c.circles[:3])
    assert nb3 == int(free.sum())


def test_states_variant(engine, oracle):
    import torch
    c = oc.case(2177, 3, "qk21")
    oc.check_preconditions(c)
    v, b = _dev(c)
    s_plain = torch.zeros((3, 3, c.n_cand), dtype=torch.float64, device=engine.device)
    s_obs = torch.full_like(s_plain, -1.0)
    engine.rollout_argmin(c.problem, v, b, integrator="qk21", states=s_plain)
    res, _, nb = _run(engine, c, "qk21", c.circles, states=s_obs)
    assert torch.equal(s_plain.view(torch.int64), s_obs.view(torch.int64))
    _check_winner(res, nb, c)


@pytest.mark.parametrize("mode", oc.MODES)
def test_shards(engine, oracle, mode):
    """Two partials_obstacles + finalize calls over the halves, then
    mpc_select_winner: the single call's result."""
    import torch
    c = oc.case(2178, 3, oc.ORACLE_OF[mode])
    oc.check_preconditions(c)
    single, _, nb = _run(engine, c, mode, c.circles)
    v, b = _dev(c)
    half = c.n_cand // 2
    gathered = torch.zeros(2 * abi.RESULT_BYTES, dtype=torch.uint8, device=engine.device)
    counts = torch.zeros(2, dtype=torch.int64, device=engine.device)
    for r, (lo, hi) in enumerate([(0, half), (half, c.n_cand)]):
        vs, bs = v[:, lo:hi].contiguous(), b[:, lo:hi].contiguous()
        engine.partials(c.problem, vs, bs, mode, obstacles=c.circles, n_blocked=counts[r:r + 1])
        engine.finalize(c.problem, vs, bs, index_base=lo, integrator=mode,
                        out=gathered[r * abi.RESULT_BYTES:(r + 1) * abi.RESULT_BYTES])
    got = engine.fetch(engine.select_winner(gathered))
    assert int(counts.sum().item()) == nb == c.n_blocked
    assert (got.index, got.found, got.cost, got.v, got.beta, got.n_steps) == \
        (single.index, single.found, single.cost, single.v, single.beta, single.n_steps)
    assert got.trajectory() == single.trajectory()


class _Stop(Exception):
    pass


def _math_mpc_calls(mmt, n_calls, barrier=None):
    """Poses and controls math_mpc returns in its first n_calls calls of the
    reference scenario's model run."""
    log = []

    def on_step(p, coords):
        log.append(tuple(coords))
        if len(log) == n_calls:
            raise _Stop

    mmt.reset_state()
    if barrier is not None:
        mmt.add_barrier_circle(*barrier)
    try:
        mmt.math_mpc([0, 0, 0, 0, 0], [2, 3], False, on_step=on_step)
    except _Stop:
        pass
    return log


def test_drop_in_barrier(engine):
    from diplomjourney_amd import math_model_tree as mmt
    r = 0.15
    try:
        free = _math_mpc_calls(mmt, 40)
        assert len(free) == 40 and mmt.barriers == []
        cx, cy = free[19][0], free[19][1]             # the pose call 20 returns
        assert any(math.hypot(x - cx, y - cy) < r for x, y, *_ in free)   # it drives in
        kept = _math_mpc_calls(mmt, 40, barrier=(cx, cy, r))
        assert mmt.barriers == [(cx, cy, r)] and len(kept) >= 1
        for x, y, *_ in kept:
            assert math.hypot(x - cx, y - cy) - r > 1e-9, (x, y)
        mmt.clear_barriers()
        assert mmt.barriers == []
        again = _math_mpc_calls(mmt, 40)
        assert [(q[3], q[4]) for q in again] == [(q[3], q[4]) for q in free]
    finally:
        mmt.reset_state()


def test_host_episode(engine):
    """Episode(obstacles=...): partials with circles, the unchanged finalize
    (no chained / exchange entry involved)."""
    from diplomjourney_amd.episode import Episode
    r = 0.15

    def poses(obstacles):
        ep = Episode(engine, 4096, 5, obstacles=obstacles)
        out = []
        for _ in range(60):
            ep.step()
            out.append((ep.last_log[3], ep.last_log[4]))
        return out

    free = poses(())
    cx, cy = free[29]
    assert sum(math.hypot(x - cx, y - cy) < r for x, y in free) >= 1
    kept = poses([(cx, cy, r)])
    assert len(kept) == 60
    for x, y in kept:
        assert math.hypot(x - cx, y - cy) - r > 1e-9, (x, y)
