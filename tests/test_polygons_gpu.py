"""Keep-out polygons on the GPU (mpc_rollout_partials_keepout /
mpc_rollout_argmin_keepout and the Python layers over them) against the CPU
oracle: tests/polygon_cases.py forms the blocked mask and the expected winner
from the oracle's states and costs."""
import math

import pytest

import obstacle_cases as oc
import polygon_cases as pc
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


def _run(engine, c, mode, polygons, circles=None, states=None):
    """(MpcResult, raw 808 bytes, n_blocked) of one keep-out call."""
    import torch
    v, b = _dev(c)
    nb = torch.full((1,), -7, dtype=torch.int64, device=engine.device)
    out = engine.rollout_argmin(c.problem, v, b, integrator=mode, states=states,
                                obstacles=circles, polygons=polygons, n_blocked=nb)
    res = engine.fetch(out)
    return res, out.cpu().numpy().tobytes(), int(nb.item())


def _check_winner(res, n_blocked, c):
    print(f"n_blocked {n_blocked} (oracle {c.n_blocked}) index {res.index} ({c.index}) "
          f"cost {res.cost!r} ({c.cost!r})")
    assert n_blocked == c.n_blocked                     # exactly the oracle's count
    assert res.index == c.index and res.found == 1
    assert math.isclose(res.cost, c.cost, rel_tol=1e-12), (res.cost, c.cost)


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_steps", [1, 3, 10])
@pytest.mark.parametrize("n_cand", [2178, 2177, 130])
def test_mask_and_winner(engine, oracle, n_cand, n_steps, mode):
    """The four polygons.  2178: four blocks and a partial wave on the LDS-DMA
    ring path; 2177: the one-candidate-per-lane path; N = 10 wraps the ring,
    N = 1 never refills it."""
    c = pc.case(n_cand, n_steps, oc.ORACLE_OF[mode])
    pc.check_preconditions(c)
    res, _, nb = _run(engine, c, mode, c.polygons)
    _check_winner(res, nb, c)


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("n_cand", [2178, 130])
def test_mixed_with_a_circle(engine, oracle, n_cand, n_steps, mode):
    """Polygons and a circle in one call: the count is the union's, not the sum."""
    c = pc.case(n_cand, n_steps, oc.ORACLE_OF[mode], mixed=True)
    pc.check_preconditions(c)
    by_poly = int(pc.polygon_mask(c.states, c.polygons).sum())
    by_circle = int(oc.blocked_mask(c.states, c.circles).sum())
    assert max(by_poly, by_circle) < c.n_blocked <= by_poly + by_circle
    if n_steps > 1:     # some candidates enter both (one state cannot: the shapes are disjoint)
        assert c.n_blocked < by_poly + by_circle
    res, _, nb = _run(engine, c, mode, c.polygons, circles=c.circles)
    _check_winner(res, nb, c)


@pytest.mark.parametrize("mode", oc.MODES)
def test_one_polygon_alone(engine, oracle, mode):
    """(b), the clockwise triangle: the smallest table."""
    c = pc.case(2178, 3, oc.ORACLE_OF[mode])
    mask = pc.polygon_mask(c.states, c.polygons[1:2])
    assert 0 < mask.sum() < c.n_cand
    want_i, want_c = oc.expected_winner(c.costs, mask)
    res, _, nb = _run(engine, c, mode, c.polygons[1:2])
    assert nb == int(mask.sum())
    assert res.index == want_i and res.found == 1
    assert math.isclose(res.cost, want_c, rel_tol=1e-12)


@pytest.mark.parametrize("shape", [(2178, 3), (2177, 10)])
def test_wheelbase_not_a_power_of_two(engine, oracle, shape):
    """L = 0.3, rect+cum: the frame of the unscaled sums."""
    c = pc.case(shape[0], shape[1], "rect", L=0.3)
    pc.check_preconditions(c)
    res, _, nb = _run(engine, c, "rect+cum", c.polygons)
    _check_winner(res, nb, c)


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_cand", [2178, 2177])
def test_no_polygons_is_the_old_call(engine, oracle, n_cand, mode):
    """polygons=[] with and without circles, and a square nothing reaches: the
    808 result bytes and the count of the corresponding existing call."""
    import torch
    c = pc.case(n_cand, 3, oc.ORACLE_OF[mode], mixed=True)
    v, b = _dev(c)
    plain = engine.rollout_argmin(c.problem, v, b, integrator=mode).cpu().numpy().tobytes()
    assert len(plain) == 808
    nb = torch.full((1,), -7, dtype=torch.int64, device=engine.device)
    circ = engine.rollout_argmin(c.problem, v, b, integrator=mode, obstacles=c.circles,
                                 n_blocked=nb).cpu().numpy().tobytes()
    n_circ = int(nb.item())
    assert n_circ == int(oc.blocked_mask(c.states, c.circles).sum()) > 0
    _, raw, n0 = _run(engine, c, mode, [])
    assert raw == plain and n0 == 0
    _, raw, n1 = _run(engine, c, mode, [], circles=c.circles)
    assert raw == circ and n1 == n_circ
    _, raw, n2 = _run(engine, c, mode, c.polygons[2:3])            # (c), never reached
    assert raw == plain and n2 == 0
    _, raw, n3 = _run(engine, c, mode, c.polygons[2:3], circles=c.circles)
    assert raw == circ and n3 == n_circ


def test_zero_polygons_through_the_entry(engine, oracle):
    """n_polygons == 0 at the C entry itself (Expansion never calls it so):
    the circle entry's bytes and count, and with no circles the plain call's."""
    import ctypes
    import torch
    from diplomjourney_amd import native
    c = pc.case(2178, 3, "rect", mixed=True)
    v, b = _dev(c)
    ws = torch.empty(engine.lib.mpc_workspace_bytes(c.n_cand, c.n_steps), dtype=torch.uint8,
                     device=engine.device)
    integ = abi.INTEGRATORS["rect+cum"]
    want = {}
    nb = torch.full((1,), -7, dtype=torch.int64, device=engine.device)
    # (a record's states past n_steps are not written: both calls start from zeros)
    out = torch.zeros(abi.RESULT_BYTES, dtype=torch.uint8, device=engine.device)
    for circles in ((), tuple(c.circles)):
        out.zero_()
        raw = engine.rollout_argmin(c.problem, v, b, integrator="rect+cum", obstacles=circles,
                                    n_blocked=nb, out=out).cpu().numpy().tobytes()
        want[circles] = (raw, int(nb.item()))
    assert want[()][1] == 0 < want[tuple(c.circles)][1]
    for circles in ((), tuple(c.circles)):
        obs, n_obs = abi.make_obstacles(circles)
        out.zero_()
        nb.fill_(-7)
        native.check(engine.lib.mpc_rollout_argmin_keepout(
            ctypes.byref(c.problem), obs, n_obs, None, 0, v.data_ptr(), b.data_ptr(), c.n_cand,
            c.n_steps, 0, math.inf, integ, None, ws.data_ptr(), ws.numel(), nb.data_ptr(),
            out.data_ptr(), native.current_stream()), "mpc_rollout_argmin_keepout")
        assert (out.cpu().numpy().tobytes(), int(nb.item())) == want[circles]


@pytest.mark.parametrize("mode", oc.MODES)
@pytest.mark.parametrize("n_cand", [2178, 2177])
def test_all_blocked(engine, oracle, n_cand, mode):
    c = pc.case(n_cand, 3, oc.ORACLE_OF[mode])
    res, _, nb = _run(engine, c, mode, [pc.ngon(oc.POSE[:2], 10.0, 8, 0.0)])
    assert res.index == -1 and res.found == 0 and nb == n_cand
    assert res.cost == math.inf


@pytest.mark.parametrize("mode", ["rect+rot", "rect+cum"])
def test_irregular_candidate(engine, oracle, mode):
    """A candidate with beta = 1.2 at step 0 is recomputed by step_safe; the
    square on its state after step 2 must block it there as well (the world
    table)."""
    c = pc.case(130, 3, oc.ORACLE_OF[mode], irregular=True)
    pc.check_preconditions(c)
    res, _, nb = _run(engine, c, mode, c.polygons)
    _check_winner(res, nb, c)
    # without the replaced square the irregular candidate is free (and whoever else it blocked)
    rest = c.polygons[:2] + c.polygons[3:]
    free = pc.polygon_mask(c.states, rest)
    assert not free[c.irr] and free.sum() < c.n_blocked
    _, _, nb3 = _run(engine, c, mode, rest)
    assert nb3 == int(free.sum())


def test_states_variant(engine, oracle):
    import torch
    c = pc.case(2177, 3, "qk21")
    pc.check_preconditions(c)
    v, b = _dev(c)
    s_plain = torch.zeros((3, 3, c.n_cand), dtype=torch.float64, device=engine.device)
    s_poly = torch.full_like(s_plain, -1.0)
    engine.rollout_argmin(c.problem, v, b, integrator="qk21", states=s_plain)
    res, _, nb = _run(engine, c, "qk21", c.polygons, states=s_poly)
    assert torch.equal(s_plain.view(torch.int64), s_poly.view(torch.int64))
    _check_winner(res, nb, c)


@pytest.mark.parametrize("mode", oc.MODES)
def test_shards(engine, oracle, mode):
    """Two partials + finalize calls over the halves, then mpc_select_winner:
    the single call's result."""
    import torch
    c = pc.case(2178, 3, oc.ORACLE_OF[mode])
    pc.check_preconditions(c)
    single, _, nb = _run(engine, c, mode, c.polygons)
    v, b = _dev(c)
    half = c.n_cand // 2
    gathered = torch.zeros(2 * abi.RESULT_BYTES, dtype=torch.uint8, device=engine.device)
    counts = torch.zeros(2, dtype=torch.int64, device=engine.device)
    for r, (lo, hi) in enumerate([(0, half), (half, c.n_cand)]):
        vs, bs = v[:, lo:hi].contiguous(), b[:, lo:hi].contiguous()
        engine.partials(c.problem, vs, bs, mode, polygons=c.polygons, n_blocked=counts[r:r + 1])
        engine.finalize(c.problem, vs, bs, index_base=lo, integrator=mode,
                        out=gathered[r * abi.RESULT_BYTES:(r + 1) * abi.RESULT_BYTES])
    got = engine.fetch(engine.select_winner(gathered))
    assert int(counts.sum().item()) == nb == c.n_blocked
    assert (got.index, got.found, got.cost, got.v, got.beta, got.n_steps) == \
        (single.index, single.found, single.cost, single.v, single.beta, single.n_steps)
    assert got.trajectory() == single.trajectory()


class _Stop(Exception):
    pass


def _math_mpc_calls(mmt, n_calls, polygon=None):
    """Poses and controls math_mpc returns in its first n_calls calls of the
    reference scenario's model run."""
    log = []

    def on_step(p, coords):
        log.append(tuple(coords))
        if len(log) == n_calls:
            raise _Stop

    mmt.reset_state()
    if polygon is not None:
        mmt.add_barrier_polygon(polygon)
    try:
        mmt.math_mpc([0, 0, 0, 0, 0], [2, 3], False, on_step=on_step)
    except _Stop:
        pass
    return log


def _min_margin(poses, square):
    """The smallest over the poses of: how far outside the square the pose is
    (the largest outward distance over the edges; negative: inside)."""
    import numpy as np
    x, y = np.array([q[0] for q in poses]), np.array([q[1] for q in poses])
    return float((-pc.edge_distances(x, y, square)).max(axis=0).min())


def test_drop_in_barrier_polygon(engine):
    from diplomjourney_amd import math_model_tree as mmt
    try:
        free = _math_mpc_calls(mmt, 40)
        assert len(free) == 40 and mmt.barrier_polygons == []
        square = pc.ngon((free[19][0], free[19][1]), 0.15, 4, 0.0)   # about the pose call 20 returns
        assert _min_margin(free, square) < 0                          # the free run enters it
        kept = _math_mpc_calls(mmt, 40, polygon=square)
        assert mmt.barrier_polygons == [tuple(square)] and mmt.barriers == [] and len(kept) >= 1
        assert _min_margin(kept, square) > 1e-9
        mmt.clear_barriers()
        assert mmt.barrier_polygons == []
        again = _math_mpc_calls(mmt, 40)
        assert [(q[3], q[4]) for q in again] == [(q[3], q[4]) for q in free]
    finally:
        mmt.reset_state()


def test_host_episode(engine):
    """Episode(polygons=...): partials with polygons, the unchanged finalize."""
    from diplomjourney_amd.episode import Episode

    def poses(polygons):
        ep = Episode(engine, 4096, 5, polygons=polygons)
        out = []
        for _ in range(60):
            ep.step()
            out.append((ep.last_log[3], ep.last_log[4]))
        return out

    free = poses(())
    square = pc.ngon(free[29], 0.15, 4, 0.0)
    assert _min_margin(free, square) < 0
    kept = poses([square])
    assert len(kept) == 60
    assert _min_margin(kept, square) > 1e-9
