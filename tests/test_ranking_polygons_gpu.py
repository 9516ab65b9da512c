"""Every candidate of the keep-out polygon kernels (mpc_rollout_argmin_keepout)
ranked against the host replica, off the origin.

The scheme is test_ranking_gpu.py's test_rank_obstacles: the fixed 1026-column
input of a horizon (ranking.controls: duplicates, irregular, NaN and +inf
candidates planted) is launched, the winner removed, and again until nothing is
left; the sequence of (cost, index) must be the replica's ranking restricted to
the expected mask, `==` on the doubles, and n_blocked the mask's count in every
launch (a peeled candidate was free, and its NaN states are inside nothing).

The expected mask carries no margin.  It is the host build of the lane hook's
own functions (csrc/mpc_keepout.h: world_polygons, frame_edge, inside_polygons;
two fma and a compare per edge) on what the hook is handed: the replica's
states, which are the device's bit for bit, and in rect+cum the recurrence's
sums, which tests/replica_harness.cpp exports (replica_cum_sums; cum_pose of
them is asserted to be the replica's state bit for bit), an irregular
candidate's recomputed states meeting the world table as in the kernels.  So
one misjudged candidate anywhere in a launch changes the sequence, also where
two would cancel in the count.  Before any launch that mask is itself compared
with the exact rule (polygon_cases.exact_inside: rational side of every edge
line) on every state outside the header's bound — for rect+cum plus the
measured distance of the sums' image from the state — and the scene's
conditions are asserted (ranking.check_polygon_scene).

Every case prints what it ranked.
"""
import sys

import numpy as np
import pytest
import torch

import polygon_cases as pc
import ranking as R

pytestmark = pytest.mark.gpu

INC_MAX = float(sys.maxsize)
MOVED = tuple(n for n in pc.PLACEMENTS if n != "start")


def _dev(a):
    return torch.as_tensor(np.array(a), device="cuda")


def _off8(a):
    """a on the device, 8 bytes off a 16-byte boundary."""
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[1:].view(a.shape)
    t.copy_(_dev(a))
    assert t.data_ptr() % 16 == 8
    return t


def _rank(engine, c, unaligned=False):
    """Peel case c (ranking.polygon_case) through engine.rollout_argmin."""
    put = _off8 if unaligned else _dev
    vd, bd = put(c.inp.v), put(c.inp.b)
    nb = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def launch():
        out = engine.rollout_argmin(c.problem, vd, bd, incumbent=INC_MAX, integrator=c.mode,
                                    obstacles=c.circles or None, polygons=c.polygons,
                                    n_blocked=nb)
        return torch.cat([R.result_words(out), nb.view(1, 1)], dim=1)

    got = R.peel(launch, vd, R.soa_offset(), c.n_free + 2)[:, 0]
    n_blocked = int(c.mask.sum())
    assert got[0, R.REC_WORDS] == n_blocked, (got[0, R.REC_WORDS], n_blocked)
    assert (got[:, R.REC_WORDS] == n_blocked).all()
    assert R.check_ranking(got, c.costs, excluded=c.mask, states=c.states,
                           what=c.what) == c.n_free
    print(f"{c.what}{' unaligned' if unaligned else ''}: ranked {c.n_free} candidates "
          f"({n_blocked} blocked, {len(c.polygons)} polygons, {len(c.circles)} circles"
          f"{', an edge through candidate %d' % c.through[0] if c.through else ''})")


# ----------------------------------------------------------------------------
# C1, C2: the four polygons
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", (1, 3, 10))
@pytest.mark.parametrize("mode", R.MODES)
def test_rank_polygons(engine, mode, n_steps):
    """Every mode at the ranking module's START.  At N = 3 the square nobody
    reaches gives way to one with an edge line through the final state of the
    best regular candidate the other polygons leave free — the exact distance
    an ulp or two, far inside the header's bound: host build and device must
    agree on that candidate too, and it decides rank 0."""
    _rank(engine, R.polygon_case("start", mode, n_steps, plant=n_steps == 3, device=True))


@pytest.mark.parametrize("mode", ("rect", "rect+cum", "qk21+rot"))
@pytest.mark.parametrize("name", MOVED)
def test_rank_polygons_moved(engine, name, mode):
    """Every other placement: order 10 in two quadrants with the divided
    wheelbases, phi = pi/2, phi = 4, L = 1/4, order 1000."""
    _rank(engine, R.polygon_case(name, mode, 3, device=True))


# ----------------------------------------------------------------------------
# C3: circles and polygons in one call
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("rect", "rect+cum", "qk21"))
@pytest.mark.parametrize("name", ("start", "ten-II"))
def test_rank_keepout_mixed(engine, name, mode):
    """The union of ranking.circles' mask (the header's formula on the replica's
    states, every state further than ranking.MARGIN from every circle, as in
    test_rank_obstacles) and the polygons': some candidate blocked by a circle
    alone, some by a polygon alone, some by both."""
    _rank(engine, R.polygon_case(name, mode, 3, mixed=True, device=True))


# ----------------------------------------------------------------------------
# C4: one candidate per lane
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", (1, 3))
@pytest.mark.parametrize("mode", ("rect", "rect+cum"))
@pytest.mark.parametrize("shape", ("odd", "unaligned"))
def test_rank_polygons_scalar_fallback(engine, shape, mode, n_steps):
    """test_rank_scalar_fallback's two inputs: KeepoutObs::test<1> in loop()."""
    c = R.polygon_case("start", mode, n_steps, n=1025 if shape == "odd" else R.N_CAND,
                       device=True)
    _rank(engine, c, unaligned=shape == "unaligned")


# ----------------------------------------------------------------------------
# C5: the hook's loop over the polygon count
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_poly", (1, 2, 3))
def test_rank_polygon_counts(engine, n_poly):
    """The first 1, 2, 3 polygons of the scene, each blocking somebody."""
    _rank(engine, R.polygon_case("ten-III", "rect+cum", 3, n_poly=n_poly, device=True))


# ----------------------------------------------------------------------------
# C6: a polygon nobody reaches, from a moved pose
# ----------------------------------------------------------------------------
def test_unreached_polygon_is_the_plain_call_moved(engine):
    """test_no_polygons_is_the_old_call's identity at an order-10 placement."""
    c = R.polygon_case("ten-II", "rect+cum", 3, device=True)
    vd, bd = _dev(c.inp.v), _dev(c.inp.b)
    plain = engine.rollout_argmin(c.problem, vd, bd, integrator="rect+cum").cpu().numpy().tobytes()
    assert len(plain) == 808
    nb = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    far = c.polygons[3:]
    assert len(far) == 1 and not R.host_polygon_mask(c.problem, far, "rect", c.states).any()
    raw = engine.rollout_argmin(c.problem, vd, bd, integrator="rect+cum", polygons=far,
                                n_blocked=nb).cpu().numpy().tobytes()
    assert raw == plain and int(nb.item()) == 0
    print(f"{c.what}: a polygon nobody reaches gives the plain call's 808 bytes")
