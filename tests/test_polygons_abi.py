"""Keep-out polygons, CPU side: the two exports, the mpc_polygon_t layout, the
argument checks (all before any HIP call), make_polygons and the barrier lists
of math_model_tree.  No GPU."""
import ctypes
import os
import re
import subprocess

import pytest

import obstacle_cases
import polygon_cases as pc
from diplomjourney_amd import abi, native

HEADER = native.HEADER
NEW = ("mpc_rollout_partials_keepout", "mpc_rollout_argmin_keepout")


@pytest.fixture(scope="module")
def L():
    if native.needs_build():
        native.build()
    return native.lib()


def test_exports_declared_and_present(L):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name)


def test_polygon_layout_matches_c(tmp_path):
    src = tmp_path / "layout_poly.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "mpc_rollout.h"\n'
        "int main(void){printf(\"%zu %zu %zu %zu %zu %d %d\\n\", sizeof(mpc_polygon_t),"
        " offsetof(mpc_polygon_t, n_vertices), offsetof(mpc_polygon_t, reserved_),"
        " offsetof(mpc_polygon_t, x), offsetof(mpc_polygon_t, y),"
        " MPC_MAX_POLYGONS, MPC_MAX_POLYGON_VERTICES); return 0;}\n")
    exe = tmp_path / "layout_poly"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    G = abi.MpcPolygon
    assert got == [136, 0, 4, 8, 72, 4, 8]
    assert got == [ctypes.sizeof(G), G.n_vertices.offset, G.reserved_.offset, G.x.offset,
                   G.y.offset, abi.MPC_MAX_POLYGONS, abi.MPC_MAX_POLYGON_VERTICES]


def test_argument_validation_without_gpu(L):
    """Every rejection happens before any HIP call (fake device pointers)."""
    p = abi.make_problem(0, 0, 0.3, 2, 3, 0, 0, 0.5, 0.05, 0.1)
    fake = ctypes.c_void_p(0x1000)
    circle = (abi.MpcObstacle * 1)(abi.MpcObstacle(1.0, 1.0, 0.5))
    ok = pc.polygons_array(pc.OK_POLYGON, pc.OK_POLYGON[::-1])
    base = dict(p=ctypes.byref(p), obs=circle, n_obs=1, poly=ok, n_poly=2, v=fake, b=fake, n=100,
                ns=3, base=0, inc=1e300, integ=0, st=None, ws=fake, wsb=1 << 20, nb=None, out=fake)

    def argmin(**kw):
        a = {**base, **kw}
        return L.mpc_rollout_argmin_keepout(a["p"], a["obs"], a["n_obs"], a["poly"], a["n_poly"],
                                            a["v"], a["b"], a["n"], a["ns"], a["base"], a["inc"],
                                            a["integ"], a["st"], a["ws"], a["wsb"], a["nb"],
                                            a["out"], None)

    def partials(**kw):
        a = {**base, **kw}
        return L.mpc_rollout_partials_keepout(a["p"], a["obs"], a["n_obs"], a["poly"], a["n_poly"],
                                              a["v"], a["b"], a["n"], a["ns"], a["integ"], a["st"],
                                              a["ws"], a["wsb"], a["nb"], None)

    rejected = pc.rejected_polygons()
    assert len(rejected) == 3 + 2 * 11
    circles = obstacle_cases.rejected_circles()
    for call in (argmin, partials):
        for what, (poly, n_poly) in rejected.items():
            assert call(poly=poly, n_poly=n_poly) == abi.MPC_ERR_ARG, what
            assert call(poly=poly, n_poly=n_poly, obs=None, n_obs=0) == abi.MPC_ERR_ARG, what
        # a rejected circle with valid polygons
        for what, (obs, n_obs) in circles.items():
            assert call(obs=obs, n_obs=n_obs) == abi.MPC_ERR_ARG, what
        # the base entries' own rejections hold behind valid tables
        assert call(p=None) == abi.MPC_ERR_ARG
        assert call(n=0) == abi.MPC_ERR_ARG
        assert call(ns=abi.MPC_MAX_STEPS + 1) == abi.MPC_ERR_ARG
        assert call(v=None) == abi.MPC_ERR_ARG
        assert call(integ=7) == abi.MPC_ERR_UNSUPPORTED
        assert call(integ=abi.MPC_INTEG_RECT | abi.MPC_LAYOUT_TILED) == abi.MPC_ERR_UNSUPPORTED
        assert call(wsb=8) == abi.MPC_ERR_WORKSPACE
        # ... and without polygons, where the circle entry is called
        assert call(poly=None, n_poly=0, n=0) == abi.MPC_ERR_ARG
        assert call(poly=None, n_poly=0, wsb=8) == abi.MPC_ERR_WORKSPACE
    assert argmin(out=None) == abi.MPC_ERR_ARG
    assert argmin(base=-1) == abi.MPC_ERR_ARG


def test_python_rule_is_the_library_rule(L):
    """abi.polygon_is_convex (add_barrier_polygon's check) and the entries' check
    agree on every shape of rejected_polygons() that make_polygons can express."""
    shapes = [pc.OK_POLYGON, pc.OK_POLYGON[::-1], pc.ngon((3.0, -2.0), 0.25, 8, 0.3),
              pc.ngon((1e6, 1e6), 0.01, 3, 1.0, cw=True)]
    for pts in shapes:
        assert abi.polygon_is_convex(tuple(pts))
    for what, (arr, n) in pc.rejected_polygons().items():
        if arr is None or not 0 < n <= abi.MPC_MAX_POLYGONS:
            continue
        g = arr[n - 1]
        if 3 <= g.n_vertices <= abi.MPC_MAX_POLYGON_VERTICES:
            pts = tuple((g.x[i], g.y[i]) for i in range(g.n_vertices))
            assert not abi.polygon_is_convex(pts), what


def test_make_polygons():
    assert abi.make_polygons(None) == (None, 0) and abi.make_polygons([]) == (None, 0)
    tri = [(0, 0), (1, 0), (0.5, 2)]
    arr, n = abi.make_polygons([tri, pc.OK_POLYGON])
    assert n == 2 and arr[0].n_vertices == 3 and arr[1].n_vertices == 4
    assert [(arr[0].x[i], arr[0].y[i]) for i in range(3)] == [(0.0, 0.0), (1.0, 0.0), (0.5, 2.0)]
    # the reference's closed form: the repeated first vertex is dropped
    closed, n1 = abi.make_polygons([tri + [tri[0]]])
    assert n1 == 1 and closed[0].n_vertices == 3
    assert bytes(closed[0]) == bytes(arr[0])
    octagon = pc.ngon((0.0, 0.0), 1.0, 8, 0.0)
    assert abi.make_polygons([octagon + [octagon[0]]])[0][0].n_vertices == 8
    for bad in ([[(0, 0), (1, 0)]], [[(0, 0), (1, 0), (0, 0)]], [[(0, 0, 1), (1, 0, 1), (1, 1, 1)]],
                [pc.ngon((0.0, 0.0), 1.0, 9, 0.0)], [[(0, 0), (1,), (1, 1)]]):
        with pytest.raises(ValueError):
            abi.make_polygons(bad)


def test_barrier_lists():
    from diplomjourney_amd import math_model_tree as mmt
    assert mmt.barriers == [] and mmt.barrier_polygons == []
    try:
        mmt.add_barrier_polygon([(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)])      # closed form
        mmt.add_barrier_polygon([(2, 2), (2, 3), (3, 2)])                      # clockwise
        mmt.add_barrier_circle(1, 2, 0.5)
        assert mmt.barrier_polygons == [((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)),
                                        ((2.0, 2.0), (2.0, 3.0), (3.0, 2.0))]
        assert mmt.barriers == [(1.0, 2.0, 0.5)]          # circles only, as other modules read it
        mmt.clear_barriers()
        assert mmt.barriers == [] and mmt.barrier_polygons == []
        mmt.add_barrier_polygon(pc.OK_POLYGON)
        mmt.reset_state()
        assert mmt.barrier_polygons == []
    finally:
        mmt.reset_state()


def test_add_barrier_polygon_refuses_a_dart():
    from diplomjourney_amd import math_model_tree as mmt
    try:
        with pytest.raises(ValueError, match="convex pieces"):
            mmt.add_barrier_polygon([(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)])
        with pytest.raises(ValueError, match="convex pieces"):
            mmt.add_barrier_polygon([(0.0, 0.0), (1.0, 1.0), (2.0, 2.0)])
        with pytest.raises(ValueError):
            mmt.add_barrier_polygon([(0.0, 0.0), (1.0, 1.0)])
        assert mmt.barrier_polygons == []
    finally:
        mmt.reset_state()


def test_circle_only_drivers_refuse_registered_polygons():
    """The entries that read math_model_tree.barriers by default take circles
    only: with a polygon registered and no obstacles argument they raise before
    they need a device; an explicit obstacles argument is the caller's word."""
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd import run_math_model as rmm
    start = (0.0, 0.0, 0.0, 2.0, 3.0)
    try:
        mmt.add_barrier_polygon(pc.OK_POLYGON)
        for call in (lambda: rmm.run_tree_batched([start], max_calls=1),
                     lambda: rmm.run_tree_fleet([start], 0.1, max_calls=1),
                     lambda: rmm.run_batched([start], max_calls=1),
                     lambda: rmm.run_batched_lockstep([start], max_calls=1),
                     lambda: rmm.device_ft_episodes([start], max_calls=1),
                     lambda: rmm.predictive_control(0.0, 0.0, 0.0, 0.0, 2.0, 3.0)):
            with pytest.raises(ValueError, match="barrier_polygons"):
                call()
        mmt.clear_barriers()
        mmt.require_no_barrier_polygons("anybody")          # nothing registered: no error
    finally:
        mmt.reset_state()
