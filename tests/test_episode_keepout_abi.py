"""Keep-out polygons in the device-resident episode steps, without a GPU: the
three entries' declarations and argument checks (fake device pointers: every
call returns before any HIP call), the order of those checks, and
DeviceEpisode's polygon arguments as far as they need no device."""
import ctypes
import re

import pytest

import obstacle_cases
import polygon_cases as pc
from diplomjourney_amd import abi, native

ENTRIES = ("mpc_episode_partials_keepout", "mpc_episode_step_keepout",
           "mpc_episode_chain_step_keepout")
_P = ctypes.c_void_p


def test_exports_declared_and_present():
    text = re.sub(r"/\*.*?\*/", "", open(native.HEADER).read(), flags=re.S)
    so = ctypes.CDLL(native.LIB_PATH)
    for name in ENTRIES:
        assert name in native.EXPORTS and name in native.PROTOTYPES
        assert re.search(r"\b%s\s*\(" % name, text), name
        getattr(so, name)
        # the _obstacles twin's arguments with (polygons, count) directly after n_obstacles
        twin = native.PROTOTYPES[name.replace("_keepout", "_obstacles")][1]
        at = 3 if name != "mpc_episode_chain_step_keepout" else 4
        assert twin[at - 2:at] == [_P, ctypes.c_int32]
        assert native.PROTOTYPES[name][1] == twin[:at] + [_P, ctypes.c_int32] + twin[at:]
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert re.search(r"n_obstacles,\s*const mpc_polygon_t\*\s*polygons,\s*int32_t n_polygons,",
                         decl), name


def _calls():
    """{entry: call(circles, polygons, **overrides)} over fake pointers; every
    default is an acceptable argument, so a call without a fault would launch.
    circles / polygons: (array, count)."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    cfg = reference_episode_config()
    f, g = _P(0x1000), _P(0x2000)
    base = dict(cfg=cfg, state=f, v=f, b=g, n=1024, ns=10, base=0,
                integ=abi.INTEGRATORS["rect+cum"], ws=f, wsb=1 << 24, out=f, log=f, cap=8,
                epoch=3, mode=1, ws_prev=f, v_prev=None, b_prev=None, advance=None, nb=None)

    def ref(c):
        return ctypes.byref(c) if c is not None else None

    def partials(a, obs, poly):
        return L.mpc_episode_partials_keepout(
            a["state"], *obs, *poly, a["v"], a["b"], a["n"], a["ns"], a["integ"], a["ws"],
            a["wsb"], a["nb"], None)

    def step(a, obs, poly):
        return L.mpc_episode_step_keepout(
            a["state"], *obs, *poly, a["v"], a["b"], a["n"], a["ns"], a["base"], a["integ"],
            a["ws"], a["wsb"], a["out"], ref(a["advance"]), a["log"], a["cap"], a["nb"], None)

    def chain(a, obs, poly):
        return L.mpc_episode_chain_step_keepout(
            ref(a["cfg"]), a["state"], *obs, *poly, a["mode"], a["epoch"], a["v"], a["b"], a["n"],
            a["ns"], a["base"], a["integ"], a["ws"], a["ws_prev"], a["wsb"], a["v_prev"],
            a["b_prev"], a["out"], None, 0, a["log"], a["cap"], a["nb"], None)

    def entry(fn):
        return lambda obs, poly, **kw: fn({**base, **kw}, obs, poly)

    return {"partials": entry(partials), "step": entry(step), "chain_step": entry(chain)}


OK_CIRCLES = abi.make_obstacles([(1.0, 2.0, 0.5), (-3.0, 0.5, 0.25)])
NONE = (None, 0)


def _ok_polygons():
    return pc.polygons_array(pc.OK_POLYGON, pc.OK_POLYGON[::-1]), 2


def test_polygon_rejections_without_gpu():
    """Every rejected polygon argument is MPC_ERR_ARG with otherwise acceptable
    arguments, with and without circles, also when the base arguments are
    wrong as well (the polygons are checked before them)."""
    bad = pc.rejected_polygons()
    assert len(bad) == 3 + 2 * 11
    for name, call in _calls().items():
        for what, poly in bad.items():
            assert call(OK_CIRCLES, poly) == abi.MPC_ERR_ARG, (name, what)
            assert call(NONE, poly) == abi.MPC_ERR_ARG, (name, what)
            assert call(NONE, poly, integ=7, wsb=8) == abi.MPC_ERR_ARG, (name, what)
        for what, obs in obstacle_cases.rejected_circles().items():
            assert call(obs, _ok_polygons()) == abi.MPC_ERR_ARG, (name, what)


def test_check_order_without_gpu():
    """Circles, then polygons, then the base entry's checks in their stage
    order.  The statuses alone cannot tell two MPC_ERR_ARG apart, so the order
    shows where a later stage would answer otherwise: a bad polygon (ARG)
    before an unsupported mode and before a short workspace; a bad circle
    likewise; and with valid tables every rejection is the base entry's."""
    dart = (pc.polygons_array([(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)]), 1)
    bad_circle = abi.make_obstacles([(1.0, 1.0, -0.5)])
    ok = _ok_polygons()
    for name, call in _calls().items():
        # a bad circle and a bad polygon together: the circle's status (both ARG), before
        # anything of the base entry
        assert call(bad_circle, dart, integ=7) == abi.MPC_ERR_ARG, name
        assert call(bad_circle, ok, integ=7) == abi.MPC_ERR_ARG, name
        assert call(bad_circle, ok, wsb=8) == abi.MPC_ERR_ARG, name
        # a bad polygon and a NULL state: the polygon's; and before the later stages
        assert call(OK_CIRCLES, dart, state=None) == abi.MPC_ERR_ARG, name
        assert call(OK_CIRCLES, dart, integ=7) == abi.MPC_ERR_ARG, name
        assert call(OK_CIRCLES, dart, wsb=8) == abi.MPC_ERR_ARG, name
        # valid tables: the base entry's stages in their order
        assert call(OK_CIRCLES, ok, state=None, integ=7, wsb=8) == abi.MPC_ERR_ARG, name
        assert call(OK_CIRCLES, ok, integ=7, wsb=8) == abi.MPC_ERR_UNSUPPORTED, name
        assert call(OK_CIRCLES, ok, wsb=8) == abi.MPC_ERR_WORKSPACE, name


def test_base_rejections_match_the_obstacle_entries_without_gpu():
    """With valid polygons (and with none, where the _obstacles entry is called)
    every rejection is the status the _obstacles entry gives the same wrong call."""
    import test_episode_obstacles_abi as circles_abi
    f, odd = _P(0x1000), _P(0x2008)
    cum = abi.INTEGRATORS["rect+cum"]
    from diplomjourney_amd.episode import reference_episode_config
    bad_cfg = reference_episode_config()
    bad_cfg.stop_rule = 2
    common = [dict(state=None), dict(v=None), dict(b=None), dict(n=0), dict(ns=0), dict(ns=33),
              dict(integ=7), dict(integ=cum | 0x800), dict(ws=None), dict(wsb=8),
              dict(ns=0, integ=7), dict(integ=7, wsb=8)]
    rows = {
        "partials": common + [dict(integ=cum | abi.MPC_LAYOUT_TILED)],
        "step": common,
        "chain_step": common + [
            dict(epoch=0), dict(mode=2), dict(mode=0), dict(integ=1), dict(b=odd), dict(cap=-1),
            dict(base=-1), dict(cfg=bad_cfg), dict(cfg=None), dict(n=1023),
            dict(v_prev=f, b_prev=None), dict(v_prev=f, b_prev=None, wsb=8),
            dict(v_prev=f, b_prev=odd), dict(b=odd, wsb=8)],
    }
    twins = circles_abi._calls()
    statuses = set()
    for name, call in _calls().items():
        for kw in rows[name]:
            want = twins[name](OK_CIRCLES, **kw)
            assert want != abi.MPC_OK, (name, kw)
            shown = {k: getattr(v, "value", v) for k, v in kw.items() if k != "cfg"}
            assert call(OK_CIRCLES, _ok_polygons(), **kw) == want, (name, shown)
            assert call(NONE, _ok_polygons(), **kw) == want, (name, shown)
            assert call(OK_CIRCLES, NONE, **kw) == want, (name, shown)
            assert call(NONE, NONE, **kw) == want, (name, shown)
            statuses.add(want)
    assert statuses == {abi.MPC_ERR_ARG, abi.MPC_ERR_UNSUPPORTED, abi.MPC_ERR_WORKSPACE}


def test_device_episode_polygon_arguments_without_gpu():
    """What DeviceEpisode(polygons=...) / set_polygons() decide before they
    touch a device: the count limit, the vertex limits and the library's
    convexity rule (the refused step forms construct an episode: the GPU
    module has them)."""
    from diplomjourney_amd.device_episode import DeviceEpisode
    check = DeviceEpisode.checked_polygons
    assert check(()) == (None, 0) and check(None) == (None, 0)
    arr, n = check([pc.OK_POLYGON, pc.OK_POLYGON[::-1] + [pc.OK_POLYGON[-1]],
                    pc.ngon((3.0, -2.0), 0.25, 8, 0.3), pc.ngon((1e3, 1e3), 0.01, 3, 1.0, cw=True)])
    assert n == abi.MPC_MAX_POLYGONS and [g.n_vertices for g in arr] == [4, 4, 8, 3]
    assert pc.host().poly_check(arr, n) == abi.MPC_OK
    with pytest.raises(ValueError, match="at most 4"):
        check([pc.OK_POLYGON] * (abi.MPC_MAX_POLYGONS + 1))
    for bad in ([(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)],          # a dart
                [(0.0, 0.0), (2.0, 2.0), (2.0, 0.0), (0.0, 1.0)],          # a bow-tie
                [(0.0, 0.0), (1.0, 1.0), (2.0, 2.0)]):                     # no area
        with pytest.raises(ValueError, match="convex pieces"):
            check([pc.OK_POLYGON, bad])
    for bad in ([(0.0, 0.0), (1.0, 0.0)], pc.ngon((0.0, 0.0), 1.0, 9, 0.0), [(0, 0), (1,), (1, 1)]):
        with pytest.raises(ValueError):
            check([bad])
    # what the Python rule refuses, the library refuses, and the other way round
    for what, (raw, n) in pc.rejected_polygons().items():
        if raw is None or not 0 < n <= abi.MPC_MAX_POLYGONS:
            continue
        g = raw[n - 1]
        if 3 <= g.n_vertices <= abi.MPC_MAX_POLYGON_VERTICES:
            with pytest.raises(ValueError):
                check([[(g.x[i], g.y[i]) for i in range(g.n_vertices)]])
    assert "polygons" in DeviceEpisode._OBSTACLE_FORMS and "circles" in DeviceEpisode._OBSTACLE_FORMS
