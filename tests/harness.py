"""Builds and loads the host test harnesses (trig_harness.cpp with g++; every
other tests/*_harness.cpp as the host side of a HIP translation unit)."""
import contextlib
import ctypes
import glob
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BUILD = os.path.join(REPO, "oracle", "_build")
_P = ctypes.c_void_p


def library_headers():
    """Every header a harness may include: the library's csrc/*.h and the ABI header."""
    return sorted(glob.glob(os.path.join(REPO, "diplomjourney_amd", "csrc", "*.h"))) + [
        os.path.join(REPO, "include", "mpc_rollout.h")]


def _build(name, cmd):
    out = os.path.join(BUILD, f"lib{name}.so")
    src = os.path.join(HERE, f"{name}.cpp")
    deps = [src, *library_headers()]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(cmd + ["-o", out, src], check=True)
    return ctypes.CDLL(out)


def host_lib(name):
    """tests/<name>.cpp as the library's host build: hipcc's host side alone,
    with the library's -ffp-contract=off."""
    return _build(name, ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                         "-shared", "--cuda-host-only", "-x", "hip", "-I",
                         os.path.join(REPO, "include")])


def trig_lib():
    L = _build("trig_harness", ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                                "-shared"])
    L.trig_eval.argtypes = [_P, ctypes.c_int64, _P, _P, _P]
    L.trig_tan_small.argtypes = [_P, ctypes.c_int64, _P]
    return L


def trig_eval(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    t, s, c = np.empty(n), np.empty(n), np.empty(n)
    trig_lib().trig_eval(x.ctypes.data_as(_P), n, t.ctypes.data_as(_P), s.ctypes.data_as(_P),
                         c.ctypes.data_as(_P))
    return t, s, c


def tan_small(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    t = np.empty(len(x))
    trig_lib().trig_tan_small(x.ctypes.data_as(_P), len(x), t.ctypes.data_as(_P))
    return t


def replica_lib():
    from diplomjourney_amd.abi import MpcFulltreeProblem, MpcProblem
    L = host_lib("replica_harness")
    L.replica_rollout.argtypes = [ctypes.POINTER(MpcProblem), _P, _P, ctypes.c_int64,
                                  ctypes.c_int32, ctypes.c_int32, _P, _P]
    L.replica_rollout_device_consts.argtypes = L.replica_rollout.argtypes
    L.replica_set_rcp_table.argtypes = [_P, _P, ctypes.c_int64]
    L.replica_rcp_misses.restype = ctypes.c_int64
    L.replica_tan_q.argtypes = [_P, ctypes.c_int64, _P]
    L.replica_fulltree.argtypes = [ctypes.POINTER(MpcFulltreeProblem), _P, ctypes.c_int32, _P,
                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P,
                                   ctypes.POINTER(ctypes.c_int32), _P, ctypes.c_int64, _P]
    L.replica_episode_layout.argtypes = [_P, ctypes.c_int32]
    L.replica_episode_layout.restype = None
    L.replica_consts.argtypes = [ctypes.POINTER(MpcProblem), _P]
    L.replica_consts.restype = None
    L.replica_cost.argtypes = [_P, ctypes.c_double, ctypes.c_double]
    L.replica_cost.restype = ctypes.c_double
    return L


def episode_layout(n):
    """replica_episode_layout's first n values and the count it reports after them."""
    out = np.full(n + 1, -1, dtype=np.int64)
    replica_lib().replica_episode_layout(out.ctypes.data_as(_P), n + 1)
    return [int(q) for q in out[:n]], int(out[n])


def robot_layout():
    """replica_robot_layout's eight values."""
    out = np.full(8, -1, dtype=np.int64)
    L = replica_lib()
    L.replica_robot_layout.argtypes = [_P]
    L.replica_robot_layout.restype = None
    L.replica_robot_layout(out.ctypes.data_as(_P))
    return [int(q) for q in out]


def replica_consts(problem, nbytes):
    """consts_from_problem(problem) as the library's host build forms it: raw bytes."""
    buf = ctypes.create_string_buffer(nbytes)
    replica_lib().replica_consts(ctypes.byref(problem), buf)
    return buf.raw


def replica_cost(consts_bytes, x, y):
    """cost(x, y, K) of the library's host build, K = replica_consts' bytes."""
    return float(replica_lib().replica_cost(ctypes.c_char_p(bytes(consts_bytes)), float(x),
                                            float(y)))


def device_rcp(q):
    """The GPU's reciprocal estimates of q (mpc_rcp_estimate)."""
    import torch
    from diplomjourney_amd import native
    qd = torch.as_tensor(np.ascontiguousarray(q, dtype=np.float64), device="cuda")
    rd = torch.empty_like(qd)
    native.check(native.lib().mpc_rcp_estimate(qd.data_ptr(), rd.data_ptr(), qd.numel(), None),
                 "mpc_rcp_estimate")
    torch.cuda.synchronize()
    return rd.cpu().numpy()


def replica_rollout(problem, v_sc, b_sc, integ="rect", device_estimates=False,
                    device_consts=False):
    """Host replica of the kernel arithmetic -> (states [N,3,C], costs [C]).
    device_estimates: the steering tangent's reciprocal estimates come from
    the GPU (every denominator of b_sc), so the result is the device's bit for
    bit; otherwise the host's 1.0 / q (within tolerances of it).
    device_consts: the problem constants as the device derives them (the
    episode entries and the batched entry: consts_from_problem) instead of the
    one-shot entries' host derivation."""
    from diplomjourney_amd.abi import INTEGRATORS
    v_sc = np.ascontiguousarray(v_sc, dtype=np.float64)
    b_sc = np.ascontiguousarray(b_sc, dtype=np.float64)
    ns, n = v_sc.shape
    states, costs = np.empty((ns, 3, n)), np.empty(n)
    L = replica_lib()
    if device_estimates:
        beta = np.unique(b_sc)
        q = np.empty_like(beta)
        L.replica_tan_q(beta.ctypes.data_as(_P), len(beta), q.ctypes.data_as(_P))
        q = np.unique(q)
        r = device_rcp(q)
        L.replica_set_rcp_table(q.ctypes.data_as(_P), r.ctypes.data_as(_P), len(q))
    try:
        fn = L.replica_rollout_device_consts if device_consts else L.replica_rollout
        fn(ctypes.byref(problem), v_sc.ctypes.data_as(_P), b_sc.ctypes.data_as(_P), n, ns,
           INTEGRATORS[integ], states.ctypes.data_as(_P), costs.ctypes.data_as(_P))
        if device_estimates:
            assert L.replica_rcp_misses() == 0, "a denominator without its device estimate"
    finally:
        if device_estimates:
            L.replica_set_rcp_table(None, None, 0)
    return states, costs


def replica_cum_sums(problem, v_sc, b_sc, device_estimates=False):
    """The rect+cum recurrence's sums after every step, as the lane hook's loop()
    sees them -> (sums [N,2,C], bad [C] bool), one-shot (host) constants;
    device_estimates as replica_rollout."""
    v_sc = np.ascontiguousarray(v_sc, dtype=np.float64)
    b_sc = np.ascontiguousarray(b_sc, dtype=np.float64)
    ns, n = v_sc.shape
    sums, bad = np.empty((ns, 2, n)), np.full(n, 7, dtype=np.uint8)
    L = replica_lib()
    L.replica_cum_sums.argtypes = [_P, _P, _P, ctypes.c_int64, ctypes.c_int32, _P, _P]
    L.replica_cum_sums.restype = None
    if device_estimates:            # every denominator of b_sc, a NaN's too: replica_rollout's table
        q = np.empty_like(np.unique(b_sc))
        L.replica_tan_q(np.unique(b_sc).ctypes.data_as(_P), len(q), q.ctypes.data_as(_P))
        q = np.unique(q)
        r = device_rcp(q)
        L.replica_set_rcp_table(q.ctypes.data_as(_P), r.ctypes.data_as(_P), len(q))
    try:
        L.replica_cum_sums(ctypes.byref(problem), v_sc.ctypes.data_as(_P),
                           b_sc.ctypes.data_as(_P), n, ns, sums.ctypes.data_as(_P),
                           bad.ctypes.data_as(_P))
        if device_estimates:
            assert L.replica_rcp_misses() == 0, "a denominator without its device estimate"
    finally:
        if device_estimates:
            L.replica_set_rcp_table(None, None, 0)
    assert set(np.unique(bad)) <= {0, 1}
    return sums, bad.astype(bool)


def _install_device_estimates(L, beta):
    """The device's reciprocal estimates of every tan_small denominator of beta."""
    beta = np.unique(np.ascontiguousarray(beta, dtype=np.float64))
    beta = beta[np.isfinite(beta)]
    q = np.empty_like(beta)
    L.replica_tan_q(beta.ctypes.data_as(_P), len(beta), q.ctypes.data_as(_P))
    q = np.unique(q)
    r = device_rcp(q)
    L.replica_set_rcp_table(q.ctypes.data_as(_P), r.ctypes.data_as(_P), len(q))


@contextlib.contextmanager
def estimates_installed(beta, device=True):
    """One table of the device's reciprocal estimates (one fetch, of every
    tan_small denominator of `beta`) kept installed across any number of
    replica_rollout calls (device_estimates=False in them: that flag fetches
    and removes a table per call).  Yields replica_rcp_misses, to be asserted 0
    before the block ends.  device=False (a CPU run): nothing is fetched, the
    host's 1.0 / q serves, and the count is 0."""
    L = replica_lib()
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    on = bool(device) and beta[np.isfinite(beta)].size > 0
    if on:
        _install_device_estimates(L, beta)
    try:
        yield (lambda: int(L.replica_rcp_misses())) if on else (lambda: 0)
    finally:
        if on:
            L.replica_set_rcp_table(None, None, 0)


def replica_fulltree(problem, V, B, integ="rect", device_estimates=False, device_consts=False,
                     leaves=()):
    """Host replica of the full-tree arithmetic (csrc/mpc_ftdevice.h and the
    control derivation of k_ft_controls) -> (costs [S1^3] in leaf order, no_rot,
    layer states [len(leaves), 3, 3] of `leaves`).  problem: MpcFulltreeProblem; V, B: the grids.
    device_consts: the batched entry's constants (the robot's by
    consts_from_problem, the control table's from the window alone) instead of
    the one-shot entry's host constants.  device_estimates: as replica_rollout
    (the table's tangent is tan_fast, whose reciprocal is Newton-corrected to
    the rounded quotient and asks for no estimate today; the table is installed
    all the same and zero misses asserted, so that a tangent that does ask for
    one cannot go unnoticed)."""
    from diplomjourney_amd.abi import INTEGRATORS
    V = np.ascontiguousarray(V, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    s1 = len(V) * len(B)
    costs = np.empty(s1 ** 3)
    flag = ctypes.c_int32(-1)
    L = replica_lib()
    if device_estimates:
        _install_device_estimates(L, B)
    lv = np.ascontiguousarray(leaves, dtype=np.int64)
    trajs = np.full((len(lv), 3, 3), np.nan)
    try:
        rc = L.replica_fulltree(ctypes.byref(problem), V.ctypes.data_as(_P), len(V),
                                B.ctypes.data_as(_P), len(B), INTEGRATORS[integ],
                                int(device_consts), costs.ctypes.data_as(_P), ctypes.byref(flag),
                                lv.ctypes.data_as(_P), len(lv), trajs.ctypes.data_as(_P))
        assert rc == 0, f"replica_fulltree: mode {integ}"
        if device_estimates:
            assert L.replica_rcp_misses() == 0, "a denominator without its device estimate"
    finally:
        if device_estimates:
            L.replica_set_rcp_table(None, None, 0)
    return costs, flag.value, trajs
