"""ctypes binding of the HIP library libmpc_rollout.so (include/mpc_rollout.h).

The product path has no CPU fallback: if the in-tree library is missing or a
call returns a non-zero status, this module raises.  Device buffers come from
PyTorch-ROCm tensors (`tensor.data_ptr()`), the stream from
`native.current_stream()`.  torch is imported first so the library's
libamdhip64.so.7 dependency resolves to the runtime torch already loaded (one
HIP runtime per process).

PROTOTYPES holds every entry's signature (tests/test_abi.py compares it with
the header).  Two handles are made from it: `lib()`, whose entries return their
status, and `calls()`, whose entries raise MpcError(status, entry name).
"""
import ctypes
import os
import subprocess
import sys
import types
from ctypes import POINTER, c_char_p, c_int, c_size_t, c_uint32, c_uint64

import torch  # before the library loads: one HIP runtime, torch's libamdhip64.so.7

from .abi import MpcEpisodeConfig, MpcError, MpcFulltreeProblem, MpcProblem

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_NAME = "libmpc_rollout.so"
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)
SRC = os.path.join(PKG_DIR, "csrc", "mpc_rollout.hip")
# every translation unit of the library, SRC first (csrc/mpc_episodes_obs_launch.h
# says why the second one is apart)
SOURCES = (SRC, os.path.join(PKG_DIR, "csrc", "mpc_episodes_obs.hip"))
HEADER = os.path.join(REPO_DIR, "include", "mpc_rollout.h")

_P = ctypes.c_void_p           # any device / host pointer, mpc_stream_t, mpc_comm_t
_PP = POINTER(_P)              # pointer arrays and handle out-parameters (byref)
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_D = ctypes.c_double
_PROB = POINTER(MpcProblem)
_CFG = POINTER(MpcEpisodeConfig)
# mpc_episode_finalize / _step / _rollout: one signature
_FINALIZE = [_P, _P, _P, _I64, _I32, _I64, _I32, _P, c_size_t, _P, _CFG, _P, _I32, _P]

# entry -> (restype, argtypes): every function include/mpc_rollout.h declares
PROTOTYPES = {
    "mpc_version": (c_char_p, []),
    "mpc_strerror": (c_char_p, [c_int]),
    "mpc_workspace_bytes": (c_size_t, [_I64, _I32]),
    "mpc_rollout_argmin": (c_int, [_PROB, _P, _P, _I64, _I32, _I64, _D, _I32, _P, _P, c_size_t,
                                   _P, _P]),
    "mpc_rollout_partials": (c_int, [_PROB, _P, _P, _I64, _I32, _I32, _P, _P, c_size_t, _P]),
    "mpc_rollout_finalize": (c_int, [_PROB, _P, _P, _I64, _I32, _I64, _D, _I32, _I32, _P,
                                     c_size_t, _P, _P]),
    "mpc_rollout_partials_obstacles": (c_int, [_PROB, _P, _I32, _P, _P, _I64, _I32, _I32, _P, _P,
                                               c_size_t, _P, _P]),
    "mpc_rollout_argmin_obstacles": (c_int, [_PROB, _P, _I32, _P, _P, _I64, _I32, _I64, _D, _I32,
                                             _P, _P, c_size_t, _P, _P, _P]),
    # ... with keep-out polygons: (polygons, count) after the circles
    "mpc_rollout_partials_keepout": (c_int, [_PROB, _P, _I32, _P, _I32, _P, _P, _I64, _I32, _I32,
                                             _P, _P, c_size_t, _P, _P]),
    "mpc_rollout_argmin_keepout": (c_int, [_PROB, _P, _I32, _P, _I32, _P, _P, _I64, _I32, _I64, _D,
                                           _I32, _P, _P, c_size_t, _P, _P, _P]),
    "mpc_batched_workspace_bytes": (c_size_t, [_I32, _I64, _I32]),
    "mpc_rollout_argmin_batched": (c_int, [_P, _P, _I32, _P, _P, _I64, _I32, _I32, _P, c_size_t,
                                           _P, _P]),
    "mpc_select_winner": (c_int, [_P, _I32, _D, _P, _P]),
    "mpc_stream_probe": (c_int, [_P, _P, _I64, _I32, _P, c_size_t, _P]),
    "mpc_stream_probe_tiled": (c_int, [_P, _I64, _I32, _P, c_size_t, _P]),
    "mpc_rcp_estimate": (c_int, [_P, _P, _I64, _P]),
    "mpc_sample_controls": (c_int, [_P, _I32, _P, _I32, _I64, _I32, c_uint64, _I64, _I32, _P, _P,
                                    _I64, _P]),
    "mpc_sample_controls_tiled": (c_int, [_P, _I32, _P, _I32, _I64, _I32, c_uint64, _I64, _I32,
                                          _P, _P]),
    # the device-resident episode
    "mpc_episode_state_bytes": (c_size_t, []),
    "mpc_episode_reset": (c_int, [_CFG, _P, _P]),
    "mpc_episode_expand": (c_int, [_CFG, _P, _P, _P, _I64, _I32, _I64, _I32, _P, c_size_t, _P,
                                   _P]),
    "mpc_episode_advance": (c_int, [_CFG, _P, _P, _I32, _P, _I32, _P]),
    "mpc_episode_rollout": (c_int, _FINALIZE),
    "mpc_episode_sample": (c_int, [_CFG, _P, _P, _P, _I64, _I32, _I64, _P]),
    "mpc_episode_partials": (c_int, [_P, _P, _P, _I64, _I32, _I32, _P, c_size_t, _P]),
    "mpc_episode_finalize": (c_int, _FINALIZE),
    "mpc_episode_step": (c_int, _FINALIZE),
    "mpc_episode_chain_step": (c_int, [_CFG, _P, _I32, c_uint32, _P, _P, _I64, _I32, _I64, _I32,
                                       _P, _P, c_size_t, _P, _P, _P, _P, _I32, _P, _I32, _P]),
    # ... with keep-out circles: the base entry's arguments, + (circles, count)
    # after the state, + n_blocked_out before the stream
    "mpc_episode_partials_obstacles": (c_int, [_P, _P, _I32, _P, _P, _I64, _I32, _I32, _P,
                                               c_size_t, _P, _P]),
    "mpc_episode_step_obstacles": (c_int, _FINALIZE[:1] + [_P, _I32] + _FINALIZE[1:-1] + [_P, _P]),
    "mpc_episode_chain_step_obstacles": (c_int, [_CFG, _P, _P, _I32, _I32, c_uint32, _P, _P, _I64,
                                                 _I32, _I64, _I32, _P, _P, c_size_t, _P, _P, _P,
                                                 _P, _I32, _P, _I32, _P, _P]),
    # ... and keep-out polygons: (polygons, count) after the circles
    "mpc_episode_partials_keepout": (c_int, [_P, _P, _I32, _P, _I32, _P, _P, _I64, _I32, _I32, _P,
                                             c_size_t, _P, _P]),
    "mpc_episode_step_keepout": (c_int, _FINALIZE[:1] + [_P, _I32, _P, _I32] + _FINALIZE[1:-1]
                                 + [_P, _P]),
    "mpc_episode_chain_step_keepout": (c_int, [_CFG, _P, _P, _I32, _P, _I32, _I32, c_uint32, _P, _P,
                                               _I64, _I32, _I64, _I32, _P, _P, c_size_t, _P, _P,
                                               _P, _P, _I32, _P, _I32, _P, _P]),
    "mpc_episode_run_workspace_bytes": (c_size_t, [_I64]),
    "mpc_episode_run": (c_int, [_CFG, _P, c_uint32, _PP, _PP, _I32, _I64, _I32, _I64, _I32, _P,
                                c_size_t, _P, _P, _I32, _P]),
    "mpc_episode_exchange_step": (c_int, [_CFG, _P, c_uint32, _P, _P, _I64, _I32, _I64, _I32, _P,
                                          c_size_t, _P, _I32, _P, _P, _P, _I32, _P]),
    "mpc_episode_exchange_step2": (c_int, [_CFG, _P, c_uint32, c_uint32, _P, _P, _I64, _I32, _I64,
                                           _I32, _P, c_size_t, _P, _I32, _P, _P, _P, _I32, _P]),
    "mpc_episode_exchange_mark": (c_int, [_P, c_uint32, _P]),
    "mpc_episode_exchange_flush": (c_int, [_CFG, _P, _I32, _P, _I32, _P, _P, _I32, _P]),
    "mpc_episode_chain_error": (c_int, [_P, POINTER(_I32), _P]),
    "mpc_episode_generate_workspace_bytes": (c_size_t, [_I64, _I32]),
    "mpc_episode_generate_step": (c_int, [_CFG, _P, _I64, _I32, _I64, _I32, _P, c_size_t, _P, _P,
                                          _I32, _P]),
    # CU-masked launch streams
    "mpc_stream_create_cu_reserved": (c_int, [_I32, _PP]),
    "mpc_stream_create_cu_share": (c_int, [_I32, _I32, _PP]),
    "mpc_stream_destroy": (c_int, [_P]),
    # the P2P mailbox exchange
    "mpc_mailbox_bytes": (c_size_t, [_I32]),
    "mpc_mailbox_alloc": (c_int, [_I32, _I32, _PP]),
    "mpc_mailbox_free": (c_int, [_P]),
    "mpc_mailbox_set_peers": (c_int, [_P, _I32, _I32, _PP]),
    "mpc_mailbox_ping": (c_int, [_P, c_uint32, _P, _P]),
    "mpc_mailbox_clear": (c_int, [_P, _I32, _P]),
    "mpc_ipc_handle": (c_int, [_P, _P]),
    "mpc_ipc_open": (c_int, [_P, _PP]),
    "mpc_ipc_close": (c_int, [_P]),
    "mpc_peer_enable": (c_int, [_I32]),
    "mpc_episode_p2p_step": (c_int, [_CFG, _P, c_uint32, c_uint32, _P, _P, _I64, _I32, _I64, _I32,
                                     _P, _P, c_size_t, _P, _P, _P, _I32, _P, _P, _I32, _P]),
    "mpc_episode_p2p_flush": (c_int, [_CFG, _P, c_uint32, _P, _P, _I64, _I32, _I64, _I32, _P,
                                      c_size_t, _P, _I32, _P, _P, _I32, _P]),
    # the RCCL exchange of a non-Python host (tests/c_host)
    "mpc_comm_unique_id": (c_int, [_P]),
    "mpc_comm_init_rank": (c_int, [_P, _I32, _I32, _PP]),
    "mpc_comm_init_all": (c_int, [_I32, POINTER(_I32), _PP]),
    "mpc_comm_destroy": (c_int, [_P]),
    "mpc_exchange_allgather": (c_int, [_P, _P, _P, _P]),
    "mpc_exchange_allgather_group": (c_int, [_I32, _PP, _PP, _PP, _PP]),
    # the full tree and the batched episodes
    "mpc_fulltree_workspace_bytes": (c_size_t, [_I32, _I32]),
    "mpc_fulltree_argmin": (c_int, [POINTER(MpcFulltreeProblem), _P, _I32, _P, _I32, _D, _I32,
                                    _I32, _I32, _P, c_size_t, _P, _P]),
    "mpc_fulltree_batched_workspace_bytes": (c_size_t, [_I32, _I32, _I32]),
    "mpc_fulltree_argmin_batched": (c_int, [_P, _P, _I32, _D, _D, _D, _P, _I32, _P, _I32, _I32,
                                            _P, c_size_t, _P, _P]),
    "mpc_episodes_state_bytes": (c_size_t, [_I32]),
    "mpc_episodes_reset": (c_int, [_P, _I32, _P, _P]),
    "mpc_episodes_run": (c_int, [_P, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "mpc_episodes_run_obstacles": (c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _P,
                                           _P]),
    # the fleet call: (state, board, call0), (circles, count), clearance, reach, then
    # mpc_episodes_run's arguments from n_robots on, + n_blocked_out and neighbours_out
    "mpc_episodes_fleet_board_bytes": (c_size_t, [_I32]),
    "mpc_episodes_fleet_begin": (c_int, [_P, _I32, _P, _P]),
    "mpc_episodes_fleet_run": (c_int, [_P, _P, _I64, _P, _I32, _D, _D, _I32, _I32, _I32, _I32, _P,
                                       _I32, _P, _P, _P, _P]),
    # the predicted fleet call: the motion board after the pose board
    "mpc_episodes_fleet_motion_bytes": (c_size_t, [_I32]),
    "mpc_episodes_fleet_run_predicted": (c_int, [_P, _P, _P, _I64, _P, _I32, _D, _D, _I32, _I32,
                                                 _I32, _I32, _P, _I32, _P, _P, _P, _P]),
    # the planned fleet call: the plan board after the pose board
    "mpc_episodes_fleet_plan_bytes": (c_size_t, [_I32]),
    "mpc_episodes_fleet_run_planned": (c_int, [_P, _P, _P, _I64, _P, _I32, _D, _D, _I32, _I32,
                                               _I32, _I32, _P, _I32, _P, _P, _P, _P]),
    "mpc_fulltree_episodes_state_bytes": (c_size_t, [_I32]),
    "mpc_fulltree_episodes_reset": (c_int, [_P, _I32, _P, _P]),
    "mpc_fulltree_episodes_run": (c_int, [_P, _I32, _P, _I32, _P, _I32, _D, _D, _D, _I32, _I32,
                                          _P, _I32, _P, _P]),
    # the full tree with keep-out circles: (circles, count) after the first
    # argument, n_blocked_out before out (the episodes: before the stream)
    "mpc_fulltree_argmin_obstacles": (c_int, [POINTER(MpcFulltreeProblem), _P, _I32, _P, _I32, _P,
                                              _I32, _D, _I32, _I32, _I32, _P, c_size_t, _P, _P,
                                              _P]),
    "mpc_fulltree_argmin_batched_obstacles": (c_int, [_P, _P, _I32, _P, _I32, _D, _D, _D, _P, _I32,
                                                      _P, _I32, _I32, _P, c_size_t, _P, _P, _P]),
    "mpc_fulltree_episodes_run_obstacles": (c_int, [_P, _P, _I32, _I32, _P, _I32, _P, _I32, _D, _D,
                                                    _D, _I32, _I32, _P, _I32, _P, _P, _P]),
}

# Every symbol include/mpc_rollout.h declares (checked by tests/test_abi.py).
EXPORTS = tuple(PROTOTYPES)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# The product build's flags.  Every tool that compiles the library does so through
# compile_cmd() below, so a tool cannot analyse another build than the one that ships.
HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ldl",
    # One IEEE rounding per reference operator: no a*b+c contraction.
    "-ffp-contract=off",
    "-Wall",
]
# The timeline variant (csrc/mpc_timeline.h, tools/timeline.py): the stamps compiled in.
TIMELINE_LIB = os.path.join(REPO_DIR, "tools", "tl_variant.so")
TIMELINE_DEFINES = ("MPC_TIMELINE",)


def compile_cmd(defines=(), out=LIB_PATH, tree=REPO_DIR, extra=()):
    """The library's compile line, assembled here only.  tree: this repository,
    or a copy of another revision (SOURCES by name, without those it lacks);
    extra: a tool's analysis flags."""
    units = [os.path.join(tree, os.path.relpath(s, REPO_DIR)) for s in SOURCES]
    return [HIPCC, *HIPCC_FLAGS, *(f"-D{d}" for d in defines), "-I", os.path.join(tree, "include"),
            *extra, "-o", out, *(u for u in units if tree == REPO_DIR or os.path.exists(u))]


def build(verbose=False, defines=(), out=LIB_PATH, tree=REPO_DIR):
    """Compile csrc/*.hip for gfx950: the in-tree library, or a variant of it."""
    cmd = compile_cmd(defines, out, tree)
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return out


C_HOST_SRC = os.path.join(REPO_DIR, "tests", "c_host", "exchange_episode.cpp")
C_HOST_BIN = os.path.join(REPO_DIR, "tests", "_build", "exchange_episode")


def build_c_host(verbose=False):
    """The test-side C++ host program (tests/c_host): the sharded episode
    through the C ABI and RCCL only, linked against the in-tree library."""
    os.makedirs(os.path.dirname(C_HOST_BIN), exist_ok=True)
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I",
           os.path.join(REPO_DIR, "include"), "-o", C_HOST_BIN, C_HOST_SRC, "-L", PKG_DIR,
           "-lmpc_rollout", "-Wl,-rpath,$ORIGIN/../../diplomjourney_amd"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return C_HOST_BIN


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    lib_m = os.path.getmtime(LIB_PATH)
    srcs = [HEADER] + [os.path.join(PKG_DIR, "csrc", f) for f in os.listdir(os.path.join(PKG_DIR, "csrc"))]
    return any(os.path.getmtime(s) > lib_m for s in srcs)


_lib = None
_calls = None


def lib():
    """Load the HIP library (raises if it was not built).  Its entries return
    their status: for the callers that inspect one."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run __graft_entry__.build() "
                           "(the MPC expansion has no CPU fallback)")
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _raises(name):
    def errcheck(status, _fn, _args):
        if status != 0:
            raise MpcError(status, name)
        return status
    return errcheck


def calls():
    """The same entries for the package's own calls: a non-zero status raises
    MpcError(status, the entry's name); size_t and string entries return theirs."""
    global _calls
    if _calls is None:
        L = lib()
        C = types.SimpleNamespace()
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = L[name]            # a function object of its own: lib()'s stays unchecked
            fn.restype, fn.argtypes = restype, argtypes
            if restype is c_int:
                fn.errcheck = _raises(name)
            setattr(C, name, fn)
        _calls = C
    return _calls


def current_stream():
    """torch's current stream as the ABI's mpc_stream_t."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(status, where):
    if status != 0:
        raise MpcError(status, where)
