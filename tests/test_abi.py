"""The C-ABI library: builds, loads, exports every symbol include/mpc_rollout.h
declares, agrees with the ctypes struct layout, and validates arguments
before touching the GPU.  CPU only (no compute calls)."""
import ctypes
import os
import re
import subprocess

import pytest

from diplomjourney_amd import abi, native

HEADER = native.HEADER


def _declared():
    """The functions the header declares for the library to export (its static
    inline helpers, defined in the header itself, excluded)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    inline = set(re.findall(r"static\s+inline\s+[a-z_0-9]+\s+(mpc_[a-z_0-9]+)\s*\(", text))
    return set(re.findall(r"\b(mpc_[a-z_0-9]+)\s*\(", text)) - inline


@pytest.fixture(scope="module")
def so():
    if native.needs_build():
        native.build()
    return ctypes.CDLL(native.LIB_PATH)


def test_exports_match_header(so):
    declared = _declared()
    assert declared == set(native.EXPORTS)
    for name in declared:
        assert hasattr(so, name), name


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t}


def _prototypes():
    """{entry: (return type, [parameter types])} of the header's exported
    functions, each type as its C text without the parameter's name."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9 ]*?[\s*]+)(mpc_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        ret, name, params = m.group(1), m.group(2), m.group(3)
        if "static" in ret or "typedef" in ret:
            continue
        types_ = []
        if params.strip() != "void":
            for p in params.split(","):
                # drop the parameter's name (any case: `double L`), keep `*`s.  Every
                # parameter of the header is named; an unnamed scalar would lose its
                # type here and fail the comparison, not pass it.
                types_.append(re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*\s*$", "", " ".join(p.split())).strip())
        out[name] = (" ".join(ret.split()), types_)
    return out


def _agrees(c_type, ct):
    """Does a ctypes type stand for this C type?"""
    if "*" in c_type or c_type in ("mpc_stream_t", "mpc_comm_t"):
        return (ct in (ctypes.c_void_p, ctypes.c_char_p)
                or isinstance(ct, type) and issubclass(ct, ctypes._Pointer))
    want = _SCALARS.get(c_type.replace("const ", ""))
    if want is None or not (isinstance(ct, type) and issubclass(ct, ctypes._SimpleCData)) \
            or ct in (ctypes.c_void_p, ctypes.c_char_p):
        return False

    def kind(t):                            # width, signedness, floating point
        return ctypes.sizeof(t), t(-1).value < 0, t._type_ in "fdg"
    return kind(ct) == kind(want)


def test_prototypes_match_header():
    """native.PROTOTYPES against every prototype of the header: present, the
    same arity, and every parameter and the return value of the same kind
    (pointer / handle, or a scalar of the same width and signedness)."""
    protos = _prototypes()
    assert set(protos) == _declared()
    table = native.PROTOTYPES
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        if name not in table:
            wrong.append((name, "not in PROTOTYPES"))
            continue
        restype, argtypes = table[name]
        if argtypes is None or len(argtypes) != len(params):
            wrong.append((name, f"arity {None if argtypes is None else len(argtypes)} != {len(params)}"))
            continue
        if not _agrees(ret, restype):
            wrong.append((name, f"returns {ret}, bound {restype}"))
        for i, (c, ct) in enumerate(zip(params, argtypes)):
            if not _agrees(c, ct):
                wrong.append((name, f"parameter {i}: {c}, bound {ct}"))
    assert not wrong, wrong
    assert set(table) == set(protos)


def test_calls_raise_with_the_entry_name():
    """native.calls(): an int-status entry raises MpcError carrying its own
    name and the status; the same call through native.lib() returns it."""
    fake = ctypes.c_void_p(0x1000)
    assert native.lib().mpc_episodes_reset(None, 1, fake, None) == abi.MPC_ERR_ARG
    with pytest.raises(abi.MpcError) as e:
        native.calls().mpc_episodes_reset(None, 1, fake, None)
    assert e.value.status == abi.MPC_ERR_ARG and "mpc_episodes_reset" in str(e.value)
    # size_t / string entries return their value, unchecked
    assert native.calls().mpc_episodes_state_bytes(0) == 0
    assert b"gfx950" in native.calls().mpc_version()


def test_binding_loads():
    L = native.lib()
    assert b"gfx950" in L.mpc_version()
    assert L.mpc_strerror(abi.MPC_ERR_WORKSPACE) == b"workspace too small"


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "mpc_rollout.h"\n'
        "int main(void){printf(\"%zu %zu %zu %zu %zu %zu\\n\", sizeof(mpc_problem_t),"
        " sizeof(mpc_result_t), offsetof(mpc_result_t, index), offsetof(mpc_result_t, found),"
        " offsetof(mpc_result_t, v), offsetof(mpc_result_t, traj)); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    R = abi.MpcResult
    assert got == [ctypes.sizeof(abi.MpcProblem), ctypes.sizeof(R), R.index.offset,
                   R.found.offset, R.v.offset, R.traj.offset]


def test_episode_struct_layouts_match_c(tmp_path):
    """mpc_episode_config_t (incl. stop_rule), mpc_episode_log_t and
    mpc_episodes_progress_t: the ctypes mirrors equal the C layouts."""
    src = tmp_path / "layout2.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "mpc_rollout.h"\n'
        "int main(void){printf(\"%zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(mpc_episode_config_t),"
        " offsetof(mpc_episode_config_t, stop_rule), offsetof(mpc_episode_config_t, seed),"
        " sizeof(mpc_episode_log_t), sizeof(mpc_episodes_progress_t),"
        " offsetof(mpc_episodes_progress_t, stop), offsetof(mpc_episodes_progress_t, candidates));"
        " return 0;}\n")
    exe = tmp_path / "layout2"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    C, P = abi.MpcEpisodeConfig, abi.MpcEpisodesProgress
    assert got == [ctypes.sizeof(C), C.stop_rule.offset, C.seed.offset,
                   ctypes.sizeof(abi.MpcEpisodeLog), ctypes.sizeof(P), P.stop.offset,
                   P.candidates.offset]


def test_batched_episodes_argument_validation_without_gpu():
    """mpc_episodes_*: sizes and rejected arguments, before any HIP call."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    assert L.mpc_episodes_state_bytes(0) == 0
    n1 = L.mpc_episodes_state_bytes(1)
    assert L.mpc_episodes_state_bytes(1000) > 1000 * ctypes.sizeof(abi.MpcEpisodeConfig) > n1 > 0
    fake = ctypes.c_void_p(0x1000)
    cfg = reference_episode_config()
    bad = reference_episode_config()
    bad.stop_rule = 2
    arr = (abi.MpcEpisodeConfig * 2)(cfg, bad)
    assert L.mpc_episodes_reset(ctypes.byref(arr), 2, fake, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_reset(None, 1, fake, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_reset(ctypes.byref(arr), 0, fake, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_run(None, 1, 3, 0, 1, None, 0, None, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_run(fake, 1, 0, 0, 1, None, 0, None, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_run(fake, 1, 3, 0, 1, fake, 0, None, None) == abi.MPC_ERR_ARG
    assert L.mpc_episodes_run(fake, 1, 3, 7, 1, None, 0, None, None) == abi.MPC_ERR_UNSUPPORTED
    assert L.mpc_episodes_run(fake, 1, 3, 0, 0, None, 0, None, None) == abi.MPC_OK   # nothing


def test_persistent_run_argument_validation_without_gpu():
    """mpc_episode_run: workspace size and rejected arguments, before any HIP
    call (epoch 0 or an epoch range past 2^32 - 1, no steps, a horizon out of
    range, a heading mode other than rect+cum, misaligned or mismatched
    tiled controls, too small a workspace)."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    n, ns = 20_000, 10
    tiles = -(-n // 512)
    wsb = L.mpc_episode_run_workspace_bytes(n)
    assert wsb == 256 + 2 * tiles * 16 and L.mpc_episode_run_workspace_bytes(1) == 0
    cfg = reference_episode_config()
    fake = 0x10000
    V = (ctypes.c_void_p * 2)(fake, fake + 16 * n)
    B = (ctypes.c_void_p * 2)(fake + 8 * n * ns, fake + 24 * n)
    cum = abi.INTEGRATORS["rect+cum"]

    def run(e0=1, k=2, nsteps=ns, integ=cum, v=V, b=B, ws=wsb, nc=n):
        return L.mpc_episode_run(ctypes.byref(cfg), ctypes.c_void_p(fake), e0, v, b, k, nc,
                                 nsteps, 0, integ, ctypes.c_void_p(fake), ws, ctypes.c_void_p(fake),
                                 None, 0, None)

    assert run(e0=0) == abi.MPC_ERR_ARG
    assert run(e0=0xFFFFFFFF) == abi.MPC_ERR_ARG          # epochs would wrap to 0
    assert run(k=0) == abi.MPC_ERR_ARG
    assert run(nsteps=0) == abi.MPC_ERR_ARG
    assert run(nc=1) == abi.MPC_ERR_ARG
    assert run(integ=abi.INTEGRATORS["rect+rot"]) == abi.MPC_ERR_UNSUPPORTED
    Bm = (ctypes.c_void_p * 2)(fake + 8, fake + 24 * n)   # misaligned beta row
    assert run(b=Bm) == abi.MPC_ERR_UNSUPPORTED
    Bt = (ctypes.c_void_p * 2)(fake + 8 * 512, fake + 8)  # tiled: beta must be v + 512
    assert run(integ=cum | abi.MPC_LAYOUT_TILED, b=Bt) == abi.MPC_ERR_UNSUPPORTED
    assert run(ws=wsb - 1) == abi.MPC_ERR_WORKSPACE


def test_workspace_sizes():
    L = native.lib()
    assert L.mpc_workspace_bytes(1, 3) == 16
    assert L.mpc_workspace_bytes(10**7, 12) == 2048 * 16   # capped grid
    assert L.mpc_batched_workspace_bytes(4, 10_000, 8) == 4 * 40 * 16


def test_argument_validation_without_gpu():
    """Invalid arguments are rejected before any HIP call."""
    L = native.lib()
    p = abi.make_problem(0, 0, 0, 2, 3, 0, 0, 0.5, 0.05, 0.1)
    fake = ctypes.c_void_p(0x1000)
    args = dict(v=fake, b=fake, n=100, ns=3, base=0, inc=1e300, integ=0, st=None, ws=fake,
                wsb=1 << 20, out=fake)

    def call(**kw):
        a = {**args, **kw}
        return L.mpc_rollout_argmin(ctypes.byref(p), a["v"], a["b"], a["n"], a["ns"], a["base"],
                                    a["inc"], a["integ"], a["st"], a["ws"], a["wsb"], a["out"],
                                    None)

    assert call(n=0) == abi.MPC_ERR_ARG
    assert call(ns=0) == abi.MPC_ERR_ARG
    assert call(ns=abi.MPC_MAX_STEPS + 1) == abi.MPC_ERR_ARG
    assert call(v=None) == abi.MPC_ERR_ARG
    assert call(out=None) == abi.MPC_ERR_ARG
    assert call(base=-1) == abi.MPC_ERR_ARG
    assert call(integ=7) == abi.MPC_ERR_UNSUPPORTED
    assert call(wsb=8) == abi.MPC_ERR_WORKSPACE
    assert L.mpc_rollout_argmin(None, fake, fake, 10, 3, 0, 1.0, 0, None, fake, 1 << 20, fake,
                                None) == abi.MPC_ERR_ARG
    assert L.mpc_select_winner(None, 1, 1.0, fake, None) == abi.MPC_ERR_ARG
    assert L.mpc_sample_controls(fake, 3, fake, 4, 10, 3, 1, 0, 1, fake, fake, 5,
                                 None) == abi.MPC_ERR_ARG  # ld < n_cand
    assert L.mpc_rollout_argmin_batched(fake, None, 0, fake, fake, 10, 3, 0, fake, 1 << 20,
                                        fake, None) == abi.MPC_ERR_ARG
    # the verification probe: nothing to do, a negative count, missing arrays
    assert L.mpc_rcp_estimate(None, None, 0, None) == abi.MPC_OK
    assert L.mpc_rcp_estimate(fake, fake, -1, None) == abi.MPC_ERR_ARG
    assert L.mpc_rcp_estimate(None, fake, 4, None) == abi.MPC_ERR_ARG


def test_no_cpu_fallback(monkeypatch, tmp_path):
    """The product binding raises when the HIP library is absent."""
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native, "LIB_PATH", str(tmp_path / "missing.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.lib()


def test_p2p_exchange_argument_validation_without_gpu():
    """mpc_mailbox_* / mpc_ipc_* / mpc_episode_p2p_*: sizes and rejected
    arguments, before any HIP call."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    assert L.mpc_mailbox_bytes(0) == 0 and L.mpc_mailbox_bytes(33) == 0
    one, eight = L.mpc_mailbox_bytes(1), L.mpc_mailbox_bytes(8)
    # header (32 peer pointers, rank, world, 32 ping words; 256-B padded), then
    # two slots of one candidate per rank, each 8-B word as a 16-B tagged granule
    rec = abi.CANDIDATE_BYTES * 2
    hdr = one - 2 * rec
    assert eight - one == 2 * 7 * rec and hdr % 256 == 0 and hdr >= 32 * 8 * 2 + 8
    out = ctypes.c_void_p()
    assert L.mpc_mailbox_alloc(0, 1, ctypes.byref(out)) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_alloc(2, 1, None) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_free(None) == abi.MPC_ERR_ARG
    assert L.mpc_ipc_handle(None, None) == abi.MPC_ERR_ARG
    assert L.mpc_ipc_open(None, ctypes.byref(out)) == abi.MPC_ERR_ARG
    assert L.mpc_ipc_close(None) == abi.MPC_ERR_ARG
    f = ctypes.c_void_p(0x1000)
    g = ctypes.c_void_p(0x2000)
    peers = (ctypes.c_void_p * 2)(f, g)
    assert L.mpc_mailbox_set_peers(None, 0, 2, peers) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_set_peers(f, 2, 2, peers) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_set_peers(f, 1, 2, peers) == abi.MPC_ERR_ARG   # own row != mailbox
    assert L.mpc_mailbox_set_peers(f, 0, 33, peers) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_ping(None, 1, f, None) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_ping(f, 0, f, None) == abi.MPC_ERR_ARG
    assert L.mpc_mailbox_ping(f, 1, None, None) == abi.MPC_ERR_ARG
    cfg = reference_episode_config()
    ig = abi.INTEGRATORS["rect+cum"]

    def step(epoch=3, prev=2, mailbox=f, world=2, out_prev=f, ws_prev=f, v_prev=f):
        return L.mpc_episode_p2p_step(ctypes.byref(cfg), f, epoch, prev, f, f, 1024, 10, 0, ig,
                                      f, ws_prev, 1 << 20, v_prev, f, mailbox, world, out_prev,
                                      f, 8, None)
    assert step(epoch=0) == abi.MPC_ERR_ARG
    assert step(prev=1) == abi.MPC_ERR_ARG             # same parity: same mailbox slot
    assert step(mailbox=None) == abi.MPC_ERR_ARG
    assert step(world=0) == abi.MPC_ERR_ARG
    assert step(world=33) == abi.MPC_ERR_ARG
    assert step(out_prev=None) == abi.MPC_ERR_ARG      # a previous step to complete ...
    assert step(ws_prev=None) == abi.MPC_ERR_ARG       # ... from its records
    assert step(v_prev=None) == abi.MPC_ERR_ARG        # ... and controls

    def flush(epoch=3, mailbox=f, world=2, out=f, ws=f):
        return L.mpc_episode_p2p_flush(ctypes.byref(cfg), f, epoch, f, f, 1024, 10, 0, ig, ws,
                                       1 << 20, mailbox, world, out, f, 8, None)
    assert flush(epoch=0) == abi.MPC_ERR_ARG
    assert flush(mailbox=None) == abi.MPC_ERR_ARG
    assert flush(world=0) == abi.MPC_ERR_ARG
    assert flush(out=None) == abi.MPC_ERR_ARG
    assert flush(ws=None) == abi.MPC_ERR_ARG


def test_tiled_layout_argument_validation_without_gpu():
    """MPC_LAYOUT_TILED: accepted only by the chained one-GPU / P2P entries and
    their flush; the tiled buffer's beta must be its base + 512, n_cand even.
    Every rejection happens before any HIP call."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    cfg = reference_episode_config()
    t = abi.MPC_LAYOUT_TILED
    cum = abi.INTEGRATORS["rect+cum"]
    base = ctypes.c_void_p(0x10000)
    b_ok = ctypes.c_void_p(0x10000 + 8 * abi.MPC_TILE)
    b_bad = ctypes.c_void_p(0x20000)
    f = ctypes.c_void_p(0x1000)

    def chain(integ=cum | t, v=base, b=b_ok, n=1024):
        return L.mpc_episode_chain_step(ctypes.byref(cfg), f, 1, 1, v, b, n, 10, 0, integ, f, f,
                                        1 << 24, None, None, f, None, 0, f, 8, None)
    assert chain(b=b_bad) == abi.MPC_ERR_UNSUPPORTED          # beta != base + 512
    assert chain(n=1023) == abi.MPC_ERR_UNSUPPORTED           # two candidates per lane
    assert chain(v=ctypes.c_void_p(0x10008), b=ctypes.c_void_p(0x10008 + 4096)) == \
        abi.MPC_ERR_UNSUPPORTED                               # 16-B aligned base
    assert chain(integ=abi.INTEGRATORS["rect"] | t) == abi.MPC_ERR_UNSUPPORTED   # chained: +cum
    # entries that read SoA controls refuse the flag
    assert L.mpc_episode_partials(f, base, b_ok, 1024, 10, cum | t, f, 1 << 24, None) == \
        abi.MPC_ERR_UNSUPPORTED
    assert L.mpc_episode_exchange_step(ctypes.byref(cfg), f, 1, base, b_ok, 1024, 10, 0, cum | t,
                                       f, 1 << 24, None, 0, f, f, f, 8, None) == \
        abi.MPC_ERR_UNSUPPORTED
    # the flush of a tiled chained step needs the episode update (advance)
    assert L.mpc_episode_finalize(f, base, b_ok, 1024, 10, 0, cum | t, f, 1 << 24, f, None, f,
                                  8, None) == abi.MPC_ERR_UNSUPPORTED
    sink = ctypes.c_void_p(0x40000)
    assert L.mpc_stream_probe_tiled(ctypes.c_void_p(0x10008), 1024, 10, sink, 1 << 30, None) == \
        abi.MPC_ERR_UNSUPPORTED
    assert L.mpc_stream_probe_tiled(base, 1024, 0, sink, 1 << 30, None) == abi.MPC_ERR_ARG
    assert L.mpc_sample_controls_tiled(f, 3, f, 4, 1023, 10, 1, 0, 1, base, None) == \
        abi.MPC_ERR_ARG


def test_tiled_index_header_matches_python(tmp_path):
    """The header's mpc_tiled_index (C) == soa_to_tiled / tiled_to_soa
    (torch, CPU): every candidate and step of a ragged last tile."""
    import torch
    from diplomjourney_amd.expansion import soa_to_tiled, tiled_to_soa
    n, ns = 1300, 3
    src = tmp_path / "ti.c"
    src.write_text(
        '#include <stdio.h>\n#include "mpc_rollout.h"\n'
        "int main(void) { for (int s = 0; s < %d; ++s) for (long c = 0; c < %d; ++c)"
        ' printf("%%ld\\n", (long)mpc_tiled_index(c, s, %d)); return 0; }\n' % (ns, n, ns))
    exe = tmp_path / "ti"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)],
                   check=True)
    idx = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    v = torch.arange(ns * n, dtype=torch.float64).reshape(ns, n)
    b = -v - 1
    t = soa_to_tiled(v, b)
    flat = t.reshape(-1)
    for s in range(ns):
        for c in range(0, n, 7):
            o = idx[s * n + c]
            assert flat[o] == v[s, c] and flat[o + abi.MPC_TILE] == b[s, c]
    v2, b2 = tiled_to_soa(t, n)
    assert torch.equal(v2, v) and torch.equal(b2, b)


def _chained_entry_calls():
    """{entry: call(**overrides)} over fake pointers.  Every default is an
    acceptable argument, so a case is wrong exactly where its overrides say
    (and none may be called without an override: the call would launch)."""
    from diplomjourney_amd.episode import reference_episode_config
    L = native.lib()
    cfg = reference_episode_config()
    cfg.enumerate = 0
    f = ctypes.c_void_p(0x1000)
    g = ctypes.c_void_p(0x2000)
    cum = abi.INTEGRATORS["rect+cum"]
    base = dict(cfg=cfg, state=f, v=f, b=g, n=1024, ns=10, base=0, integ=cum, ws=f, wsb=1 << 24,
                out=f, log=f, cap=8, epoch=3)

    def entry(fn, **extra):
        return lambda **kw: fn({**base, **extra, **kw})

    def ref(c):
        return ctypes.byref(c) if c is not None else None

    def chain(a):
        return L.mpc_episode_chain_step(
            ref(a["cfg"]), a["state"], a["mode"], a["epoch"], a["v"], a["b"], a["n"], a["ns"],
            a["base"], a["integ"], a["ws"], a["ws_prev"], a["wsb"], a["v_prev"], a["b_prev"],
            a["out"], None, 0, a["log"], a["cap"], None)

    def exchange2(a):
        return L.mpc_episode_exchange_step2(
            ref(a["cfg"]), a["state"], a["epoch"], a["wait_tag"], a["v"], a["b"], a["n"], a["ns"],
            a["base"], a["integ"], a["ws"], a["wsb"], a["gathered"], a["n_gathered"], a["out"],
            a["local"], a["log"], a["cap"], None)

    def p2p_step(a):
        return L.mpc_episode_p2p_step(
            ref(a["cfg"]), a["state"], a["epoch"], a["prev"], a["v"], a["b"], a["n"], a["ns"],
            a["base"], a["integ"], a["ws"], a["ws_prev"], a["wsb"], a["v_prev"], a["b_prev"],
            a["mailbox"], a["world"], a["out"], a["log"], a["cap"], None)

    def p2p_flush(a):
        return L.mpc_episode_p2p_flush(
            ref(a["cfg"]), a["state"], a["epoch"], a["v"], a["b"], a["n"], a["ns"], a["base"],
            a["integ"], a["ws"], a["wsb"], a["mailbox"], a["world"], a["out"], a["log"], a["cap"],
            None)

    def run(a):
        V = (ctypes.c_void_p * 2)(a["v"], a["v2"])
        B = (ctypes.c_void_p * 2)(a["b"], a["b2"])
        return L.mpc_episode_run(
            ref(a["cfg"]), a["state"], a["epoch"], V, B, 2, a["n"], a["ns"], a["base"], a["integ"],
            a["ws"], a["wsb"], a["out"], a["log"], a["cap"], None)

    def generate(a):
        return L.mpc_episode_generate_step(
            ref(a["cfg"]), a["state"], a["n"], a["ns"], a["base"], a["integ"], a["ws"], a["wsb"],
            a["out"], a["log"], a["cap"], None)

    def fin(fn):
        return lambda a: fn(a["state"], a["v"], a["b"], a["n"], a["ns"], a["base"], a["integ"],
                            a["ws"], a["wsb"], a["out"], ref(a["advance"]), a["log"], a["cap"], None)

    return {
        "chain_step": entry(chain, mode=1, ws_prev=f, v_prev=None, b_prev=None),
        "exchange_step2": entry(exchange2, wait_tag=0, gathered=None, n_gathered=0, local=f),
        "p2p_step": entry(p2p_step, prev=2, ws_prev=f, v_prev=f, b_prev=g, mailbox=f, world=2),
        "p2p_flush": entry(p2p_flush, mailbox=f, world=2),
        "run": entry(run, v2=ctypes.c_void_p(0x100000), b2=ctypes.c_void_p(0x200000)),
        "generate_step": entry(generate),
        "finalize": entry(fin(L.mpc_episode_finalize), advance=None),
        "rollout": entry(fin(L.mpc_episode_rollout), advance=None),
    }


def test_chained_entries_status_precedence_without_gpu():
    """Which status each chained-episode entry (and finalize / rollout) returns
    when a call is wrong in two classes at once, and for the conditions of its
    preamble no other test reaches.  Every expected value is what the library
    returned before the entries shared their validation helpers; every call
    returns before any HIP call (and before the entry's wall-clock check)."""
    from diplomjourney_amd.episode import reference_episode_config
    A, U, W = abi.MPC_ERR_ARG, abi.MPC_ERR_UNSUPPORTED, abi.MPC_ERR_WORKSPACE
    f = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x2008)                      # not 16-B aligned
    cum = abi.INTEGRATORS["rect+cum"]
    tiled = cum | abi.MPC_LAYOUT_TILED
    arg, integ, layout, small = dict(ns=0), dict(integ=7), dict(b=odd), dict(wsb=8)
    enum = reference_episode_config()
    enum.enumerate = 1
    bad_cfg = reference_episode_config()
    bad_cfg.stop_rule = 2
    ok_cfg = reference_episode_config()
    late = dict(advance=ok_cfg, cap=-1)                # finalize / rollout: checked after the workspace
    prev = dict(v_prev=f, b_prev=None)                 # chain_step: checked after the workspace
    two_classes = [({**arg, **integ}, A), ({**layout, **small}, U), ({**arg, **small}, A)]
    preamble = [(dict(cap=-1), A), (dict(base=-1), A)]
    cases = {
        "chain_step": two_classes + preamble + [
            (dict(epoch=0), A), (dict(mode=2), A), (dict(mode=0), A), (dict(integ=1), U),
            (prev, A), ({**prev, **small}, W), ({**prev, **integ}, U), ({**prev, **layout}, U),
            (dict(v_prev=f, b_prev=odd), A)],
        "exchange_step2": two_classes + preamble + [
            (dict(epoch=0), A), (dict(local=None), A), (dict(out=None), A), (dict(n=1 << 31), A),
            (dict(gathered=f, n_gathered=0), A), (dict(wait_tag=1), A),
            (dict(wait_tag=1, gathered=f, n_gathered=33), A),
            (dict(wait_tag=1, gathered=f, n_gathered=33, integ=7), A),
            (dict(wait_tag=1, gathered=f, n_gathered=33, wsb=8), A), (dict(integ=tiled), U)],
        "p2p_step": two_classes + preamble + [
            (dict(v_prev=odd), U), (dict(v_prev=odd, wsb=8), U), (dict(v_prev=None, wsb=8), A),
            (dict(prev=1, integ=7), A), (dict(integ=1, wsb=8), U)],
        "p2p_flush": two_classes + preamble + [
            (dict(ws=None, integ=7), A), (dict(ws=None, wsb=8), A), (dict(integ=1, wsb=8), U)],
        "run": two_classes + preamble + [
            (dict(out=None), A), (dict(n=1 << 31), A), (dict(n=1 << 31, integ=7), A),
            (dict(b2=odd), U), (dict(b2=odd, wsb=8), U), (dict(v2=None), U),
            (dict(ws=None), W), (dict(integ=1, wsb=8), U)],
        "generate_step": [
            ({**arg, **integ}, A), ({**arg, **small}, A), (dict(cfg=enum, wsb=8), U),
            (dict(n=1023, integ=7), A), (dict(n=1023, wsb=8), A), (dict(n=1023, cfg=enum), A),
            (dict(n=1023), A), (dict(cfg=enum), U), (dict(cfg=bad_cfg), A), (dict(out=None), A),
            ({**integ, **small}, U)] + preamble,
        "finalize": [
            ({**arg, **integ}, A), ({**arg, **small}, A), (dict(integ=tiled, wsb=8), U),
            (dict(integ=tiled, advance=ok_cfg, b=odd, wsb=8), U), (dict(base=-1), A),
            (dict(out=None), A), (late, A), ({**late, **small}, W), ({**late, **integ}, U),
            (dict(advance=bad_cfg), A), (dict(advance=bad_cfg, wsb=8), W),
            (dict(integ=abi.INTEGRATORS["rect"] | abi.MPC_LAYOUT_TILED, advance=ok_cfg), U)],
        "rollout": [
            ({**arg, **integ}, A), ({**arg, **small}, A), (dict(integ=tiled, wsb=8), U),
            (dict(base=-1), A), (dict(out=None), A), (late, A), ({**late, **small}, W),
            ({**late, **integ}, U), (dict(advance=bad_cfg), A), (dict(advance=bad_cfg, wsb=8), W)],
    }
    calls = _chained_entry_calls()
    assert set(cases) == set(calls)
    wrong = []
    for name, rows in cases.items():
        for kw, want in rows:
            assert kw, "a call without a fault would launch"
            got = calls[name](**kw)
            if got != want:
                wrong.append((name, {k: getattr(v, "value", v) for k, v in kw.items()}, got, want))
    assert not wrong, wrong
