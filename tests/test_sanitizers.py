"""The CPU side under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY §5,
VERDICT r4 Missing #3): the C oracle (oracle/mpc_oracle.c — the restatement of
math_model_tree.py:56-115 / run_math_model.py:82-197 every parity test checks
against) and the host replica of the kernels' arithmetic (tests/
replica_harness.cpp) linked into tests/sanitize_driver.cpp, built twice with
clang (plain and -fsanitize=address,undefined, no recovery) and run on:
  * edge-size synthetic cases (empty, odd, wave +-1 shards; horizons 1..32;
    every integrator; costs + states out; batched; sampler pitch; full tree
    with every per-leaf output; the replica's estimate table);
  * the reference's 349 recorded predictive_control calls (tests/golden): the
    sanitized oracle's chosen (v, beta) and states equal the recorded ones.
The two builds must print the same checksum of every output (sanitizing
changes no bit), and a deliberate out-of-bounds read (`canary`) must be caught,
so the instrumentation is known to be live.  Host code only: no GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import call_controls, call_problem
from harness import library_headers

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BUILD = os.path.join(REPO, "oracle", "_build", "sanitize")
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
SAN_HOST = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
            "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def _build(mode):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"driver_{mode}")
    srcs = [os.path.join(REPO, "oracle", "mpc_oracle.c"), os.path.join(HERE, "sanitize_driver.cpp"),
            os.path.join(HERE, "replica_harness.cpp")]
    deps = srcs + library_headers()
    if os.path.exists(exe) and all(os.path.getmtime(s) < os.path.getmtime(exe) for s in deps):
        return exe
    obj = os.path.join(BUILD, f"oracle_{mode}.o")
    san = SAN if mode == "san" else []
    subprocess.run(["/opt/rocm/llvm/bin/clang", "-std=c11", "-O1", "-g", "-ffp-contract=off",
                    "-fno-fast-math", "-fno-builtin", "-fPIC", *san, "-I",
                    os.path.join(REPO, "include"), "-c", srcs[0], "-o", obj], check=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1",
                    "-g", "-ffp-contract=off", *(SAN_HOST if mode == "san" else []), "-I",
                    os.path.join(REPO, "include"), srcs[1], "-x", "none", obj, "-o", exe, *san,
                    "-w"], check=True)
    return exe


@pytest.fixture(scope="module")
def drivers():
    return {m: _build(m) for m in ("plain", "san")}


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=ENV)
    return r.returncode, r.stdout.strip(), r.stderr


def test_sanitizer_is_live(drivers):
    rc, _, err = _run(drivers["san"], "canary")
    assert rc != 0 and "AddressSanitizer" in err, (rc, err[-2000:])


def test_synthetic_cases_clean_and_bit_identical(drivers):
    rc_p, out_p, _ = _run(drivers["plain"], "synth")
    rc_s, out_s, err = _run(drivers["san"], "synth")
    assert rc_p == 0 and out_p.endswith("rc 0"), out_p
    assert rc_s == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    assert out_s == out_p            # same checksum of every output


def test_reference_calls_under_sanitizers(drivers, scenario, tmp_path):
    from diplomjourney_amd.abi import MpcResult
    calls = scenario["calls"]
    path = tmp_path / "calls.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<q", len(calls)))
        for rec in calls:
            v, b = call_controls(rec)
            p = call_problem(rec)
            fh.write(struct.pack("<q", v.shape[1]))
            fh.write(struct.pack("<11d", *[getattr(p, f) for f, _ in p._fields_],
                                 rec["pre"]["optimal_criterion"]))
            fh.write(np.ascontiguousarray(v).tobytes())
            fh.write(np.ascontiguousarray(b).tobytes())
    rc, out, err = _run(drivers["san"], "calls", str(path))
    assert rc == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    raw = open(str(path) + ".out", "rb").read()
    n = len(raw) // ctypes_sizeof(MpcResult)
    assert n == len(calls) == 349
    for i, rec in enumerate(calls):
        res = MpcResult.from_buffer_copy(raw[i * ctypes_sizeof(MpcResult):])
        assert res.found == rec["found"], i
        assert (res.v, res.beta) == (rec["post"]["result_v"], rec["post"]["result_beta"]), i
        assert res.trajectory() == [s[:3] for s in rec["traj"]], i
    rc_p, out_p, _ = _run(drivers["plain"], "calls", str(path))
    assert rc_p == 0 and out_p == out


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)
