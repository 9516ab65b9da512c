"""The C-ABI calls the Python host makes for every DeviceEpisode step form.

    python tools/call_trace.py [OUT]

Wraps the library handles of diplomjourney_amd.native so that every mpc_*
call is written down as `entry(arguments)`, then drives each step form for
five steps and a read_log() on one GPU.  Pointers (the stream included) are
replaced by the ordinal of their first appearance within the form, scalars
(epochs included) are recorded literally; so two revisions of the host code
that issue the same calls print the same text, whatever the allocator hands
out.  Only public constructor arguments are used: the file runs unchanged on
any revision that has these forms (profiles/py_host/ compares two).
"""
import ctypes
import os
import socket
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diplomjourney_amd import math_model_tree as mmt  # noqa: E402
from diplomjourney_amd import native  # noqa: E402

LINES = []
_IDS = {}


def _ptr(addr):
    if not addr:
        return "null"
    return "p%d" % _IDS.setdefault(int(addr), len(_IDS))


def _is_pointer(ct):
    return ct in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ct, ctypes._Pointer)


def _arg(a, ct):
    if not _is_pointer(ct):
        return repr(float(a)) if ct is ctypes.c_double else str(int(a))
    if a is None:
        return "null"
    if isinstance(a, int):
        return _ptr(a)
    if isinstance(a, ctypes.c_void_p):
        return _ptr(a.value)
    if isinstance(a, ctypes.Array):          # host arrays live only for the call
        if a._type_ is ctypes.c_void_p:
            return "[" + " ".join(_ptr(x) for x in a) + "]"
        return "&bytes[%d]" % len(a)
    obj = a._obj                             # ctypes.byref(...)
    if isinstance(obj, ctypes.Structure):    # a config: lives as long as the episode
        return _ptr(ctypes.addressof(obj))
    return "&out"


class Traced:
    """A library handle whose mpc_* entries write their call down first."""

    def __init__(self, handle):
        self._handle = handle

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("mpc_"):
            return fn

        def call(*args):
            assert len(args) == len(fn.argtypes), name
            LINES.append("%s(%s)" % (name, ", ".join(_arg(a, t) for a, t in zip(args, fn.argtypes))))
            return fn(*args)
        return call


def section(title):
    _IDS.clear()
    LINES.append("## " + title)


def main(out):
    raw = Traced(native.lib())
    if hasattr(native, "calls"):             # a revision with the raising handle: trace both
        checked = Traced(native.calls())
        native.calls = lambda: checked
    native.lib = lambda: raw
    from diplomjourney_amd.episode import DeviceEpisode, cu_reserved_stream
    from diplomjourney_amd.expansion import Expansion

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    eng = Expansion("cuda")
    ns, steps = 3, 5
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    reserved = cu_reserved_stream(torch.device("cuda", 0))

    def drive(title, n, controls=None, runs=1, use_run=False, stream=None, **kw):
        section("%s, n_cand_total=%d" % (title, n))
        pool = [None] * steps
        if controls == "soa":
            pool = [eng.sample_controls(V, B, n, ns, 700 + i) for i in range(steps)]
        elif controls == "tiled":
            pool = [eng.sample_controls_tiled(V, B, n, ns, 700 + i) for i in range(steps)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            ep = DeviceEpisode(eng, n, ns, log_capacity=16, **kw)
            for r in range(runs):
                if r:
                    ep.reset()
                if use_run:
                    ep.run(pool)
                else:
                    for c in pool:
                        ep.step(controls=c)
                log = ep.read_log()
                LINES.append("# read_log: %s" % [(x.step, x.index, repr(x.cost)) for x in log])
            LINES.append("# p2p=%s p2p_status=%s" % (ep.p2p, ep.p2p_status))
            ep.close()
        torch.cuda.synchronize()

    cum = dict(integrator="rect+cum")
    drive("1 plain split", 1536)
    drive("2 split=False", 1536, split=False)
    drive("3 generate=True", 1536, generate=True)
    for n in (1536, 1030):
        drive("4 chain=True, SoA controls", n, "soa", chain=True, **cum)
        drive("5 chain=True, tiled controls", n, "tiled", chain=True, **cum)
        drive("6 run() over five batches", n, "soa", use_run=True, chain=True, **cum)
    drive("7 exchange=True on one rank", 1536, exchange=True)
    for n in (1536, 1030):
        drive("8 exchange=True, chain=True", n, "soa", exchange=True, chain=True, **cum)
        drive("9 exchange=True, chain=True, overlap=True on a cu_reserved_stream", n, "soa",
              stream=reserved, exchange=True, chain=True, overlap=True, **cum)
        drive("10 p2p=True, chain=True, world=1, reset() between two runs", n, "soa", runs=2,
              exchange=True, chain=True, p2p=True, **cum)
    dist.destroy_process_group()
    text = "\n".join(LINES) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
