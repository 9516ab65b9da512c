"""CU-masked launch streams (mpc_stream_create_cu_*): torch streams whose
kernels run on a subset of the device's CUs.  Each lives until the process
exits: an atexit hook synchronises the device and destroys it (before the HIP
runtime's own teardown, which otherwise finds a stream it did not create
still registered)."""
import atexit
import ctypes

import torch

from . import native

_CU_RESERVED = set()   # handles of the streams that leave CUs free (cu_reserved_stream)
_CREATED = []          # (handle, device) of every stream these helpers made


def _check_overlap_stream():
    """An overlapped exchange launch must leave CUs to the collective that runs
    beside it: a launch larger than one resident round (config C: 1954 blocks,
    1536 resident) fills every CU with blocks that wait, at the end of their
    tile, for block 0 — which waits for the collective.  Eager launches must
    therefore go to a cu_reserved_stream().  Eager only: a replayed hipGraph
    runs its parallel branches on runtime streams that carry no CU mask
    (measured: the 1M-candidate graph's launches filled every CU and block 0
    timed out, chain error 4)."""
    if torch.cuda.is_current_stream_capturing():
        raise ValueError("overlapped exchange: eager launches only (a replayed graph's branches "
                         "lose the launch stream's CU mask)")
    if torch.cuda.current_stream().cuda_stream in _CU_RESERVED:
        return
    raise ValueError("overlapped exchange: launch on a cu_reserved_stream() so the collective "
                     "beside each launch finds free CUs")


def _masked_stream(device, create, *args, reserved=False):
    """create(*args, &handle) on `device`; the handle registered for the atexit
    teardown and wrapped as a torch stream."""
    p = ctypes.c_void_p()
    with torch.cuda.device(device):
        create(*args, ctypes.byref(p))
    if reserved:
        _CU_RESERVED.add(p.value)
    if not _CREATED:
        atexit.register(_destroy_streams)
    _CREATED.append((p.value, torch.device(device)))
    return torch.cuda.ExternalStream(p.value, device=device)


def cu_reserved_stream(device, reserved_per_xcd=1):
    """A torch stream whose kernels (and hipGraphs replayed on it) leave
    `reserved_per_xcd` CUs of every XCD free (mpc_stream_create_cu_reserved):
    the launch stream of the overlapped exchange (DeviceEpisode(overlap=True)),
    so that the collective running beside a chained launch always finds CUs."""
    return _masked_stream(device, native.calls().mpc_stream_create_cu_reserved,
                          int(reserved_per_xcd), reserved=reserved_per_xcd > 0)


def cu_share_stream(device, part, parts):
    """A torch stream on the part-th of `parts` disjoint CU sets of the device
    (mpc_stream_create_cu_share): the launch stream of each of several ranks
    that rehearse a multi-GPU run on ONE GPU.  A chained exchange launch
    larger than one resident round fills every CU with tile blocks waiting for
    block 0, which waits for the peers — whose launches then find no CU.  On
    disjoint sets every rank keeps CUs for its block 0."""
    return _masked_stream(device, native.calls().mpc_stream_create_cu_share, int(part), int(parts))


def _destroy_streams():
    """atexit: drain and destroy the streams these helpers made."""
    lib = native.lib()
    while _CREATED:
        h, dev = _CREATED.pop()
        try:
            with torch.cuda.device(dev):
                torch.cuda.synchronize()
                torch.cuda.set_stream(torch.cuda.default_stream(dev))
            lib.mpc_stream_destroy(ctypes.c_void_p(h))   # status ignored: best effort at exit
        except Exception:   # the runtime is already gone: nothing left to release
            pass
        _CU_RESERVED.discard(h)
