"""ctypes mirrors of the device-resident episode's state (csrc/mpc_episode.h:
Consts, EpisodeHead, StaleTraj, EarlyPub, EpisodeState) for the tests that
write a state, launch, and read every field back.  The mirrors are written
out by hand, padding included; check_layout() asserts every size and offset
against the compiler's (replica_episode_layout, tests/replica_harness.cpp).
Test infrastructure only."""
import ctypes

D, I32, I64, U32, U64 = (ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32,
                         ctypes.c_uint64)

EP_MAX_GRID = 64      # kEpMaxGrid
PUB_WORDS = 40        # kPubWords: Consts' dwords, then t's two
STORED_WORDS = 47     # kStoredWords: head + stale trajectory, in 8-B words


class Consts(ctypes.Structure):
    _fields_ = [(n, D) for n in ("x", "y", "phi", "x_t", "y_t", "x_0", "y_0", "A", "B", "C1",
                                 "C2", "inv_den", "L", "inv_L", "h", "hlgth", "s0", "c0")] + [
        ("L_pow2", I32), ("pad_", I32)]


class EpisodeHead(ctypes.Structure):
    _fields_ = [("K", Consts), ("incumbent", D)] + [(n, D) for n in (
        "x", "y", "phi", "v", "beta", "x_t", "y_t", "x_0", "y_0", "t")] + [
        ("seed", U64), ("step", I64)] + [(n, I32) for n in (
            "p", "m", "steps_for_slowing", "episodes", "nv", "nb", "recursive", "has_traj")]


class StaleTraj(ctypes.Structure):
    _fields_ = [("ot", (D * 3) * 3), ("v", D), ("beta", D)]


class EarlyPub(ctypes.Structure):
    _fields_ = [("step", I64), ("k", I32), ("alt", I32)] + [(n, D) for n in (
        "t", "h", "hl", "x", "y", "ph")]


class EpisodeState(ctypes.Structure):
    _fields_ = [("h", EpisodeHead), ("st", StaleTraj), ("early", EarlyPub),
                ("grid_v", D * EP_MAX_GRID), ("grid_b", D * EP_MAX_GRID),
                ("done", U32), ("chain_error", U32), ("p2p_seq", U32),
                ("pad0_", ctypes.c_uint8 * 60),          # chain_pub: alignas(128)
                ("chain_pub", U64 * PUB_WORDS),
                ("pad1_", ctypes.c_uint8 * 64),          # gathered_tag: alignas(128)
                ("gathered_tag", U64),
                ("pad2_", ctypes.c_uint8 * 120)]         # sizeof: a multiple of 128


_STRUCTS = (("Consts", Consts), ("EpisodeHead", EpisodeHead), ("StaleTraj", StaleTraj),
            ("EarlyPub", EarlyPub), ("EpisodeState", EpisodeState))
_SIZE_ORDER = ("EpisodeHead", "StaleTraj", "EarlyPub", "EpisodeState", "Consts")


def named_fields(cls):
    return [n for n, _ in cls._fields_ if not (n.startswith("pad") and n.endswith("_")
                                               and cls is EpisodeState)]


def layout_names():
    """The order of replica_episode_layout's values."""
    names = [f"sizeof {n}" for n in _SIZE_ORDER]
    for sname, cls in _STRUCTS:
        names += [f"{sname}.{f}" for f in named_fields(cls)]
    return names + ["kEpMaxGrid", "kPubWords", "kStoredWords"]


def mirror_layout():
    """The same values from the ctypes mirrors."""
    by_name = dict(_STRUCTS)
    vals = [ctypes.sizeof(by_name[n]) for n in _SIZE_ORDER]
    for _, cls in _STRUCTS:
        vals += [getattr(cls, f).offset for f in named_fields(cls)]
    return vals + [EP_MAX_GRID, PUB_WORDS, STORED_WORDS]


def check_layout():
    """Every size and offset of the mirrors equals the compiler's; returns the
    number of values compared."""
    import harness
    names, mine = layout_names(), mirror_layout()
    theirs, count = harness.episode_layout(len(names))
    assert count == len(names), f"the harness reports {count} layout values, not {len(names)}"
    bad = [(n, a, b) for n, a, b in zip(names, mine, theirs) if a != b]
    assert not bad, f"(name, mirror, compiler): {bad}"
    return len(names)


def state_bytes():
    return ctypes.sizeof(EpisodeState)


def read_state(tensor, index=0):
    """EpisodeState number `index` of a uint8 tensor of states (device or host)."""
    n = ctypes.sizeof(EpisodeState)
    raw = tensor.detach().cpu().numpy().tobytes()[index * n:(index + 1) * n]
    return EpisodeState.from_buffer_copy(raw)


def write_state(tensor, state, index=0):
    """Store `state` as EpisodeState number `index` of the uint8 tensor."""
    import numpy as np
    import torch
    n = ctypes.sizeof(EpisodeState)
    src = torch.from_numpy(np.frombuffer(bytes(state), dtype=np.uint8).copy())
    tensor[index * n:(index + 1) * n].copy_(src)


def leaves(obj, prefix="", raw=None, base=0):
    """[(dotted name, raw bytes)] of every scalar of a mirror, arrays element
    by element: what a bitwise comparison names when it fails."""
    raw = bytes(obj) if raw is None else raw
    out = []
    for name, _ in obj._fields_:
        val = getattr(obj, name)
        field = getattr(type(obj), name)
        lo = base + field.offset
        if isinstance(val, ctypes.Structure):
            out += leaves(val, f"{prefix}{name}.", raw, lo)
        elif isinstance(val, ctypes.Array):
            n = _flat_len(val)
            step = field.size // n
            out += [(f"{prefix}{name}[{i}]", raw[lo + i * step:lo + (i + 1) * step])
                    for i in range(n)]
        else:
            out.append((prefix + name, raw[lo:lo + field.size]))
    return out


def _flat_len(arr):
    n = len(arr)
    return n * _flat_len(arr[0]) if isinstance(arr[0], ctypes.Array) else n


def diff(got, want, skip=()):
    """Names of the scalars whose bits differ (padding excepted)."""
    bad = []
    for (name, a), (_, b) in zip(leaves(got), leaves(want)):
        if a != b and not name.startswith(("pad0_", "pad1_", "pad2_")) and name not in skip:
            bad.append(name)
    return bad
