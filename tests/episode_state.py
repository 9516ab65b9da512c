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


class RobotState(ctypes.Structure):
    """One robot of the batched device episodes (csrc/mpc_episodes.h): the
    head and the stale trajectory as in EpisodeState, then what
    k_episodes_run carries across launches.  csrc/mpc_episodes.h parses in
    the host-only harness build (its kernels as ordinary device functions,
    without their launch bounds), so check_robot_layout() asserts the size
    and every offset against the compiler's; the library's own
    mpc_episodes_state_bytes is compared with the mirror as well
    (tests/test_robots_model_cpu.py)."""
    _fields_ = [("h", EpisodeHead), ("st", StaleTraj), ("stop", I32), ("calls", I32),
                ("candidates", I64)]


def check_robot_layout():
    """RobotState's size and offsets, sizeof(mpc_episode_config_t) and the
    configurations' offset for one robot: mirror == compiler."""
    import harness
    from diplomjourney_amd.abi import MpcEpisodeConfig
    mine = [ctypes.sizeof(RobotState)] + [getattr(RobotState, n).offset
                                          for n, _ in RobotState._fields_]
    mine += [ctypes.sizeof(MpcEpisodeConfig), robots_cfg_offset(1)]
    theirs = harness.robot_layout()
    assert mine == theirs, f"(mirror, compiler): {mine} {theirs}"
    assert RobotState.st.offset == ctypes.sizeof(EpisodeHead) == 8 * (
        STORED_WORDS - ctypes.sizeof(StaleTraj) // 8)
    return len(mine)


def robots_cfg_offset(n):
    """episodes_cfg_offset: where the n robots' configurations start."""
    return (n * ctypes.sizeof(RobotState) + 255) & ~255


def robots_state_bytes(n):
    """mpc_episodes_state_bytes(n) from the mirrors."""
    from diplomjourney_amd.abi import MpcEpisodeConfig
    return robots_cfg_offset(n) + n * ctypes.sizeof(MpcEpisodeConfig)


def read_robots(raw, n):
    """(RobotState[n], the n configurations' bytes) of a batch's state
    (bytes, or a uint8 tensor, device or host)."""
    from diplomjourney_amd.abi import MpcEpisodeConfig
    if not isinstance(raw, (bytes, bytearray)):
        raw = raw.detach().cpu().numpy().tobytes()
    assert len(raw) == robots_state_bytes(n)
    size = ctypes.sizeof(RobotState)
    robots = [RobotState.from_buffer_copy(raw[r * size:(r + 1) * size]) for r in range(n)]
    return robots, raw[robots_cfg_offset(n):robots_cfg_offset(n)
                       + n * ctypes.sizeof(MpcEpisodeConfig)]


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


def leaf_values(obj, prefix=""):
    """[(name, value)] of every scalar of a mirror, in leaves()' order, for a
    report: an element of an array is named by its own indices (st.ot[1][2];
    leaves() counts a 2-D array's elements flat) and a double is given as hex."""
    def walk(val, name):
        if isinstance(val, ctypes.Structure):
            return leaf_values(val, name + ".")
        if isinstance(val, ctypes.Array):
            return [q for i in range(len(val)) for q in walk(val[i], f"{name}[{i}]")]
        return [(name, val.hex() if isinstance(val, float) else val)]
    return [q for n, _ in obj._fields_ for q in walk(getattr(obj, n), prefix + n)]


def named_diff(got, want):
    """[(name, got's value, want's value)] of the scalars whose bits differ
    (diff()'s rule: padding excepted), each named by leaf_values()."""
    def bits(val, raw):    # (two NaNs print alike: their bits then)
        return f"{val} 0x{int.from_bytes(raw, 'little'):x}"
    rows = zip(leaves(got), leaves(want), leaf_values(got), leaf_values(want))
    return [(name, a, b) if a != b else (name, bits(a, ra), bits(b, rb))
            for (flat, ra), (_, rb), (name, a), (_, b) in rows
            if ra != rb and not flat.startswith(("pad0_", "pad1_", "pad2_"))]


def diff(got, want, skip=()):
    """Names of the scalars whose bits differ (padding excepted)."""
    bad = []
    for (name, a), (_, b) in zip(leaves(got), leaves(want)):
        if a != b and not name.startswith(("pad0_", "pad1_", "pad2_")) and name not in skip:
            bad.append(name)
    return bad
