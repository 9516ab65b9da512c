"""The fleet tests' comparison (tests/robots_bench.py: fleet_against,
assert_counts) without a GPU, with planted differences, as
test_robots_model_cpu.py checks robots_model.compare: the "device" is the
model's own bytes, which pass; with exactly one thing changed — a blocked
count, a neighbour, the last bit of a board entry, a state byte, the counts'
dtype — the comparison fails and names the launch and the thing."""
import ctypes

import numpy as np
import pytest

import episode_state as ES
import fleet_model as FM
import robots_bench as RB
from fleet_cases import RING_CLEARANCE, ring

LAUNCHES, CAP = (1, 2), 16


def _bytes_of(F, cfgs):
    """What a device that is the model would have left: fleet_device_run's result."""
    per, done = [], 0
    for k, counts in zip(LAUNCHES, FM.launch_counts(F, LAUNCHES)):
        done += k
        per.append(RB.FleetLaunch(counts, F.neighbours(done), F.board(done),
                                  F.motion(done) if F.predict else None))
    return FM.expected(F, cfgs, CAP, LAUNCHES), per


def _flipped(raw, at, bit=1):
    out = bytearray(raw)
    out[at] ^= bit
    return bytes(out)


def _entry(side, robot, n_robots, xy=0):
    """The byte offset of a board entry's lowest byte: [side][robot]{x, y}."""
    return ((side * n_robots + robot) * 2 + xy) * 8


@pytest.mark.parametrize("predict", (False, True))
def test_fleet_against_names_launch_and_thing(predict):
    cfgs = ring()
    F = RB.fleet_model(cfgs, 3, "rect+cum", RING_CLEARANCE, None, (), sum(LAUNCHES),
                       predict=predict, device=False)
    assert F.predict == predict
    got, per = _bytes_of(F, cfgs)
    assert (per[1].motion is not None) == predict
    RB.fleet_against(F, cfgs, CAP, LAUNCHES, got, per, "model")

    def fails(match, got=got, **launch):
        """One field of one launch replaced (launch: index=, then the field)."""
        i = launch.pop("index", None)
        planted = [p._replace(**launch) if j == i else p for j, p in enumerate(per)]
        with pytest.raises(AssertionError, match=match):
            RB.fleet_against(F, cfgs, CAP, LAUNCHES, got, planted, "planted")

    counts = per[1].blocked.copy()
    counts[4] += 1
    fails(r"planted launch 1: n_blocked of robots \[4\]", index=1, blocked=counts)
    fails("planted launch 0: n_blocked is int32", index=0, blocked=per[0].blocked.astype(np.int32))
    table = per[0].neighbours.copy()
    table[3, 1] += 1
    fails(r"planted launch 0: neighbours of robots \[3\]", index=0, neighbours=table)
    for side in (0, 1):
        board = _flipped(per[1].board, _entry(side, 5, 6, xy=1))
        fails(rf"planted launch 1: the pose board, \(side, robot\) \[\[{side}, 5\]\]",
              index=1, board=board)
        if predict:
            assert any(per[1].motion[_entry(side, 2, 6):_entry(side, 2, 6) + 8])
            motion = _flipped(per[1].motion, _entry(side, 2, 6))
            fails(rf"planted launch 1: the motion board, \(side, robot\) \[\[{side}, 2\]\]",
                  index=1, motion=motion)
    at = 2 * ctypes.sizeof(ES.RobotState) + ES.RobotState.calls.offset
    fails(r"planted: 1 differences:\nrobot 2 state after step 2 .*'calls', 2, 3",
          got=(_flipped(got[0], at), got[1], got[2]))


def test_assert_counts_names_launch_and_robots():
    want = [np.array([3, 0, 7], dtype=np.int64), np.array([1, 1, 0], dtype=np.int64)]
    RB.assert_counts("counts", [w.copy() for w in want], want)
    with pytest.raises(AssertionError, match="counts launch 1: n_blocked is int32"):
        RB.assert_counts("counts", [want[0], want[1].astype(np.int32)], want)
    off = want[0].copy()
    off[2] -= 1
    match = r"counts launch 0: n_blocked of robots \[2\]: device \[6\], model \[7\]"
    with pytest.raises(AssertionError, match=match):
        RB.assert_counts("counts", [off, want[1]], want)
    with pytest.raises(AssertionError):
        RB.assert_counts("counts", want[:1], want)
