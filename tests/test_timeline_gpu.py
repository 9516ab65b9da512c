"""GPU: the timeline variant (-DMPC_TIMELINE, csrc/mpc_timeline.h) at the
smallest shapes that reach every stamp.  One child process per case runs
tools/timeline.py's run mode against tools/tl_variant.so; this process runs
the product on the same inputs.  Asserted: the stamps change no result, every
slot of a block that ran is set, a block past the grid wrote nothing, and a
thread's entry stamp is not after its last one.  No order between different
threads' stamps and no duration is asserted."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "timeline.py")
_spec = importlib.util.spec_from_file_location("timeline_tool", TOOL)
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

N_CAND = 1026   # 512 + 512 + 2: the last tile block holds one lane pair


def _child(*args):
    """The tool's JSON result against the variant library, in a process of its own."""
    r = subprocess.run([sys.executable, TOOL, *map(str, args)], capture_output=True, text=True,
                       timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("JSON ")][-1]
    return json.loads(last[5:])


@pytest.mark.parametrize("n_steps", [2, 3])   # the mid-loop re-read needs a third step
@pytest.mark.parametrize("mode", ["soa", "tiled", "p2p"])
def test_chained_step_stamps(engine, mode, n_steps):
    """Four chained steps and the flush from reset()."""
    got = _child("chain", N_CAND, n_steps, mode, "--reps", 1, "--steps", 4)
    ep = T.chain_steps(N_CAND, n_steps, mode, 1, 4)
    want = T.digest(ep)
    ep.close()
    assert got["state"] == want and want["chain_error"] == 0
    nb, tiles, b0 = got["blocks"], got["tiles"], got["b0"]
    assert nb == 4
    for b in range(1, nb):
        slots = tiles[8 * b:8 * b + 8]
        assert all(slots[:len(T.TILE)]) and not any(slots[len(T.TILE):]), (b, slots)
        assert slots[T.TILE.index("entry")] <= slots[T.TILE.index("record stored")], (b, slots)
    assert tiles[0] and not any(tiles[1:8]), tiles[:8]
    unset = [q for q in got["b0_slots"] if not b0[q]]
    assert not unset, (unset, b0)
    assert not b0[0] and not any(b0[len(T.B0):]), b0   # (its entry is tiles[0]; no such phases)
    assert tiles[0] <= b0[8]                       # block 0: entry, published (thread 0)
    assert not any(tiles[8 * nb:8 * (nb + 2)])     # past the grid, after the table's reset


def test_persistent_run_stamps(engine):
    K = 3
    got = _child("run", N_CAND, 3, K, "--reps", 1)
    ep = T.run_steps(N_CAND, 3, K, "soa", 1)
    want = T.digest(ep)
    ep.close()
    assert got["state"] == want and want["chain_error"] == 0
    rest = [0, 0, 0, 2 ** 64 - 1, 0, 0, 0, 0]
    for j, row in enumerate(got["steps"]):
        if j >= K:
            assert row == rest, (j, row)
            continue
        assert all(row[:7]) and row[3] != rest[3], (j, row)    # (7: a count, may be zero)
        assert row[0] <= row[1] <= row[2], (j, row)            # the selector's thread 0


@pytest.mark.parametrize("integ", ["qk21", "rect+cum"])
def test_workload_r_stamps(engine, integ):
    """Three robots, robot 1 starting on its target (no call), at most 4 calls."""
    R, K = 3, 4
    got = _child("episodes", R, K, "--integ", integ, "--reps", 1, "--park", 1)
    eps = T.robots(R, K, integ, park=1)
    eps.run(K)
    want = T.digest(eps)
    assert got["state"] == want
    calls = want["calls"]
    assert calls[1] == 0 and calls[0] > 0 and calls[2] > 0
    for r, row in enumerate(got["robots"]):
        if r >= R or calls[r] == 0:
            assert not any(row), (r, row)        # past the grid / ran no call
            continue
        assert row[6] == calls[r] and row[7] == 0, (r, row)
        # per-phase sums of unsigned differences: set, and none wrapped below zero
        assert all(0 < x < 2 ** 62 for x in row[:6]), (r, row)
