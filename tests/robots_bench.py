"""The bench of the batched robots' kernel (k_episodes_run behind its four
entries: plain, circles, fleet, predicted fleet): run a DeviceEpisodes or a
DeviceFleet over a case's launches, take its bytes, and compare them with a
host model's — what tests/test_robots_replica_gpu.py,
tests/test_robots_obstacles_gpu.py, tests/test_fleet_gpu.py and
tests/test_fleet_predict_gpu.py share.  Everything that keeps such a test from
passing vacuously is here, once: the poison in every buffer an entry must
write, the state tensor's size, the count of fleet calls, and the model's
margins asserted before any kernel is looked at.  The comparisons take bytes,
so tests/test_robots_bench_cpu.py checks them without a GPU, with planted
differences.  Test infrastructure only."""
from collections import namedtuple

import numpy as np

import episode_state as ES
import fleet_model as FM
import robots_model as RM
from ranking import MARGIN

# what a fleet's test reads after every run(): read_blocked(), the neighbour
# table, the pose board's bytes and (predicted, else None) the motion board's
FleetLaunch = namedtuple("FleetLaunch", "blocked neighbours board motion")


def snapshot(eps):
    """The (state, log, progress) bytes of a batch, everything enqueued done."""
    import torch
    torch.cuda.synchronize()
    return (eps.state.cpu().numpy().tobytes(), eps.log.cpu().numpy().tobytes(),
            eps.progress.cpu().numpy().tobytes())


def run_launches(eps, launches, after=lambda eps: None):
    """eps.run(k) for every k of `launches` -> what after(eps) returns after each."""
    assert ES.robots_state_bytes(eps.R) == eps.state.numel()
    out = []
    for k in launches:
        eps.run(k)
        out.append(after(eps))
    return out


def assert_model(case, got, models, recs):
    """robots_model.compare of the (state, log, progress) bytes `got`."""
    bad = RM.compare(case, *got, models, recs)
    assert not bad, f"{case['name']}: {len(bad)} differences:\n" + "\n".join(bad[:8])


def assert_counts(name, blocked_per_launch, want):
    """read_blocked() after every launch against the model's counts
    (robots_obstacle_model.launch_counts)."""
    assert len(blocked_per_launch) == len(want)
    for i, (g, w) in enumerate(zip(blocked_per_launch, want)):
        assert g.dtype == np.int64, f"{name} launch {i}: n_blocked is {g.dtype}"
        assert (g == w).all(), (
            f"{name} launch {i}: n_blocked of robots "
            f"{np.flatnonzero(g != w)[:8]}: device {g[g != w][:8]}, model {w[g != w][:8]}")


def episodes_run(engine, case, circles=None, cls=None):
    """DeviceEpisodes (or `cls`) over the case's launches -> (the (state, log,
    progress) bytes, per launch None, the batch); with `circles` (a list, ()
    too): made with obstacles=circles, n_blocked poisoned first, and
    read_blocked() per launch."""
    from diplomjourney_amd.device_episodes import DeviceEpisodes
    kw = {} if circles is None else dict(obstacles=circles)
    eps = (cls or DeviceEpisodes)(engine, case["cfgs"], case["n_steps"], case["integ"],
                                  log_capacity=case["cap"], **kw)
    if circles is None:
        blocked = run_launches(eps, case["launches"])
    else:
        eps.n_blocked.fill_(77)      # (written, not accumulated)
        blocked = run_launches(eps, case["launches"], lambda e: e.read_blocked())
    return snapshot(eps), blocked, eps


# ----------------------------------------------------------------------------
# the fleet
# ----------------------------------------------------------------------------
def fleet_device_run(engine, cfgs, n_steps, integ, clearance, reach, static, launches, cap,
                     predict=False):
    """DeviceFleet over `launches` -> the final (state, log, progress) bytes and
    a FleetLaunch per launch."""
    from diplomjourney_amd.device_episodes import DeviceFleet
    eps = DeviceFleet(engine, cfgs, clearance, n_steps, integ, log_capacity=cap, obstacles=static,
                      reach=reach, predict=predict)
    eps.n_blocked.fill_(77)          # (zeroed by the entry, then added to)
    eps.neighbours.fill_(55)         # (every row written by the last launch)
    if predict:
        eps.motion.fill_(0x5A)       # (side 0 zeroed by the entry before call 0, side 1 written)
    per = run_launches(eps, launches, lambda e: FleetLaunch(
        e.read_blocked(), e.neighbours.cpu().numpy().copy(), e.board.cpu().numpy().tobytes(),
        e.motion.cpu().numpy().tobytes() if predict else None))
    got = snapshot(eps)
    assert eps.call0 == sum(launches)
    return got, per


def fleet_model(cfgs, n_steps, integ, clearance, reach, static, n_calls, predict=False,
                ties=False, device=True):
    """The fleet's model over n_calls, its margins asserted (ties: the case is
    about exact ties at the reach and at the cap, so those two are not)."""
    from diplomjourney_amd.device_episodes import fleet_reach
    reach = fleet_reach(cfgs, n_steps, clearance, predict=predict) if reach is None else reach
    F = FM.Fleet(cfgs, n_steps, integ, clearance, reach, static, predict=predict).run(
        n_calls, device=device)
    assert F.margin() > MARGIN, F.margin()
    if not ties:
        assert F.edge > MARGIN and F.gap > FM.CAP_GAP, (F.edge, F.gap)
    return F


def _board_rows(name, device, model):
    """The (side, robot) entries in which two boards' bytes differ, with both values."""
    dev = np.frombuffer(device, dtype=np.float64).reshape(2, -1, 2)
    want = np.frombuffer(model, dtype=np.float64).reshape(2, -1, 2)
    rows = np.argwhere((dev.view(np.uint64) != want.view(np.uint64)).any(axis=2))[:4]
    return (f"the {name} board, (side, robot) {rows.tolist()}: "
            f"device {[dev[s, r].tolist() for s, r in rows]}, "
            f"model {[want[s, r].tolist() for s, r in rows]}")


def fleet_against(F, cfgs, cap, launches, got, per, name):
    """The device's bytes against the model's: the batch after the last launch
    and, after every launch, the counts, the neighbour table, the pose board
    and — a predicted fleet's — the motion board."""
    assert_model(dict(cfgs=cfgs, cap=cap, launches=launches, name=name), got, F.models, F.recs)
    assert_counts(name, [p.blocked for p in per], FM.launch_counts(F, launches))
    done = 0
    for i, p in enumerate(per):
        done += launches[i]
        want = F.neighbours(done)
        rows = np.flatnonzero((p.neighbours != want).any(axis=1))[:4]
        assert not len(rows), (f"{name} launch {i}: neighbours of robots {rows}: device "
                               f"{p.neighbours[rows]}, model {want[rows]}")
        assert p.board == F.board(done), (
            f"{name} launch {i}: " + _board_rows("pose", p.board, F.board(done)))
        if F.predict:
            assert p.motion == F.motion(done), (
                f"{name} launch {i}: " + _board_rows("motion", p.motion, F.motion(done)))


def fleet_check(engine, cfgs, n_steps, integ, clearance, launches, reach=None, static=(), cap=16,
                precondition=None, ties=False, name="fleet", predict=False):
    """The model, its margins and the case's precondition; then the device
    against it -> (the model, the device's bytes, its FleetLaunch records)."""
    F = fleet_model(cfgs, n_steps, integ, clearance, reach, static, sum(launches), predict, ties)
    if precondition:
        precondition(F)
    got, per = fleet_device_run(engine, cfgs, n_steps, integ, clearance, reach, static, launches,
                                cap, predict)
    fleet_against(F, cfgs, cap, launches, got, per, name)
    return F, got, per
