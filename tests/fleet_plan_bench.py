"""The bench of the planned fleet call (mpc_episodes_fleet_run_planned through
DeviceFleet(predict="plan")): robots_bench's fleet bench with the plan board —
the device run that poisons the board before the first run() and takes its
bytes after every launch, the model with its margins asserted, and the
comparison of both.  What tests/test_fleet_plan_cpu.py and
tests/test_fleet_plan_gpu.py share.  Test infrastructure only."""
from collections import namedtuple

import numpy as np

import fleet_model as FM
import fleet_plan_model as PM
import robots_bench as RB
from ranking import MARGIN

# robots_bench.FleetLaunch and the plan board's bytes (motion: None, a planned
# fleet has no motion board)
PlanLaunch = namedtuple("PlanLaunch", "blocked neighbours board motion plan")


def device_run(engine, cfgs, n_steps, integ, clearance, reach, static, launches, cap,
               predict="plan"):
    """DeviceFleet(predict=) over `launches` -> the final (state, log, progress)
    bytes and a record per launch; predict=True / False: robots_bench's run."""
    if predict != "plan":
        return RB.fleet_device_run(engine, cfgs, n_steps, integ, clearance, reach, static,
                                   launches, cap, predict)
    from diplomjourney_amd.device_episodes import DeviceFleet
    eps = DeviceFleet(engine, cfgs, clearance, n_steps, integ, log_capacity=cap, obstacles=static,
                      reach=reach, predict="plan")
    assert eps.motion is None
    eps.n_blocked.fill_(77)          # (zeroed by the entry, then added to)
    eps.neighbours.fill_(55)         # (every row written by the last launch)
    eps.plan.fill_(0x5A)             # (side 0 filled by the entry before call 0, side 1 written)
    per = RB.run_launches(eps, launches, lambda e: PlanLaunch(
        e.read_blocked(), e.neighbours.cpu().numpy().copy(), e.board.cpu().numpy().tobytes(),
        None, e.plan.cpu().numpy().tobytes()))
    got = RB.snapshot(eps)
    assert eps.call0 == sum(launches)
    return got, per


def model(cfgs, n_steps, integ, clearance, reach, static, n_calls, ties=False, device=True):
    """The planned fleet's model over n_calls, its margins asserted: any state
    against any planned rim, the reach and the cap (ties: the case is about
    exact ties there)."""
    from diplomjourney_amd.device_episodes import fleet_reach
    reach = fleet_reach(cfgs, n_steps, clearance, predict=True) if reach is None else reach
    F = PM.PlanFleet(cfgs, n_steps, integ, clearance, reach, static).run(n_calls, device=device)
    assert F.margin() > MARGIN, F.margin()
    if not ties:
        assert F.edge > MARGIN and F.gap > FM.CAP_GAP, (F.edge, F.gap)
    return F


def _plan_rows(device, want):
    """The (side, robot) entries in which two plan boards' bytes differ."""
    dev = np.frombuffer(device, dtype=np.float64).reshape(2, -1, 4)
    mod = np.frombuffer(want, dtype=np.float64).reshape(2, -1, 4)
    rows = np.argwhere((dev.view(np.uint64) != mod.view(np.uint64)).any(axis=2))[:4]
    return (f"the plan board, (side, robot) {rows.tolist()}: "
            f"device {[dev[s, r].tolist() for s, r in rows]}, "
            f"model {[mod[s, r].tolist() for s, r in rows]}")


def against(F, cfgs, cap, launches, got, per, name):
    """robots_bench.fleet_against, and the plan board after every launch."""
    RB.fleet_against(F, cfgs, cap, launches, got, per, name)
    done = 0
    for i, p in enumerate(per):
        done += launches[i]
        assert len(p.plan) == 2 * len(cfgs) * 32
        assert p.plan == F.plan(done), f"{name} launch {i}: " + _plan_rows(p.plan, F.plan(done))


def check(engine, cfgs, n_steps, integ, clearance, launches, reach=None, static=(), cap=16,
          precondition=None, ties=False, name="planned fleet"):
    """The model, its margins and the case's precondition; then the device
    against it -> (the model, the device's bytes, its per-launch records)."""
    F = model(cfgs, n_steps, integ, clearance, reach, static, sum(launches), ties)
    if precondition:
        precondition(F)
    got, per = device_run(engine, cfgs, n_steps, integ, clearance, reach, static, launches, cap)
    against(F, cfgs, cap, launches, got, per, name)
    return F, got, per
