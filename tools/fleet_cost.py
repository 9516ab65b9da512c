"""What a fleet call costs beside the launch it grew from (built
after tools/robots_obstacle_cost.py).

Per fleet call: ONE launch of mpc_episodes_fleet_run (n_calls = 1) against ONE
launch of mpc_episodes_run_obstacles (max_calls = 1) that carries THE SAME
NUMBER OF CIRCLES PER ROBOT, at workload R's robot count (bench.py) and at 64
robots, with 0, 1, 4 and 13 neighbours per robot.  The robots stand in clusters
of k + 1, 0.05 apart, the clusters 10 apart: every robot has exactly k others
within reach.  The clearance is 1e-6 and the baseline's k circles lie where no
robot goes, so no row blocks a candidate and every row's robots take the same
first step.  What differs is the board scan, the selection and the table as
LDS operands instead of kernel arguments.

One object per variant; the variants alternate launch by launch in one
process; each timed launch follows an untimed reset (fleet: with
mpc_episodes_fleet_begin) and ~60 us of filler work on the device, so that the
host is ahead of the device, and sits between two device events.  The rows pass
neither n_blocked_out nor neighbours_out; fleet_4_counted passes both.  plain_a
/ plain_b: the plain entry twice, the run's own spread.  The 0-neighbour row
has nothing but the scan over the plain launch: it must lie inside the plain
quartile band shifted up by the scan time.  The scan time is measured apart
from the launch times: tools/timeline.py fleet N 0 (the MPC_TIMELINE variant,
a process of its own) stamps the selection per block, and a launch pays it
once per round of blocks (two blocks per CU at a time).  512 robots are
measured as well.

The predicted column (mpc_episodes_fleet_run_predicted): predicted_K is one
predicted fleet call for fleet_K's robots, alternated with it in the same
process, so predicted_K - fleet_K is what the prediction adds — the motion
loads, the per-step tables' formation and the motion write.  It is launched as
fleet call 2 (an even call on a motion board of zeros), so that the row holds
the launch alone; predicted_4_call0 is fleet call 0, with the entry's
hipMemsetAsync of the motion board's side 0 inside the event pair.  The
formation's time per block comes from the stamps as the selection's does
(tools/timeline.py fleet: formation_ns).

The planned column (mpc_episodes_fleet_run_planned): planned_K is one planned
fleet call for the same robots, alternated with fleet_K and predicted_K in the
same process; planned_K - predicted_K is what the plan board costs over the
motion board — a 32-B entry per neighbour instead of 16 B, staged in LDS, and
a 32-B write.  It is made as the predicted column is: fleet call 2 on a board
of standing plans (both sides every robot's position twice, so the work is the
fleet call's); planned_4_call0 is fleet call 0, with the entry's fill of the
plan board's side 0 inside the event pair.  plan_formation_ns comes from the
stamps as formation_ns does.

    python tools/fleet_cost.py [--launches 40] [--out profiles/fleet/cost.json]
Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools import cost_timing  # noqa: E402

NEIGHBOURS = (0, 1, 4, 13)
CLEARANCE = 1e-6
REACH = 1.0


def fleet_configs(n, k):
    """n robots in clusters of k + 1 (the last cluster may be smaller: its
    robots have fewer neighbours; the rows report the minimum and maximum),
    all headed the same way at far targets."""
    from diplomjourney_amd.episode_config import tree_episode_config
    cfgs = []
    for r in range(n):
        c, j = divmod(r, k + 1)
        x, y = 10.0 * (c % 32), 10.0 * (c // 32) + 0.05 * j
        cfgs.append(tree_episode_config((x, y, 0.3, x + 300.0, y + 100.0), 1))
    return cfgs


def classes():
    from diplomjourney_amd import native
    from diplomjourney_amd.device_episodes import DeviceEpisodes, DeviceFleet

    class Baseline(DeviceEpisodes):
        """mpc_episodes_run_obstacles, with no circles too, no count."""
        obstacle_entry = False

        def _obstacle_args(self):
            if not (self._n_obs or self.obstacle_entry):
                return None
            return self._obs, self._n_obs, None

    class Fleet(DeviceFleet):
        counted = False

        def run(self, n_calls):
            self._C.mpc_episodes_fleet_run(
                self.state.data_ptr(), self.board.data_ptr(), self.call0, self._obs, self._n_obs,
                self.clearance, self.reach, self.R, self.n_steps, self._integ, int(n_calls),
                self.log.data_ptr(), self.log_capacity, self.progress.data_ptr(),
                self.n_blocked.data_ptr() if self.counted else None,
                self.neighbours.data_ptr() if self.counted else None, native.current_stream())
            self.call0 += int(n_calls)

    class Predicted(Fleet):
        call = 2        # the fleet call each launch is made as (0: the entry zeroes side 0 first)

        def run(self, n_calls):
            self._C.mpc_episodes_fleet_run_predicted(
                self.state.data_ptr(), self.board.data_ptr(), self.motion.data_ptr(), self.call,
                self._obs, self._n_obs, self.clearance, self.reach, self.R, self.n_steps,
                self._integ, int(n_calls), self.log.data_ptr(), self.log_capacity,
                self.progress.data_ptr(), self.n_blocked.data_ptr() if self.counted else None,
                self.neighbours.data_ptr() if self.counted else None, native.current_stream())
            self.call0 += int(n_calls)

    class Planned(Fleet):
        call = 2        # (0: the entry fills the plan board's side 0 first)

        def reset(self):
            """... and a plan board on which everybody stands: both sides every
            robot's (x, y, x, y), from the pose board's side 0 (untimed)."""
            super().reset()
            import torch
            pos = self.board.view(torch.float64)[:2 * self.R].view(self.R, 2)
            side = torch.cat([pos, pos], dim=1).reshape(-1)
            self.plan.view(torch.float64).copy_(torch.cat([side, side]))

        def run(self, n_calls):
            self._C.mpc_episodes_fleet_run_planned(
                self.state.data_ptr(), self.board.data_ptr(), self.plan.data_ptr(), self.call,
                self._obs, self._n_obs, self.clearance, self.reach, self.R, self.n_steps,
                self._integ, int(n_calls), self.log.data_ptr(), self.log_capacity,
                self.progress.data_ptr(), self.n_blocked.data_ptr() if self.counted else None,
                self.neighbours.data_ptr() if self.counted else None, native.current_stream())
            self.call0 += int(n_calls)

    return Baseline, Fleet, Predicted, Planned


def measure(eng, integ, n, launches, warmup):
    import torch
    Baseline, Fleet, Predicted, Planned = classes()

    def planned(k):
        return Planned(eng, fleet_configs(n, k), CLEARANCE, 3, integ, log_capacity=1, reach=REACH,
                       predict="plan")
    far = lambda k: cost_timing.circles(k, lambda i: (-100.0 - 0.1 * i, -100.0))
    objs, variants = {}, [("plain_a", None)]
    objs["plain_a"] = Baseline(eng, fleet_configs(n, 0), 3, integ, log_capacity=1)
    for k in NEIGHBOURS:
        cfgs = fleet_configs(n, k)
        objs[f"obstacles_{k}"] = Baseline(eng, cfgs, 3, integ, log_capacity=1, obstacles=far(k))
        objs[f"obstacles_{k}"].obstacle_entry = True
        objs[f"fleet_{k}"] = Fleet(eng, cfgs, CLEARANCE, 3, integ, log_capacity=1, reach=REACH)
        objs[f"predicted_{k}"] = Predicted(eng, cfgs, CLEARANCE, 3, integ, log_capacity=1,
                                           reach=REACH, predict=True)
        objs[f"planned_{k}"] = planned(k)
        variants += [(f"obstacles_{k}", k), (f"fleet_{k}", k), (f"predicted_{k}", k),
                     (f"planned_{k}", k)]
    objs["fleet_4_counted"] = Fleet(eng, fleet_configs(n, 4), CLEARANCE, 3, integ, log_capacity=1,
                                    reach=REACH)
    objs["fleet_4_counted"].counted = True
    objs["predicted_4_call0"] = Predicted(eng, fleet_configs(n, 4), CLEARANCE, 3, integ,
                                          log_capacity=1, reach=REACH, predict=True)
    objs["predicted_4_call0"].call = 0
    objs["planned_4_call0"] = planned(4)
    objs["planned_4_call0"].call = 0
    objs["plain_b"] = Baseline(eng, fleet_configs(n, 0), 3, integ, log_capacity=1)
    variants += [("fleet_4_counted", 4), ("predicted_4_call0", 4), ("planned_4_call0", 4),
                 ("plain_b", None)]
    variants = tuple(variants)

    # ~60 us of device work ahead of every timed launch: the host has enqueued the
    # launch and both events long before the device reaches them, so an event
    # pair holds device time only (without it the device waits for the host's
    # call, and a variant whose Python call is longer looks slower by that)
    filler = torch.zeros(32 << 20, dtype=torch.float32, device=eng.device)

    def launch(name, _k, _batch, ev):
        ep = objs[name]
        ep.reset()
        filler.add_(1.0)
        if ev:
            ev[0].record()
        ep.run(1)
        if ev:
            ev[1].record()

    events = cost_timing.alternate(variants, warmup, launches, launch)
    torch.cuda.synchronize()
    rows = {}
    for name, evs in events.items():
        calls, stop, cands = objs[name].read_progress()
        rows[name] = {**cost_timing.summary(evs, "launches"), "calls": int(calls.sum()),
                      "candidates": int(cands.sum())}
    for k in NEIGHBOURS:      # the neighbours the kernel found: exactly k per robot of a full cluster
        objs[f"fleet_{k}"].counted = True
        objs[f"fleet_{k}"].reset()
        objs[f"fleet_{k}"].run(1)
        within = [w for w, _ in objs[f"fleet_{k}"].read_neighbours()]
        rows[f"fleet_{k}"]["neighbours_min_max"] = [min(within), max(within)]
    same = len({(r["calls"], r["candidates"]) for r in rows.values()}) == 1
    a, b = rows["plain_a"], rows["plain_b"]
    base = 0.5 * (a["median_us"] + b["median_us"])
    for k in NEIGHBOURS:
        f, o = rows[f"fleet_{k}"], rows[f"obstacles_{k}"]
        f["over_same_circles_us"] = f["median_us"] - o["median_us"]
        f["share_of_call"] = f["over_same_circles_us"] / f["median_us"]
        p = rows[f"predicted_{k}"]
        p["over_fleet_us"] = p["median_us"] - f["median_us"]
        p["over_fleet_share"] = p["over_fleet_us"] / f["median_us"]
        p["fleet_quartile_band_us"] = [f["p25_us"], f["p75_us"]]
        q = rows[f"planned_{k}"]
        q["over_fleet_us"] = q["median_us"] - f["median_us"]
        q["over_fleet_share"] = q["over_fleet_us"] / f["median_us"]
        q["over_predicted_us"] = q["median_us"] - p["median_us"]
        q["predicted_quartile_band_us"] = [p["p25_us"], p["p75_us"]]
        q["slower_than_predicted_by_more_than_its_spread"] = (
            q["over_predicted_us"] > p["p75_us"] - p["p25_us"])
    return {"integrator": integ, "robots": n, "n_steps": 3, "rows": rows,
            "same_step_in_every_row": same, "plain_median_us": base,
            "plain_quartile_band_us": [min(a["p25_us"], b["p25_us"]),
                                       max(a["p75_us"], b["p75_us"])],
            "fleet_0_over_plain_us": rows["fleet_0"]["median_us"] - base}


def stamped_ns(n, integ, k=0):
    """The selection's time per block and the per-step tables' formation
    (predicted, planned), from the stamps: tools/timeline.py fleet N K in a
    process of its own (it loads the variant library), its JSON line's
    selection_ns, formation_ns and plan_formation_ns."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "timeline.py"), "fleet",
                          str(n), str(k), "--integ", integ], capture_output=True, text=True,
                         check=True).stdout
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("JSON ")][-1][5:])
    return (float(line["selection_ns"]), float(line["formation_ns"]),
            float(line["plan_formation_ns"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--robots", type=int, default=1000, help="workload R's robot count")
    ap.add_argument("--mid", type=int, default=512, help="a size between the two")
    ap.add_argument("--launches", type=int, default=40, help="timed launches per variant")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches per variant")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fleet", "cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fleet_cost.py needs a GPU")
    from diplomjourney_amd.expansion import Expansion
    eng = Expansion("cuda:0")
    sizes = []
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for integ in ("qk21", "rect+cum"):
        for n in (args.robots, args.mid, 64):
            m = measure(eng, integ, n, args.launches, args.warmup)
            # the scan, measured where it runs: the selection's time per block from
            # the stamps (tools/timeline.py fleet, the variant library, a process of
            # its own), once per round of blocks (two blocks per CU at a time)
            (m["selection_ns_per_block"], m["formation_0_ns_per_block"],
             m["plan_formation_0_ns_per_block"]) = stamped_ns(n, integ)
            _, m["formation_13_ns_per_block"], m["plan_formation_13_ns_per_block"] = stamped_ns(
                n, integ, 13)
            m["rounds_of_blocks"] = -(-n // (2 * cus))
            m["scan_us"] = m["selection_ns_per_block"] * m["rounds_of_blocks"] / 1e3
            m["formation_0_us"] = m["formation_0_ns_per_block"] * m["rounds_of_blocks"] / 1e3
            f0, p0 = m["rows"]["fleet_0"], m["rows"]["predicted_0"]
            m["predicted_0_inside_fleet_band_plus_formation"] = (
                p0["median_us"] <= f0["p75_us"] + max(m["formation_0_us"], 0.0))
            lo, hi = m["plain_quartile_band_us"]
            z = m["rows"]["fleet_0"]["median_us"]
            m["zero_inside_band_plus_scan"] = lo + m["scan_us"] <= z <= hi + m["scan_us"]
            sizes.append(m)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "one device-event pair per launch (one fleet call / one max_calls = 1 "
                        "launch after an untimed reset), variants alternated launch by launch",
              "sizes": sizes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for m in sizes:
        print(m["integrator"], m["robots"], "robots: plain band", m["plain_quartile_band_us"],
              "scan", m["scan_us"], "fleet_0 - plain", m["fleet_0_over_plain_us"],
              "zero inside band + scan", m["zero_inside_band_plus_scan"], "same step",
              m["same_step_in_every_row"], "formation per block (0 / 13 neighbours, ns)",
              m["formation_0_ns_per_block"], m["formation_13_ns_per_block"],
              "planned", m["plan_formation_0_ns_per_block"], m["plan_formation_13_ns_per_block"],
              "predicted_0 inside the fleet band + formation",
              m["predicted_0_inside_fleet_band_plus_formation"])
        for name, r in m["rows"].items():
            extra = (f"  over same circles {r['over_same_circles_us']:7.2f} us "
                     f"({100 * r['share_of_call']:.1f} % of the call)  neighbours "
                     f"{r['neighbours_min_max']}" if "share_of_call" in r else
                     f"  over the fleet call {r['over_fleet_us']:7.2f} us "
                     f"({100 * r['over_fleet_share']:.1f} %)"
                     + (f"  over the predicted call {r['over_predicted_us']:7.2f} us"
                        if "over_predicted_us" in r else "") if "over_fleet_us" in r else "")
            print(f"  {name:16s} median {r['median_us']:8.2f} us  p25 {r['p25_us']:8.2f}  "
                  f"p75 {r['p75_us']:8.2f}{extra}")


if __name__ == "__main__":
    main()
