"""What keep-out circles cost the batched robots' device-resident episodes
(built after tools/episode_obstacle_cost.py).

Workload R's shape (bench.py): run_math_model.py's 1000 seeded episodes over
the tree expansion, N = 3, one block per robot, every episode run to its end
in ONE launch.  Per mode (qk21, rect+cum) the plain entry (timed twice: the
run's own spread) and mpc_episodes_run_obstacles with 0, 1, 4 and 16 circles.
The circles lie where no robot goes: the VALU of the test is paid either way
(straight-line predicates), and every variant's episodes make the same choices
and have the same length.  One DeviceEpisodes per variant; the variants
alternate launch by launch in one process; each launch (after an untimed
reset) sits between two device events.  With 0 circles the obstacle entry
launches the plain kernel: that row must lie inside the quartile band of the
two plain timings.  The rows pass no n_blocked_out; obstacles_4_counted passes
one (DeviceEpisodes' default) and shows what the end-of-launch reduction costs.

    python tools/robots_obstacle_cost.py [--robots 1000] [--steps 1000] [--launches 30]
                                         [--out profiles/robots_obstacles/cost.json]
Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools import cost_timing  # noqa: E402

VARIANTS = (("plain_a", None), ("obstacles_0", 0), ("obstacles_1", 1), ("obstacles_4", 4),
            ("obstacles_16", 16), ("obstacles_4_counted", 4), ("plain_b", None))


def circles(n):
    """n small circles far from every start and target: never entered."""
    return cost_timing.circles(n, lambda i: (100.0 + 0.1 * i, -100.0))


def episodes_class():
    """DeviceEpisodes for the measured rows: the obstacle entry with no circles
    too (obstacles_0), and n_blocked_out = NULL except in the counted row."""
    from diplomjourney_amd.device_episodes import DeviceEpisodes

    class MeasuredEpisodes(DeviceEpisodes):
        obstacle_entry = counted = False

        def _obstacle_args(self):
            if not (self._n_obs or self.obstacle_entry):
                return None
            return self._obs, self._n_obs, self.n_blocked.data_ptr() if self.counted else None

    return MeasuredEpisodes


def measure(eng, integ, cfgs, steps, launches, warmup):
    import torch
    eps = {}
    for name, n in VARIANTS:
        ep = episodes_class()(eng, cfgs, 3, integ, log_capacity=steps, obstacles=circles(n or 0))
        ep.obstacle_entry = n == 0
        ep.counted = name.endswith("_counted")
        eps[name] = ep

    def launch(name, _n, _batch, ev):
        ep = eps[name]
        ep.reset()
        if ev:
            ev[0].record()
        ep.run(steps)
        if ev:
            ev[1].record()

    events = cost_timing.alternate(VARIANTS, warmup, launches, launch)
    torch.cuda.synchronize()
    rows = {}
    for name, evs in events.items():
        calls, stop, cands = eps[name].read_progress()
        rows[name] = {**cost_timing.summary(evs, "launches"), "calls": int(calls.sum()),
                      "candidates": int(cands.sum()), "running": int((stop == 0).sum())}
    same = len({(r["calls"], r["candidates"]) for r in rows.values()}) == 1
    a, b, z = rows["plain_a"], rows["plain_b"], rows["obstacles_0"]
    base = 0.5 * (a["median_us"] + b["median_us"])
    for name, _ in VARIANTS:
        rows[name]["ratio_to_plain"] = rows[name]["median_us"] / base
    band = [min(a["p25_us"], b["p25_us"]), max(a["p75_us"], b["p75_us"])]
    return {"integrator": integ, "robots": len(cfgs), "n_steps": 3, "max_calls": steps,
            "rows": rows, "same_episodes_in_every_row": same,
            "plain_median_spread_us": sorted((a["median_us"], b["median_us"])),
            "plain_quartile_band_us": band,
            "zero_inside_quartile_band": band[0] <= z["median_us"] <= band[1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--robots", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=1000, help="max_calls of a launch")
    ap.add_argument("--launches", type=int, default=30, help="timed launches per variant")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches per variant")
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "robots_obstacles", "cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("robots_obstacle_cost.py needs a GPU")
    from diplomjourney_amd import run_math_model as rmm
    from diplomjourney_amd.episode_config import tree_episode_config
    from diplomjourney_amd.expansion import Expansion
    eng = Expansion("cuda:0")
    starts = rmm.draw_starts(args.robots, seed=20261015)
    cfgs = [tree_episode_config(s, args.steps) for s in starts]
    modes = [measure(eng, integ, cfgs, args.steps, args.launches, args.warmup)
             for integ in ("qk21", "rect+cum")]
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "one device-event pair per launch (a whole run of every episode), "
                        "variants alternated launch by launch",
              "modes": modes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for m in modes:
        print(m["integrator"], "plain band", m["plain_quartile_band_us"], "zero inside",
              m["zero_inside_quartile_band"], "same episodes", m["same_episodes_in_every_row"])
        for name, r in m["rows"].items():
            print(f"  {name:19s} median {r['median_us']:9.1f} us  p25 {r['p25_us']:9.1f}  "
                  f"p75 {r['p75_us']:9.1f}  x{r['ratio_to_plain']:.3f}")


if __name__ == "__main__":
    main()
