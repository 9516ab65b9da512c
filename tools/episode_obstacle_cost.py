"""What keep-out circles cost a device-resident episode step.

Config C's shape (1e6 x 10, L = 0.5, rect+cum), two step forms:
  two_launch     mpc_episode_partials + mpc_episode_finalize on SoA controls
  chained_tiled  mpc_episode_chain_step on MPC_LAYOUT_TILED controls
each as the plain entry (timed twice: the run's own spread) and as the obstacle
entry with 0, 1, 4 and 16 circles.  One DeviceEpisode per variant, all stepping
over one pool of resident control batches larger than the 256-MiB Infinity
Cache; the variants alternate step by step in one process, each step between
two device events.  The circles lie beside the path, so every variant's episode
makes the same choices and the selection does the same work.  With 0 circles
the obstacle entries call the plain ones: that row must lie inside the quartile
band of the two plain timings.  The rows pass no n_blocked_out, so that they time
the launches alone; obstacles_4_counted passes one (DeviceEpisode's default) and
shows the cost of zeroing it on the stream.

    python tools/episode_obstacle_cost.py [--n-cand 1000000] [--n-steps 10] [--steps 200]
                                          [--out profiles/episode_obstacles/cost.json]
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
    """n small circles beside the path from (0, 0) to the target (2, 3): never
    entered."""
    return cost_timing.circles(n, lambda i: (0.6 + 0.1 * i, -0.5))


def episode_class():
    """DeviceEpisode for the measured rows: the obstacle entries with no
    circles too (obstacles_0: their dispatch of the plain kernels), and
    n_blocked_out = NULL (no memset node on the stream: the launches alone)
    except in the row that shows what the count costs."""
    from diplomjourney_amd.episode import DeviceEpisode

    class MeasuredEpisode(DeviceEpisode):
        obstacle_entries = counted = False

        def _obstacle_args(self):
            if not (self._n_obs or self.obstacle_entries):
                return None
            return self._obs, self._n_obs, self.n_blocked.data_ptr() if self.counted else None

    return MeasuredEpisode


def measure(eng, form, n_cand, n_steps, steps, warmup, pool):
    import torch
    chained = form == "chained_tiled"
    eps = {}
    for name, n in VARIANTS:
        ep = episode_class()(eng, n_cand, n_steps, integrator="rect+cum", chain=chained,
                             log_capacity=64, obstacles=circles(n or 0))
        ep.obstacle_entries = n == 0
        ep.counted = name.endswith("_counted")
        eps[name] = ep
    events = cost_timing.alternate(
        VARIANTS, warmup, steps,
        lambda name, _n, batch, ev: eps[name].step(events=ev, controls=pool[batch % len(pool)]))
    for ep in eps.values():
        ep.flush()
    torch.cuda.synchronize()
    rows = {name: {**cost_timing.summary(evs, "steps"), "chain_error": eps[name].chain_error()}
            for name, evs in events.items()}
    a, b, z = rows["plain_a"], rows["plain_b"], rows["obstacles_0"]
    base = 0.5 * (a["median_us"] + b["median_us"])
    for name, _ in VARIANTS:
        rows[name]["ratio_to_plain"] = rows[name]["median_us"] / base
    band = [min(a["p25_us"], b["p25_us"]), max(a["p75_us"], b["p75_us"])]
    return {"form": form, "n_cand": n_cand, "n_steps": n_steps, "L": 0.5,
            "integrator": "rect+cum", "pool_bytes": 16 * n_cand * n_steps * len(pool),
            "rows": rows, "plain_median_spread_us": sorted((a["median_us"], b["median_us"])),
            "plain_quartile_band_us": band,
            "zero_inside_quartile_band": band[0] <= z["median_us"] <= band[1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-cand", type=int, default=1_000_000)
    ap.add_argument("--n-steps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps per variant")
    ap.add_argument("--pool", type=int, default=4, help="distinct control batches")
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "episode_obstacles", "cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("episode_obstacle_cost.py needs a GPU")
    if 16 * args.n_cand * args.n_steps * args.pool <= 256 << 20:
        print("warning: the batch pool fits the 256-MiB Infinity Cache", file=sys.stderr)
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.expansion import Expansion, soa_to_tiled
    eng = Expansion("cuda:0")
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device=eng.device)
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device=eng.device)
    soa = [eng.sample_controls(V, B, args.n_cand, args.n_steps, 1000 + k)
           for k in range(args.pool)]
    forms = [measure(eng, "two_launch", args.n_cand, args.n_steps, args.steps, args.warmup, soa)]
    tiled = [soa_to_tiled(v, b) for v, b in soa]
    del soa
    forms.append(measure(eng, "chained_tiled", args.n_cand, args.n_steps, args.steps, args.warmup,
                         tiled))
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "one device-event pair per step, variants alternated step by step",
              "forms": forms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for m in forms:
        print(m["form"], "plain band", m["plain_quartile_band_us"], "zero inside",
              m["zero_inside_quartile_band"])
        for name, r in m["rows"].items():
            print(f"  {name:19s} median {r['median_us']:8.2f} us  p25 {r['p25_us']:8.2f}  "
                  f"p75 {r['p75_us']:8.2f}  x{r['ratio_to_plain']:.3f}")


if __name__ == "__main__":
    main()
