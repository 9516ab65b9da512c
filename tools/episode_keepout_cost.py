"""What keep-out polygons cost a device-resident episode step.

Config C's shape (1e6 x 10, L = 0.5, rect+cum), two step forms:
  two_launch     mpc_episode_partials + mpc_episode_finalize on SoA controls
  chained_tiled  mpc_episode_chain_step on MPC_LAYOUT_TILED controls
each as the plain entry (timed twice: the run's own spread) and as the keep-out
entry with no polygon, one triangle, one octagon, four octagons, four octagons
and 16 circles, and four octagons with n_blocked_out.  One DeviceEpisode per
variant, all stepping over one pool of resident control batches larger than the
256-MiB Infinity Cache; the variants alternate step by step in one process,
each step between two device events.  The shapes lie beside the path, so every
variant's episode makes the same choices and the selection does the same work.
With no polygon (and no circle) the keep-out entries call the plain ones: that
row must lie inside the quartile band of the two plain timings.  The rows pass
no n_blocked_out, so that they time the launches alone, except the last.

Each row states the VALU instructions the hook adds per candidate and step, as
counted in the source: an edge slot is 2 fma and 1 compare per candidate, and a
polygon's 8 slots are all evaluated whatever its vertex count (24 per polygon);
a circle is 2 subtractions, 1 product, 1 fma and 1 compare (5 per circle, all
16 slots of the instantiation: 80).

    python tools/episode_keepout_cost.py [--n-cand 1000000] [--n-steps 10] [--steps 200]
                                         [--out profiles/episode_keepout/cost.json]
Needs a GPU (no fallback)."""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools import cost_timing  # noqa: E402

# (row, polygons as vertex counts or None for the plain entry, circles, counted)
VARIANTS = (("plain_a", None, 0, False), ("keepout_0", (), 0, False),
            ("triangle_1", (3,), 0, False), ("octagon_1", (8,), 0, False),
            ("octagon_4", (8,) * 4, 0, False), ("octagon_4_circles_16", (8,) * 4, 16, False),
            ("octagon_4_counted", (8,) * 4, 0, True), ("plain_b", None, 0, False))
EDGE_VALU, SLOTS, CIRCLE_VALU, CIRCLE_SLOTS = 3, 8, 5, 16
# the one-shot kernels' ratios to their plain call (DESIGN.md §5 "Keep-out polygons",
# profiles/polygons/cost.json): the scalar-operand form of the same loop
ONE_SHOT_RATIO = {"octagon_1": 1.17, "octagon_4": 1.95}


def polygons(counts):
    """Small regular polygons beside the path from (0, 0) to the target (2, 3):
    never entered."""
    out = []
    for i, n in enumerate(counts):
        cx, cy, r = 0.6 + 0.2 * i, -0.6, 0.05
        out.append([(cx + r * math.cos(2 * math.pi * k / n), cy + r * math.sin(2 * math.pi * k / n))
                    for k in range(n)])
    return out


def circles(n):
    return cost_timing.circles(n, lambda i: (0.6 + 0.1 * i, -1.0))


def added_valu(poly, n_circles):
    """VALU per candidate and step that the hook adds (see the module's text)."""
    if poly is None:
        return 0
    return len(poly) * SLOTS * EDGE_VALU + (CIRCLE_SLOTS * CIRCLE_VALU if n_circles else 0)


def episode_class():
    """DeviceEpisode for the measured rows: the keep-out entries with no polygon
    too (keepout_0: their dispatch of the plain kernels), and n_blocked_out =
    NULL (no memset node on the stream) except in the counted row."""
    from diplomjourney_amd.episode import DeviceEpisode

    class MeasuredEpisode(DeviceEpisode):
        keepout_entries = counted = False

        def _polygon_args(self):
            if not (self._n_poly or self.keepout_entries):
                return None
            return self._poly, self._n_poly

        def _obstacle_args(self):
            if not (self._n_obs or self._n_poly or self.keepout_entries):
                return None
            return self._obs, self._n_obs, self.n_blocked.data_ptr() if self.counted else None

    return MeasuredEpisode


def measure(eng, form, n_cand, n_steps, steps, warmup, pool):
    import torch
    chained = form == "chained_tiled"
    eps = {}
    for name, poly, n_circ, counted in VARIANTS:
        ep = episode_class()(eng, n_cand, n_steps, integrator="rect+cum", chain=chained,
                             log_capacity=64, obstacles=circles(n_circ),
                             polygons=polygons(poly or ()))
        ep.keepout_entries = poly == ()
        ep.counted = counted
        eps[name] = ep
    order = tuple((name, None) for name, *_ in VARIANTS)
    events = cost_timing.alternate(
        order, warmup, steps,
        lambda name, _n, batch, ev: eps[name].step(events=ev, controls=pool[batch % len(pool)]))
    for ep in eps.values():
        ep.flush()
    torch.cuda.synchronize()
    rows = {name: {**cost_timing.summary(evs, "steps"), "chain_error": eps[name].chain_error()}
            for name, evs in events.items()}
    a, b, z = rows["plain_a"], rows["plain_b"], rows["keepout_0"]
    base = 0.5 * (a["median_us"] + b["median_us"])
    for name, poly, n_circ, _ in VARIANTS:
        rows[name]["ratio_to_plain"] = rows[name]["median_us"] / base
        rows[name]["added_valu_per_candidate_step"] = added_valu(poly, n_circ)
        if name in ONE_SHOT_RATIO:
            rows[name]["one_shot_ratio_to_plain"] = ONE_SHOT_RATIO[name]
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
                    default=os.path.join(REPO, "profiles", "episode_keepout", "cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("episode_keepout_cost.py needs a GPU")
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
            print(f"  {name:21s} median {r['median_us']:8.2f} us  p25 {r['p25_us']:8.2f}  "
                  f"p75 {r['p75_us']:8.2f}  x{r['ratio_to_plain']:.3f}  "
                  f"+{r['added_valu_per_candidate_step']} VALU")


if __name__ == "__main__":
    main()
