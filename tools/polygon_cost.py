"""What keep-out polygons cost the streaming rollout kernel.

Times mpc_rollout_partials (twice: the run's own spread), the keep-out entry
with nothing (the same kernel), 16 circles through the existing circle entry,
and the keep-out entry with 1 triangle, 1 octagon, 4 octagons and 4 octagons +
16 circles — alternating the variants launch by launch inside one process,
each launch between two device events, over a pool of distinct control batches
larger than the 256-MiB Infinity Cache.  Every variant is reported as a ratio
to the plain timing of the same run, with its quartiles.

One child process per mode, each under its own `timeout`; the first that fails
ends the run (nothing more is started on the GPU after it).

    python tools/polygon_cost.py [--n-cand 1000000] [--n-steps 10] [--launches 200]
                                 [--out profiles/polygons/cost.json]
Needs a GPU (no fallback)."""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools import cost_timing  # noqa: E402

# name -> (circles, polygons as (count, vertices)); None: mpc_rollout_partials
VARIANTS = (("partials_a", None), ("keepout_nothing", (0, 0, 0)), ("circles_16", (16, 0, 0)),
            ("triangle_1", (0, 1, 3)), ("octagon_1", (0, 1, 8)), ("octagons_4", (0, 4, 8)),
            ("octagons_4_circles_16", (16, 4, 8)), ("partials_b", None))
MODES = "rect+cum,rect+rot,qk21"


def _ring(i):
    return 0.3 * math.cos(0.3 + 0.15 * i), 0.3 * math.sin(0.3 + 0.15 * i)


def polygons(n, vertices):
    """n small regular polygons on the ring the candidates cross (the test is a
    loop over the count with straight-line code per polygon: its cost does not
    depend on where they are)."""
    return [[(cx + cost_timing.RADIUS * math.cos(0.1 + 2 * math.pi * k / vertices),
              cy + cost_timing.RADIUS * math.sin(0.1 + 2 * math.pi * k / vertices))
             for k in range(vertices)] for cx, cy in (_ring(2 * i + 1) for i in range(n))]


def measure(eng, mode, n_cand, n_steps, launches, warmup, pool_batches):
    import torch
    from diplomjourney_amd import native
    from diplomjourney_amd.abi import INTEGRATORS, make_obstacles, make_polygons, make_problem
    lib, dev = eng.lib, eng.device
    V = torch.linspace(0.2, 0.95, 16, dtype=torch.float64, device=dev)
    B = torch.linspace(-0.5, 0.5, 33, dtype=torch.float64, device=dev)
    pool = [eng.sample_controls(V, B, n_cand, n_steps, seed=1000 + k, const_prefix=False)
            for k in range(pool_batches)]
    prob = make_problem(0, 0, 0.3, 2, 3, 0, 0, 0.5, 0.05, 0.10)
    integ = INTEGRATORS[mode]
    ws_bytes = lib.mpc_workspace_bytes(n_cand, n_steps)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    args = {name: (make_obstacles(cost_timing.circles(a[0], _ring)),
                   make_polygons(polygons(a[1], a[2])))
            for name, a in VARIANTS if a is not None}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(name, a, batch, events):
        v, b = pool[batch % len(pool)]
        if events:
            events[0].record()
        if a is None:
            st = lib.mpc_rollout_partials(ctypes.byref(prob), v.data_ptr(), b.data_ptr(), n_cand,
                                          n_steps, integ, None, ws.data_ptr(), ws_bytes, stream)
        elif a[1] == 0 and a[0] > 0:
            (obs, n_obs), _ = args[name]
            st = lib.mpc_rollout_partials_obstacles(
                ctypes.byref(prob), obs, n_obs, v.data_ptr(), b.data_ptr(), n_cand, n_steps, integ,
                None, ws.data_ptr(), ws_bytes, None, stream)
        else:
            (obs, n_obs), (poly, n_poly) = args[name]
            st = lib.mpc_rollout_partials_keepout(
                ctypes.byref(prob), obs, n_obs, poly, n_poly, v.data_ptr(), b.data_ptr(), n_cand,
                n_steps, integ, None, ws.data_ptr(), ws_bytes, None, stream)
        native.check(st, "rollout partials")
        if events:
            events[1].record()

    events = cost_timing.alternate(VARIANTS, warmup, launches, launch)
    torch.cuda.synchronize()
    rows = {name: cost_timing.summary(evs, "launches") for name, evs in events.items()}
    a, b, z = rows["partials_a"], rows["partials_b"], rows["keepout_nothing"]
    lo, hi = sorted((a["median_us"], b["median_us"]))
    base = 0.5 * (lo + hi)
    for name, _ in VARIANTS:
        for q in ("median", "p25", "p75"):
            rows[name][f"{q}_ratio_to_plain"] = rows[name][f"{q}_us"] / base
    return {
        "mode": mode, "n_cand": n_cand, "n_steps": n_steps,
        "pool_bytes": 16 * n_cand * n_steps * len(pool), "rows": rows,
        "plain_median_spread_us": [lo, hi],
        "plain_quartile_spread_us": [min(a["p25_us"], b["p25_us"]), max(a["p75_us"], b["p75_us"])],
        "nothing_inside_quartile_spread":
            min(a["p25_us"], b["p25_us"]) <= z["median_us"] <= max(a["p75_us"], b["p75_us"]),
        "octagons_4_over_circles_16":
            rows["octagons_4"]["median_us"] / rows["circles_16"]["median_us"],
    }


def one_mode(args):
    """The child: one mode, its result as JSON to args.out."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("polygon_cost.py needs a GPU")
    from diplomjourney_amd.expansion import Expansion
    eng = Expansion("cuda:0")
    m = measure(eng, args.one_mode, args.n_cand, args.n_steps, args.launches, args.warmup,
                args.pool)
    m["device"] = torch.cuda.get_device_name(0)
    with open(args.out, "w") as fh:
        json.dump(m, fh)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-cand", type=int, default=1_000_000)
    ap.add_argument("--n-steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200, help="timed launches per variant")
    ap.add_argument("--warmup", type=int, default=20, help="untimed launches per variant")
    ap.add_argument("--pool", type=int, default=4, help="distinct control batches")
    ap.add_argument("--modes", default=MODES)
    ap.add_argument("--mode-timeout", type=int, default=150, help="seconds per mode's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "polygons", "cost.json"))
    ap.add_argument("--one-mode", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one_mode:
        return one_mode(args)
    if 16 * args.n_cand * args.n_steps * args.pool <= 256 << 20:
        print("warning: the batch pool fits the 256-MiB Infinity Cache", file=sys.stderr)
    modes = []
    with tempfile.TemporaryDirectory() as tmp:
        for mode in args.modes.split(","):
            part = os.path.join(tmp, "mode.json")
            cmd = ["timeout", "-k", "10", str(args.mode_timeout), sys.executable,
                   os.path.abspath(__file__), "--one-mode", mode, "--out", part]
            for k in ("n_cand", "n_steps", "launches", "warmup", "pool"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
            rc = subprocess.run(cmd).returncode
            if rc != 0:   # a fault, an abort or the time limit: start nothing more
                sys.exit(f"polygon_cost.py: mode {mode} ended with status {rc}; stopping")
            with open(part) as fh:
                modes.append(json.load(fh))
    result = {"device": modes[0].pop("device"),
              "timing": "one device-event pair per launch, variants alternated launch by launch",
              "modes": modes}
    for m in modes[1:]:
        m.pop("device", None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for m in modes:
        print(m["mode"], "plain spread", m["plain_median_spread_us"], "nothing inside",
              m["nothing_inside_quartile_spread"], "4 octagons / 16 circles",
              round(m["octagons_4_over_circles_16"], 3))
        for name, r in m["rows"].items():
            print(f"  {name:22s} median {r['median_us']:8.2f} us  p25 {r['p25_us']:8.2f}  "
                  f"p75 {r['p75_us']:8.2f}  x{r['median_ratio_to_plain']:.3f} "
                  f"(x{r['p25_ratio_to_plain']:.3f}-x{r['p75_ratio_to_plain']:.3f})")


if __name__ == "__main__":
    main()
