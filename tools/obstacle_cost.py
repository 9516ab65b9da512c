"""What a keep-out circle costs the streaming rollout kernel.

Times mpc_rollout_partials (twice: the run's own spread) and
mpc_rollout_partials_obstacles with 0, 1, 4 and 16 circles, alternating the
variants launch by launch inside one process, each launch between two device
events, over a pool of distinct control batches larger than the 256-MiB
Infinity Cache.  n_obstacles = 0 dispatches the kernel of mpc_rollout_partials,
so its time must lie inside the spread of the two plain timings.

    python tools/obstacle_cost.py [--n-cand 1000000] [--n-steps 10] [--launches 200]
                                  [--out profiles/obstacles/cost.json]
Needs a GPU (no fallback)."""
import argparse
import ctypes
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools import cost_timing  # noqa: E402

VARIANTS = (("partials_a", None), ("obstacles_0", 0), ("obstacles_1", 1), ("obstacles_4", 4),
            ("obstacles_16", 16), ("partials_b", None))


def circles(n):
    """n small circles on a ring the candidates cross."""
    return cost_timing.circles(
        n, lambda i: (0.3 * math.cos(0.3 + 0.15 * i), 0.3 * math.sin(0.3 + 0.15 * i)))


def measure(eng, mode, n_cand, n_steps, launches, warmup, pool_batches):
    import torch
    from diplomjourney_amd import native
    from diplomjourney_amd.abi import INTEGRATORS, make_obstacles, make_problem
    lib, dev = eng.lib, eng.device
    V = torch.linspace(0.2, 0.95, 16, dtype=torch.float64, device=dev)
    B = torch.linspace(-0.5, 0.5, 33, dtype=torch.float64, device=dev)
    pool = [eng.sample_controls(V, B, n_cand, n_steps, seed=1000 + k, const_prefix=False)
            for k in range(pool_batches)]
    prob = make_problem(0, 0, 0.3, 2, 3, 0, 0, 0.5, 0.05, 0.10)
    integ = INTEGRATORS[mode]
    ws_bytes = lib.mpc_workspace_bytes(n_cand, n_steps)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    obs = {n: make_obstacles(circles(n)) for _, n in VARIANTS if n is not None}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(_name, n, batch, events):
        v, b = pool[batch % len(pool)]
        if events:
            events[0].record()
        if n is None:
            st = lib.mpc_rollout_partials(ctypes.byref(prob), v.data_ptr(), b.data_ptr(), n_cand,
                                          n_steps, integ, None, ws.data_ptr(), ws_bytes, stream)
        else:
            st = lib.mpc_rollout_partials_obstacles(
                ctypes.byref(prob), obs[n][0], obs[n][1], v.data_ptr(), b.data_ptr(), n_cand,
                n_steps, integ, None, ws.data_ptr(), ws_bytes, None, stream)
        native.check(st, "rollout partials")
        if events:
            events[1].record()

    events = cost_timing.alternate(VARIANTS, warmup, launches, launch)
    torch.cuda.synchronize()
    rows = {name: cost_timing.summary(evs, "launches") for name, evs in events.items()}
    a, b, z = rows["partials_a"], rows["partials_b"], rows["obstacles_0"]
    lo, hi = sorted((a["median_us"], b["median_us"]))
    base = 0.5 * (lo + hi)
    for name, _ in VARIANTS:
        rows[name]["ratio_to_plain"] = rows[name]["median_us"] / base
    return {
        "mode": mode, "n_cand": n_cand, "n_steps": n_steps,
        "pool_bytes": 16 * n_cand * n_steps * len(pool), "rows": rows,
        "plain_median_spread_us": [lo, hi],
        "plain_quartile_spread_us": [min(a["p25_us"], b["p25_us"]), max(a["p75_us"], b["p75_us"])],
        "zero_inside_median_spread": lo <= z["median_us"] <= hi,
        "zero_inside_quartile_spread":
            min(a["p25_us"], b["p25_us"]) <= z["median_us"] <= max(a["p75_us"], b["p75_us"]),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-cand", type=int, default=1_000_000)
    ap.add_argument("--n-steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200, help="timed launches per variant")
    ap.add_argument("--warmup", type=int, default=20, help="untimed launches per variant")
    ap.add_argument("--pool", type=int, default=4, help="distinct control batches")
    ap.add_argument("--modes", default="rect+rot,qk21")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "obstacles", "cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("obstacle_cost.py needs a GPU")
    if 16 * args.n_cand * args.n_steps * args.pool <= 256 << 20:
        print("warning: the batch pool fits the 256-MiB Infinity Cache", file=sys.stderr)
    from diplomjourney_amd.expansion import Expansion
    eng = Expansion("cuda:0")
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "one device-event pair per launch, variants alternated launch by launch",
              "modes": [measure(eng, m, args.n_cand, args.n_steps, args.launches, args.warmup,
                                args.pool) for m in args.modes.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for m in result["modes"]:
        print(m["mode"], "plain spread", m["plain_median_spread_us"], "zero inside",
              m["zero_inside_median_spread"], m["zero_inside_quartile_spread"])
        for name, r in m["rows"].items():
            print(f"  {name:13s} median {r['median_us']:8.2f} us  p25 {r['p25_us']:8.2f}  "
                  f"p75 {r['p75_us']:8.2f}  x{r['ratio_to_plain']:.3f}")


if __name__ == "__main__":
    main()
