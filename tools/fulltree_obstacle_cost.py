"""What keep-out circles cost the full tree's leaf kernel.

Times mpc_fulltree_argmin (twice: the run's own spread) and
mpc_fulltree_argmin_obstacles with 0 circles and with 1, 4 and 16 circles in
three placements, at workload F's first call (S1 = 451, 9.17e7 leaves),
alternating the variants launch by launch inside one process, each launch
between two device events with the next launches already queued (the method of
tools/obstacle_cost.py).  n_obstacles = 0 dispatches the plain entry's kernels,
so its time must lie inside the spread of the two plain timings.
  far     circles no layer-1 state can reach: what the per-piece layer and reach
          tests and the second code path cost
  graze   circles on the rim of the reachable set: some lanes' layer-1 states
          reach them, few leaves enter them (the hooked k2 loop runs)
  subtree circles on layer-0 states of the fastest controls: whole (k0, *)
          subtrees blocked, pieces skipped
Each row also records the blocked leaves of one launch.

    python tools/fulltree_obstacle_cost.py [--launches 40]
                                           [--out profiles/fulltree_obstacles/cost.json]
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

START, TARGET = (-3.0, -2.0, 0.3), (4.0, 5.0)     # bench.py's full-tree step
T_A, T_B = 0.05, 0.1
COUNTS = (1, 4, 16)


def placements(n, step):
    """{placement: n circles (x, y, r)}; step = v_max * (T_B - T_A)."""
    x, y, phi = START
    r = 0.2 * step
    far = [(x + 100.0 + 3.0 * i, y + 80.0, 1.0) for i in range(n)]
    fan = [phi + 0.08 * (i - (n - 1) / 2) for i in range(n)]
    graze = [(x + (3 * step + 0.8 * r) * math.cos(a), y + (3 * step + 0.8 * r) * math.sin(a), r)
             for a in fan]
    subtree = [(x + step * math.cos(a), y + step * math.sin(a), 0.1 * step) for a in fan]
    return {"far": far, "graze": graze, "subtree": subtree}


def measure(eng, mode, V, B, L, launches, warmup):
    import torch
    from diplomjourney_amd import native
    from diplomjourney_amd.abi import (FT_RESULT_BYTES, INTEGRATORS, MpcFulltreeProblem,
                                       make_obstacles)
    lib, dev = eng.lib, eng.device
    vg = torch.tensor(V, dtype=torch.float64, device=dev)
    bg = torch.tensor(B, dtype=torch.float64, device=dev)
    nv, nb = len(V), len(B)
    s1 = nv * nb
    prob = MpcFulltreeProblem(*START, *TARGET, START[0], START[1],
                              float(math.atan(TARGET[0] / TARGET[1])), L, T_A, T_B)
    integ = INTEGRATORS[mode]
    ws_bytes = lib.mpc_fulltree_workspace_bytes(nv, nb)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.zeros(FT_RESULT_BYTES, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = float(max(abs(v) for v in V)) * (T_B - T_A)
    variants = [("plain_a", None), ("obstacles_0", [])]
    for n in COUNTS:
        for where, circles in placements(n, step).items():
            variants.append((f"{where}_{n}", circles))
    variants.append(("plain_b", None))
    tables = {name: make_obstacles(c) for name, c in variants if c is not None}
    args = (vg.data_ptr(), nv, bg.data_ptr(), nb, math.inf, integ, 0, 1, ws.data_ptr(), ws_bytes)

    def launch(name, circles, _batch, events, counted=None):
        if events:
            events[0].record()
        if circles is None:
            st = lib.mpc_fulltree_argmin(ctypes.byref(prob), *args, out.data_ptr(), stream)
        else:
            st = lib.mpc_fulltree_argmin_obstacles(ctypes.byref(prob), *tables[name], *args,
                                                   counted, out.data_ptr(), stream)
        native.check(st, "full-tree argmin")
        if events:
            events[1].record()

    events = cost_timing.alternate(variants, warmup, launches, launch)
    torch.cuda.synchronize()
    rows = {name: cost_timing.summary(evs, "launches") for name, evs in events.items()}
    a, b, z = rows["plain_a"], rows["plain_b"], rows["obstacles_0"]
    lo, hi = sorted((a["median_us"], b["median_us"]))
    q_lo, q_hi = min(a["p25_us"], b["p25_us"]), max(a["p75_us"], b["p75_us"])
    base = 0.5 * (lo + hi)
    for name, circles in variants:
        rows[name]["ratio_to_plain"] = rows[name]["median_us"] / base
        rows[name]["above_plain_p75_us"] = max(0.0, rows[name]["median_us"] - q_hi)
        if circles is not None:
            launch(name, circles, 0, None, count.data_ptr())
            rows[name]["blocked_leaves"] = int(count.cpu()[0])
    return {"mode": mode, "s1": s1, "leaves": s1 ** 3, "rows": rows,
            "plain_median_spread_us": [lo, hi], "plain_quartile_spread_us": [q_lo, q_hi],
            "zero_inside_median_spread": lo <= z["median_us"] <= hi,
            "zero_inside_quartile_spread": q_lo <= z["median_us"] <= q_hi}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=40, help="timed launches per variant")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches per variant")
    ap.add_argument("--modes", default="rect+rot,qk21")
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "fulltree_obstacles", "cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fulltree_obstacle_cost.py needs a GPU")
    from diplomjourney_amd import run_math_model as rmm
    from diplomjourney_amd.expansion import Expansion
    rmm.configure(0.1, math.radians(3))           # workload F's grid: 11 x 41 = 451
    V = np.asarray(rmm.vector_v, dtype=np.float64).tolist()
    B = np.asarray(rmm.vector_beta, dtype=np.float64).tolist()
    eng = Expansion("cuda:0")
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "one device-event pair per launch, variants alternated launch by launch",
              "modes": [measure(eng, m, V, B, float(rmm.L), args.launches, args.warmup)
                        for m in args.modes.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for m in result["modes"]:
        print(m["mode"], "S1", m["s1"], "plain spread", m["plain_median_spread_us"],
              "quartiles", m["plain_quartile_spread_us"], "zero inside",
              m["zero_inside_median_spread"], m["zero_inside_quartile_spread"])
        for name, r in m["rows"].items():
            print(f"  {name:13s} median {r['median_us']:9.1f} us  p25 {r['p25_us']:9.1f}  "
                  f"p75 {r['p75_us']:9.1f}  x{r['ratio_to_plain']:.4f}  "
                  f"blocked {r.get('blocked_leaves', '-')}")


if __name__ == "__main__":
    main()
