"""Phase timelines of the three device-resident step forms, from the stamps that
csrc/mpc_timeline.h compiles in under -DMPC_TIMELINE (s_memrealtime, 100 MHz;
the product carries none).  The variant library is tools/tl_variant.so
(__graft_entry__.build() makes it).  Every mode runs in a process of its own
against it, on the GPU, and ends with a `JSON ` line.

    python tools/timeline.py chain N_CAND N [soa|tiled|p2p] [--reps 5] [--steps 300]
    python tools/timeline.py episodes [R] [K] [--integ qk21] [--n-steps 3] [--reps 3] [--park I]
    python tools/timeline.py run N_CAND N K [soa|tiled] [--reps 3]
    python tools/timeline.py fleet [R] [NEIGHBOURS] [--integ qk21] [--reps 5]

chain: the chained step (k_episode_chain), one launch among back-to-back ones
(tiled: the bench default's tiled batches; p2p: the one-rank P2P exchange form).
Block 0 (completion of step k-1, B0): entry, records loaded + lane minima, wave
arg-min, block winner (after the barrier), winner re-rolled (emit_winner),
episode updated (thread 0), head stored + constants published.  P2P (B0_P2P):
candidate from the records, posted, the world's gathered, advance, published.
Tile blocks (TILE): entry, first control DMAs in flight (pre0), final constants
in hand (after the loop), record stored.
episodes: workload R's kernel (k_episodes_run: one block per robot runs its
episode's MPC steps back to back), summed per phase over every call of a block
(thread 0's view), then the mean per call (PH): grid (episode_grids + barrier),
rollout (thread 0's own candidates), argmin (block arg-min + barrier), re-roll
(emit_winner), advance (thread 0: episode_advance), log (barrier + log store).
The plain kernel only: the circle instantiations live in the second translation
unit and stamp a table of their own that no entry reads.  --park I: robot I
starts on its target (no call).
fleet: one fleet call (mpc_episodes_fleet_run, n_calls = 1) beside one
max_calls = 1 launch of the plain kernel for the same robots (tools/fleet_cost.py's
clusters: every robot with NEIGHBOURS others within reach, nothing blocked), the
same phases, the mean over the robots.  The fleet call forms its table — the
board scan, the selection — between the call's start and the grid's barrier, so
its `grid` phase less the plain one's is what the selection takes (the second
unit's table: mpc_debug_timeline's which = 3).  A predicted fleet call
(mpc_episodes_fleet_run_predicted, fleet call 0: every motion entry zero, the
work the same) is stamped beside it: its `grid` phase less the fleet call's is
the per-step tables' formation; the motion write follows the last stamp.  A
planned fleet call (mpc_episodes_fleet_run_planned, fleet call 0: everybody's
plan is to stand, the work the same) likewise: plan_formation_ns, and its phases
less the predicted call's.
run: the persistent run (k_episode_run), per step of the last launch (the
fields: csrc/mpc_timeline.h)."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 2048 + 1            # tl::kChainBlocks
B0_BASE = 8 * NB         # block 0's stamps follow the blocks' 8 each
B0 = ["entry", "records", "wave argmin", "block winner", "controls in LDS", "re-roll",
      "advance", "update", "published", "adv-entry", "finishing", "pre-prepare", "prepared",
      "early pub", "tail done", "t64 early prep", "ew bcast", "ew phase1", "w1 sincos", "l0 pose"]
B0_P2P = {1: "candidate", 2: "posted", 3: "gathered", 6: "advance", 8: "published"}
TILE = ["entry", "DMAs issued", "final consts", "record stored", "costs done", "argmin done"]
PH = ["grid", "rollout", "argmin", "re-roll", "advance", "log"]
RUN_STEPS = 64           # tl::kRunSteps
CHAIN_TL, EPISODES_TL, RUN_TL, FLEET_TL = 0, 1, 2, 3   # mpc_debug_timeline's `which`


def variant():
    """The variant library, chosen before this process's first native.lib(); its debug entry."""
    sys.path.insert(0, REPO)
    from diplomjourney_amd import native
    native.LIB_PATH = native.TIMELINE_LIB
    L = native.lib()
    L.mpc_debug_timeline.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return L


def table(L, which, words):
    buf = (ctypes.c_uint64 * words)()   # (the first words of the table; the device is idle)
    assert L.mpc_debug_timeline(which, buf, ctypes.sizeof(buf), 0) == 0
    return list(buf)


def digest(ep):
    """What a timeline run must leave as the product leaves it (syncs)."""
    log = hashlib.sha256(ep.log.cpu().numpy().tobytes()).hexdigest()
    if hasattr(ep, "local"):
        return {"log": log, "result": ep.local.cpu().numpy().tobytes().hex(), "chain_error": ep.chain_error()}
    calls, stop, cands = (a.tolist() for a in ep.read_progress())
    return {"log": log, "calls": calls, "stop": stop, "candidates": cands}


def chain_episode(n, ns, mode="soa", pool=8, seed0=0x5EED0000):
    """The chained rect+cum episode of `chain` and `run`, and its control batches."""
    import torch
    from diplomjourney_amd import math_model_tree as mmt
    from diplomjourney_amd.episode import DeviceEpisode
    from diplomjourney_amd.expansion import Expansion
    eng = Expansion("cuda:0")
    V = torch.tensor(mmt.vector_of_velocities(0.5), dtype=torch.float64, device="cuda")
    B = torch.tensor(mmt.vector_of_beta_angles(0.0), dtype=torch.float64, device="cuda")
    smp = eng.sample_controls_tiled if mode == "tiled" else eng.sample_controls
    p2p = mode == "p2p"
    ep = DeviceEpisode(eng, n, ns, integrator="rect+cum", chain=True, log_capacity=4096,
                       exchange=p2p, p2p=p2p)
    return ep, [smp(V, B, n, ns, seed0 + i) for i in range(pool)]


def chain_steps(n, ns, mode, reps, steps, each=None):
    """reps x steps chained steps, each(rep) after a rep's (synchronised), then the flush."""
    import torch
    ep, pool = chain_episode(n, ns, mode)
    for rep in range(reps):
        for i in range(steps):
            ep.step(controls=pool[i % len(pool)])
        torch.cuda.synchronize()
        if each:
            each(rep)
    ep.flush()
    return ep


def chain(a):
    L = variant()
    n, ns = a.n_cand, a.n_steps
    nb = min((n + 511) // 512, NB - 1) + 1   # block 0 + the tile blocks (512 candidates each)
    names = B0_P2P if a.mode == "p2p" else {q: name for q, name in enumerate(B0) if q}
    assert L.mpc_debug_timeline(CHAIN_TL, None, 0, 1) == 0
    rows, raw = [], []

    def each(_rep):
        raw[:] = table(L, CHAIN_TL, B0_BASE + 32)
        t0 = min(raw[8 * b] for b in range(nb))
        us = lambda x: (x - t0) * 0.01   # noqa: E731
        row = {"block0": {"entry": us(raw[0]), **{nm: us(raw[B0_BASE + q]) for q, nm in names.items()}}}
        for q, name in enumerate(TILE):
            xs = sorted(us(raw[8 * b + q]) for b in range(1, nb))
            row[name] = [xs[int(p * (len(xs) - 1))] for p in (0.1, 0.5, 0.9)] + [xs[-1]]
        rows.append(row)

    state = digest(chain_steps(n, ns, a.mode, a.reps, a.steps, each))
    assert state["chain_error"] == 0
    print(f"chained step, {n} candidates, N = {ns}, {nb} blocks; us after the first block's entry")
    for r in rows:
        print("  block 0: " + "  ".join(f"{k} {v:5.2f}" for k, v in r["block0"].items()))
        print("  tiles p10/p50/p90/max: " + "  ".join(
            f"{k} " + "/".join(f"{x:.2f}" for x in r[k]) for k in TILE))
    # the raw stamps of the last rep: the grid's blocks and two past it; block 0's own
    print("JSON " + json.dumps({"rows": rows, "blocks": nb, "b0_slots": sorted(names), "state": state,
                                "tiles": raw[:8 * (nb + 2)], "b0": raw[B0_BASE:]}))


def robots(R, K, integ="qk21", park=None, n_steps=3):
    """Workload R's batch: R drawn run_math_model episodes, at most K calls each."""
    from diplomjourney_amd import run_math_model as rmm
    from diplomjourney_amd.episode import DeviceEpisodes, tree_episode_config
    from diplomjourney_amd.expansion import Expansion
    starts = rmm.draw_starts(R, seed=20261015)
    if park is not None:
        starts[park] = starts[park][:3] + starts[park][:2]
    return DeviceEpisodes(Expansion("cuda:0"), [tree_episode_config(s, K) for s in starts], n_steps,
                          integ, log_capacity=K)


def episodes(a):
    L = variant()
    import time
    import torch
    R, K = a.robots, a.calls
    eps = robots(R, K, a.integ, a.park, a.n_steps)
    for rep in range(a.reps):
        eps.reset()
        assert L.mpc_debug_timeline(EPISODES_TL, None, 0, 1) == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eps.run(K)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        calls, _, _ = eps.read_progress()
        raw = table(L, EPISODES_TL, 8 * (R + 2))
        tl = [raw[8 * r:8 * r + 8] for r in range(R + 2)]   # (two blocks past the grid)
        longest = max(range(R), key=lambda r: tl[r][6])
        tot = [sum(tl[r][q] for r in range(R)) for q in range(7)]

        def fmt(row):
            n = max(1, row[6])
            per = {p: row[q] * 10.0 / n for q, p in enumerate(PH)}   # ns per call
            return per, "  ".join(f"{k} {v:.0f}" for k, v in per.items()) + \
                f"  total {sum(per.values()):.0f} ns/call over {n} calls"
        per, txt = fmt(tl[longest])
        print(f"run {dt * 1e3:.2f} ms ({dt / max(1, calls.max()) * 1e6:.2f} us/lockstep step)\n"
              f"  longest robot {longest}: {txt}\n  all robots: {fmt(tot)[1]}", flush=True)
    print("JSON " + json.dumps({"per_call_ns": per, "robots": tl, "state": digest(eps)}))


def fleet(a):
    L = variant()
    import torch
    from diplomjourney_amd.device_episodes import DeviceEpisodes, DeviceFleet
    from diplomjourney_amd.expansion import Expansion
    from tools import fleet_cost as FC
    eng = Expansion("cuda:0")
    R = a.robots
    cfgs = FC.fleet_configs(R, a.neighbours)
    batches = {"plain": (EPISODES_TL, DeviceEpisodes(eng, cfgs, 3, a.integ, log_capacity=1)),
               "fleet": (FLEET_TL, DeviceFleet(eng, cfgs, FC.CLEARANCE, 3, a.integ,
                                               log_capacity=1, reach=FC.REACH)),
               "predicted": (FLEET_TL, DeviceFleet(eng, cfgs, FC.CLEARANCE, 3, a.integ,
                                                   log_capacity=1, reach=FC.REACH, predict=True)),
               "planned": (FLEET_TL, DeviceFleet(eng, cfgs, FC.CLEARANCE, 3, a.integ,
                                                 log_capacity=1, reach=FC.REACH, predict="plan"))}
    out = {}
    for name, (which, ep) in batches.items():
        mean = [0.0] * 6
        for _ in range(a.reps):
            ep.reset()
            assert L.mpc_debug_timeline(which, None, 0, 1) == 0
            torch.cuda.synchronize()
            ep.run(1)
            torch.cuda.synchronize()
            raw = table(L, which, 8 * R)
            assert all(raw[8 * r + 6] == 1 for r in range(R)), "a robot without its one call"
            for q in range(6):
                mean[q] += sum(raw[8 * r + q] for r in range(R)) * 10.0 / (R * a.reps)
        out[name] = dict(zip(PH, mean))
        # the last rep's blocks: the launch ends with its slowest
        tot = sorted(sum(raw[8 * r:8 * r + 6]) * 10 for r in range(R))
        out[name + "_block_ns_p50_p99_max"] = [tot[len(tot) // 2], tot[(99 * len(tot)) // 100],
                                               tot[-1]]
        print(f"{name:9s} " + "  ".join(f"{k} {v:.0f}" for k, v in out[name].items())
              + f"  total {sum(mean):.0f} ns/call; blocks p50 / p99 / max "
              + " / ".join(str(t) for t in out[name + "_block_ns_p50_p99_max"]), flush=True)
    within = [w for w, _ in batches["fleet"][1].read_neighbours()]
    out["selection_ns"] = out["fleet"]["grid"] - out["plain"]["grid"]
    out["share_of_call"] = out["selection_ns"] / sum(out["fleet"][k] for k in PH)
    print(f"selection (grid, fleet less plain): {out['selection_ns']:.0f} ns, "
          f"{100 * out['share_of_call']:.1f} % of the fleet call's phases; neighbours "
          f"{min(within)}..{max(within)}")
    # a predicted call forms its per-step tables right after the selection (and,
    # rect+cum, their frame form after the grid's barrier: the rollout phase's head)
    out["formation_ns"] = out["predicted"]["grid"] - out["fleet"]["grid"]
    out["predicted_less_fleet_ns"] = {k: out["predicted"][k] - out["fleet"][k] for k in PH}
    print("predicted less fleet, per phase: "
          + "  ".join(f"{k} {v:.0f}" for k, v in out["predicted_less_fleet_ns"].items()))
    # a planned call stages the neighbours' entries in LDS ahead of the same formation
    out["plan_formation_ns"] = out["planned"]["grid"] - out["fleet"]["grid"]
    out["planned_less_predicted_ns"] = {k: out["planned"][k] - out["predicted"][k] for k in PH}
    print("planned less predicted, per phase: "
          + "  ".join(f"{k} {v:.0f}" for k, v in out["planned_less_predicted_ns"].items()))
    print("JSON " + json.dumps({"robots": R, "neighbours": a.neighbours, "integ": a.integ, **out}))


def run_steps(n, ns, K, mode, reps, before=None):
    """reps persistent runs of K steps each (before(rep): ahead of each)."""
    import torch
    ep, pool = chain_episode(n, ns, mode, pool=min(K, 20), seed0=500)
    for rep in range(reps):
        if before:
            before(rep)
        torch.cuda.synchronize()
        ep.run([pool[i % len(pool)] for i in range(K)])
        torch.cuda.synchronize()
    return ep


def run(a):
    L = variant()
    K = a.k
    assert K <= RUN_STEPS, "the table holds one launch: K <= 64"
    state = digest(run_steps(a.n_cand, a.n_steps, K, a.mode, a.reps,
                             lambda _rep: L.mpc_debug_timeline(RUN_TL, None, 0, 1)))
    print("err", state["chain_error"])
    t = [table(L, RUN_TL, 8 * RUN_STEPS)[8 * j:8 * j + 8] for j in range(RUN_STEPS)]
    us = lambda x: (x - t[0][3]) / 100.0  # noqa: E731
    print(" j  sel0   recs   done | u0    loopend waitend lastrec | poll_lat chain waited")
    for j, r in enumerate(t[:K]):
        print(f"{j:2d} {us(r[0]):6.1f} {us(r[1]):6.1f} {us(r[2]):6.1f} | {us(r[3]):6.1f} {us(r[4]):6.1f}"
              f" {us(r[5]):6.1f} {us(r[6]):6.1f} | {(r[1]-r[6])/100:5.2f} {(r[2]-r[1])/100:5.2f} {r[7]}")
    print("JSON " + json.dumps({"steps": t, "k": K, "state": state}))


# mode: (its function, positional arguments and defaults (None: required), options and defaults)
MODES = {
    "chain": (chain, {"n_cand": None, "n_steps": None, "mode": "soa"}, {"reps": 5, "steps": 300}),
    "episodes": (episodes, {"robots": 1000, "calls": 1000},
                 {"integ": "qk21", "n-steps": 3, "reps": 3, "park": None}),
    "run": (run, {"n_cand": None, "n_steps": None, "k": None, "mode": "soa"}, {"reps": 3}),
    "fleet": (fleet, {"robots": 1000, "neighbours": 4}, {"integ": "qk21", "reps": 5}),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    sub = ap.add_subparsers(required=True)
    for name, (fn, positional, options) in MODES.items():
        p = sub.add_parser(name)
        for arg, default in positional.items():
            p.add_argument(arg, type=str if arg == "mode" else int,
                           **({} if default is None else {"nargs": "?", "default": default}))
        for arg, default in options.items():
            p.add_argument("--" + arg, type=str if arg == "integ" else int, default=default)
        p.set_defaults(fn=fn)
    a = ap.parse_args(argv)
    a.fn(a)


if __name__ == "__main__":
    main()
