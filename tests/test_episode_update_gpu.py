"""The device-resident episode's update pinned to a host model, every branch
and every field, bit for bit (`==` on the raw bits, no tolerance anywhere):
what the episode DOES with a step's winner — episode_advance, episode_restart,
episode_prepare, episode_early_prepare, turn_target (csrc/mpc_episode.h),
episode_grids (csrc/mpc_generated.h) and the finishing layer the chained
step's early publication picks (csrc/mpc_finalize.h).  Which candidate wins is
pinned elsewhere (tests/test_ranking_gpu.py, tests/test_fulltree_replica_gpu.py).

The expected value of every field comes from tests/episode_model.py, a plain-
Python restatement that is itself pinned on the CPU to the reference's recorded
run and to oracle.parity's episode oracles (tests/test_episode_model_cpu.py);
nothing in it is read from the device.

  layer 1  mpc_episode_advance driven directly over tests/episode_cases.py's
           table: a model-made EpisodeState and fabricated result rows per
           case, one launch each, one synchronisation in all.
  layer 2  the step's grids, seed and sampled batch (mpc_episode_sample), and
           the generated step (mpc_episode_generate_step) on the same states.
  layer 3  the update through its other callers, from reset(): two-launch,
           fused, generated, chained SoA, chained tiled and the persistent run,
           steered by the cfg alone, every log record and the final state.

Left out here: the exchange forms' advance_from_candidates, the P2P and the
overlapped forms (multi-GPU step structures), the batched robots
(csrc/mpc_episodes.h, RESTART = false) and the full-tree episodes."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import episode_cases as EC
import episode_model as EM
import episode_state as ES
import ranking
from diplomjourney_amd import native
from diplomjourney_amd.abi import (INTEGRATORS, LOG_BYTES, RESULT_BYTES, MpcEpisodeLog,
                                   MpcResult)
from diplomjourney_amd.episode import reference_episode_config

pytestmark = pytest.mark.gpu

SB = ES.state_bytes()
MAX_ROWS = 4          # result rows per case (n_results 1..4)
LOG_SLOTS = 3         # log slots per case (cap 0, 1 or 3)
LOG_FILL = 0xA5       # what an untouched log byte holds


def _dev(buf, device):
    return torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(device)


def _name_state_diff(got_raw, want_raw):
    got = ES.EpisodeState.from_buffer_copy(bytes(got_raw))
    want = ES.EpisodeState.from_buffer_copy(bytes(want_raw))
    return [(n, getattr_path(got, n), getattr_path(want, n)) for n in ES.diff(got, want)][:12]


def getattr_path(obj, path):
    for part in path.replace("]", "").replace("[", ".").split("."):
        obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
    if isinstance(obj, ctypes.Array):
        return list(obj)
    return obj.hex() if isinstance(obj, float) else obj


# ----------------------------------------------------------------------------
# layer 1
# ----------------------------------------------------------------------------
def test_advance_every_branch_matches_model(engine):
    """Every case of tests/episode_cases.py: after ONE mpc_episode_advance over
    the case's rows the whole EpisodeState equals the model's — every
    EpisodeHead field (K field by field), all of StaleTraj, chain_pub all zero,
    EarlyPub / grids / done / chain_error / p2p_seq / gathered_tag unchanged —
    and the log ring holds the model's record in slot step % cap and its fill
    everywhere else.  All launches are enqueued, then one sync, one copy back."""
    t0 = time.perf_counter()
    table = EC.case_table()
    n = len(table)
    pre = bytearray(n * SB)
    want_state = bytearray(n * SB)
    rows = bytearray(b"\xee" * (n * MAX_ROWS * RESULT_BYTES))
    want_log = bytearray(bytes([LOG_FILL]) * (n * LOG_SLOTS * LOG_BYTES))
    for i, case in enumerate(table):
        pre[i * SB:(i + 1) * SB] = bytes(case["model"].to_state())
        for r, row in enumerate(case["results"]):
            at = (i * MAX_ROWS + r) * RESULT_BYTES
            # found as a rank's finalize left it: the update must recompute it
            rows[at:at + RESULT_BYTES] = bytes(EM.result_struct(row, found=(i + r) % 2,
                                                                poison=EC.POISON))
        M, rec, _ = EC.run_model(case)
        want_state[i * SB:(i + 1) * SB] = bytes(M.to_state())
        if case["cap"] > 0 and not case["log_null"]:
            at = (i * LOG_SLOTS + rec["step"] % case["cap"]) * LOG_BYTES
            want_log[at:at + LOG_BYTES] = bytes(EM.log_struct(rec))
    t_model = time.perf_counter() - t0
    dev = engine.device
    states, results = _dev(pre, dev), _dev(rows, dev)
    logs = torch.full((n * LOG_SLOTS * LOG_BYTES,), LOG_FILL, dtype=torch.uint8, device=dev)
    lib, st = native.lib(), native.current_stream()
    assert states.data_ptr() % 128 == 0
    for i, case in enumerate(table):
        rc = lib.mpc_episode_advance(
            ctypes.byref(case["cfg"]), states.data_ptr() + i * SB,
            results.data_ptr() + i * MAX_ROWS * RESULT_BYTES, len(case["results"]),
            None if case["log_null"] else logs.data_ptr() + i * LOG_SLOTS * LOG_BYTES,
            case["cap"], st)
        assert rc == 0, (i, case["coords"])
    torch.cuda.synchronize()
    got = torch.cat([states, logs]).cpu().numpy()
    got_state, got_log = got[:n * SB].reshape(n, SB), got[n * SB:].reshape(n, -1)
    ws = np.frombuffer(bytes(want_state), dtype=np.uint8).reshape(n, SB)
    wl = np.frombuffer(bytes(want_log), dtype=np.uint8).reshape(n, -1)
    bad = np.flatnonzero((got_state != ws).any(axis=1) | (got_log != wl).any(axis=1))
    msgs = []
    for i in bad[:5]:
        gl = [MpcEpisodeLog.from_buffer_copy(got_log[i, s * LOG_BYTES:(s + 1) * LOG_BYTES].tobytes())
              for s in range(LOG_SLOTS)]
        slots = [s for s in range(LOG_SLOTS)
                 if (got_log[i, s * LOG_BYTES:(s + 1) * LOG_BYTES]
                     != wl[i, s * LOG_BYTES:(s + 1) * LOG_BYTES]).any()]
        msgs.append(f"case {i} {table[i]['coords']}: state fields (name, device, model) "
                    f"{_name_state_diff(got_state[i], ws[i])}; log slots differing {slots} "
                    f"{[(s, gl[s].step, gl[s].index, gl[s].status) for s in slots]}")
    print(f"layer 1: {n} cases, model {t_model:.2f} s, total {time.perf_counter() - t0:.2f} s")
    assert not len(bad), f"{len(bad)} of {n} cases differ:\n" + "\n".join(msgs)


# ----------------------------------------------------------------------------
# layer 2
# ----------------------------------------------------------------------------
N_CAND, N_STEPS = ranking.N_CAND, 3
SENTINEL = -123.25        # what an unwritten batch entry holds


def _grid_cases():
    """(name, cfg changes, state changes, index_base, unaligned)."""
    bound = reference_episode_config().beta_bound
    wideV = dict(ratio_v=100.0, ratio_beta=100.0, delta_beta=0.05)       # |V| > 64 > |B|
    wideB = dict(ratio_v=100.0, ratio_beta=100.0, delta_v=0.02)         # |B| > 64 > |V|
    return [
        ("reference", {}, dict(v=0.3, beta=0.1), 0, False),
        ("reference enumerate", dict(enumerate=1), dict(v=0.3, beta=0.1), 0, False),
        ("four rounds, V clamped", wideV, dict(v=0.5, beta=0.0), 0, False),
        ("four rounds, V clamped, enumerate", dict(wideV, enumerate=1), dict(v=0.5, beta=0.0), 0,
         False),
        ("four rounds, B clamped", wideB, dict(v=0.5, beta=0.0), 0, False),
        ("four rounds, B clamped, odd base, unaligned", wideB, dict(v=0.5, beta=0.0), 7, True),
        # 50 x 64 = 3200 entries, looked up directly: the enumeration's padding there
        ("four rounds, B clamped, enumerate, base across the grid's end", dict(wideB, enumerate=1),
         dict(v=0.5, beta=0.0), 2701, False),
        ("four rounds, B clamped, enumerate, base past the grid, unaligned",
         dict(wideB, enumerate=1), dict(v=0.5, beta=0.0), 3200, True),
        ("v = 0", {}, dict(v=0.0, beta=0.0), 0, False),
        ("v below 0", {}, dict(v=-1e-3, beta=0.0), 0, False),
        ("v = v_max", {}, dict(v=1.0, beta=0.0), 0, False),
        ("v NaN: empty V", {}, dict(v=math.nan, beta=0.0), 0, False),
        ("v NaN: empty V, enumerate", dict(enumerate=1), dict(v=math.nan, beta=0.0), 0, False),
        ("beta = +bound", {}, dict(v=0.3, beta=bound), 0, False),
        ("beta = -bound", {}, dict(v=0.3, beta=-bound), 0, False),
        ("beta one ulp above +bound", {}, dict(v=0.3, beta=math.nextafter(bound, 9.0)), 0, False),
        ("beta one ulp below -bound", {}, dict(v=0.3, beta=-math.nextafter(bound, 9.0)), 0,
         False),
        ("empty B", {}, dict(v=0.3, beta=5.0), 0, False),
        ("empty B, enumerate", dict(enumerate=1), dict(v=0.3, beta=5.0), 0, False),
        ("slow-down, min(V) < v_min", {}, dict(v=0.3, beta=0.0, slowing=3), 0, False),
        ("slow-down, min(V) == v_min", dict(v_min=0.6 + 0.005 * (0.0 - 5.0)),
         dict(v=0.6, beta=0.0, slowing=1), 0, False),
        ("slow-down, min(V) > v_min", {}, dict(v=0.6, beta=0.0, slowing=20), 0, False),
        ("slow-down, empty V", {}, dict(v=math.nan, beta=0.0, slowing=3), 0, False),
        # a descending V: the clamp drops its smallest points, the minimum is still theirs
        ("slow-down, minimum past the clamp", dict(wideV, delta_v=-0.005),
         dict(v=0.5, beta=0.0, slowing=2), 0, False),
        ("steps_for_slowing = 0 and below", {}, dict(v=0.3, beta=0.0, slowing=-4), 0, False),
        ("odd base, pairs", {}, dict(v=0.3, beta=0.1, p=9, episodes=4), 7, False),
        ("even base, pairs", {}, dict(v=0.3, beta=0.1, p=9, episodes=4), 8, False),
        ("odd base, no pairs", {}, dict(v=0.3, beta=0.1, p=9, episodes=4), 7, True),
        ("even base, no pairs", dict(enumerate=1), dict(v=0.3, beta=0.1, p=9, episodes=4), 8,
         True),
    ]


def _grid_case_models():
    out = []
    for name, cfg_mod, st_mod, base, unaligned in _grid_cases():
        cfg = reference_episode_config(start=(0.5, -1.0, 0.3, 0.2, 0.1), target=(2.0, 3.0))
        for k, v in cfg_mod.items():
            setattr(cfg, k, v)
        M = EM.EpisodeModel(cfg)
        for k, v in st_mod.items():
            setattr(M, k, v)
        M.seed = M.seed_rule()               # as episode_prepare leaves it for this p, episode
        M.incumbent = 1e30
        M.nv, M.nb = 64, 64                  # stale grids of an earlier step
        M.grid_v, M.grid_b = [7.0 + i for i in range(64)], [-7.0 - i for i in range(64)]
        out.append((name, cfg, M, base, unaligned))
    return out


def _expected_batch(oracle, cfg, V, B, seed, base):
    """The sampled batch of mpc_episode_sample, or None where it writes none."""
    n_grid = len(V) * len(B)
    if n_grid == 0 and not cfg.enumerate:
        return None
    if n_grid:
        v, b = oracle.sample_controls(V, B, N_CAND, N_STEPS, seed, index_base=base)
    else:
        v, b = np.empty((N_STEPS, N_CAND)), np.empty((N_STEPS, N_CAND))
    if cfg.enumerate:
        pad = base + np.arange(N_CAND) >= n_grid
        v[:, pad], b[:, pad] = math.nan, 0.0
    return v, b


def test_grids_seed_and_sampled_batch_match_model(engine, oracle):
    """mpc_episode_sample (n_cand 1026, n_steps 3) on written states: nv, nb,
    grid_v[:nv], grid_b[:nb] as the model's grids() (the rest of the state
    untouched) and the batch as oracle.sample_controls on them with the
    model's seed, NaN / 0.0 padding past nv * nb under enumerate, bit for bit:
    more than one ballot round, the kEpMaxGrid clamp on either grid (a grid of
    more than 2048 entries: looked up directly, not staged), empty grids, the
    acceptance boundaries, the slow-down override below, at and above v_min
    with the minimum taken before the clamp, both index parities with and
    without the pair stores."""
    cases = _grid_case_models()
    n = len(cases)
    dev = engine.device
    lib, st = native.lib(), native.current_stream()
    states = _dev(b"".join(bytes(M.to_state()) for _, _, M, _, _ in cases), dev)
    per = N_STEPS * N_CAND + 2          # room for a view that starts 8 B in
    vb = torch.full((n, 2, per), SENTINEL, dtype=torch.float64, device=dev)
    for i, (name, cfg, M, base, unaligned) in enumerate(cases):
        off = 8 if unaligned else 0
        rc = lib.mpc_episode_sample(ctypes.byref(cfg), states.data_ptr() + i * SB,
                                    vb[i, 0].data_ptr() + off, vb[i, 1].data_ptr() + off,
                                    N_CAND, N_STEPS, base, st)
        assert rc == 0, name
    torch.cuda.synchronize()
    got_states = states.cpu().numpy().reshape(n, SB)
    got_vb = vb.cpu().numpy()
    seen = dict(rounds=0, clamped_v=0, clamped_b=0, direct=0, empty=0, pad=0)
    for i, (name, cfg, M, base, unaligned) in enumerate(cases):
        V, B, seed = M.sample()
        assert seed == M.seed, name
        want = np.frombuffer(bytes(M.to_state()), dtype=np.uint8)
        assert (got_states[i] == want).all(), (name, _name_state_diff(got_states[i], want))
        o = 1 if unaligned else 0
        got_v = got_vb[i, 0, o:o + N_STEPS * N_CAND].reshape(N_STEPS, N_CAND)
        got_b = got_vb[i, 1, o:o + N_STEPS * N_CAND].reshape(N_STEPS, N_CAND)
        exp = _expected_batch(oracle, cfg, V, B, seed, base)
        if exp is None:
            exp = (np.full_like(got_v, SENTINEL), np.full_like(got_b, SENTINEL))
        for what, g, w in (("v", got_v, exp[0]), ("beta", got_b, exp[1])):
            same = g.view(np.uint64) == np.ascontiguousarray(w).view(np.uint64)
            assert same.all(), (name, what, np.argwhere(~same)[:4].tolist())
        # nothing outside the view was written
        assert got_vb[i, :, :o].tolist() == [[SENTINEL] * o] * 2, name
        assert (got_vb[i, :, o + N_STEPS * N_CAND:] == SENTINEL).all(), name
        seen["rounds"] += 1 + 2 * int(cfg.ratio_v) > 64
        seen["clamped_v"] += len(V) == 64
        seen["clamped_b"] += len(B) == 64
        seen["direct"] += len(V) * len(B) > 2048
        seen["empty"] += len(V) * len(B) == 0
        seen["pad"] += bool(cfg.enumerate and base + N_CAND > len(V) * len(B))
    print("layer 2 (sample):", n, "cases", seen)
    assert all(seen.values()), seen


def test_generated_step_publishes_the_grids_and_updates_as_model(engine):
    """One mpc_episode_generate_step on the same written states as the sampler
    test, the wide grids included (four ballot rounds, either grid clamped to
    kEpMaxGrid, the slow-down minimum past the clamp: up to 64 x 64 entries, 64
    KiB of dynamic LDS): it publishes the model's nv / nb / grid_v / grid_b,
    and the state after it equals the model's advanced with the step's own
    `out` record as the winner row — for both an incumbent the winner beats
    and one it does not (stale), and for the empty grids (no candidate at
    all).  A cfg with enumerate is refused with MPC_ERR_UNSUPPORTED and leaves
    the state, the log and `out` as they were."""
    from diplomjourney_amd.abi import MPC_ERR_UNSUPPORTED
    cases = [(name, cfg, M, base, inc) for name, cfg, M, base, _ in _grid_case_models()
             for inc in ((1e30,) if cfg.enumerate else (1e30, 1e-30))]
    n = len(cases)
    dev = engine.device
    lib, st = native.lib(), native.current_stream()
    # (a case's model is shared by its two incumbents: the state is written per case)
    states = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
    blobs = []
    for i, (_, _, M, _, inc) in enumerate(cases):
        M.incumbent = inc
        blobs.append(bytes(M.to_state()))
        ES.write_state(states, M.to_state(), i)
    outs = torch.full((n * RESULT_BYTES,), LOG_FILL, dtype=torch.uint8, device=dev)
    logs = torch.full((n * LOG_BYTES,), LOG_FILL, dtype=torch.uint8, device=dev)
    wsb = lib.mpc_episode_generate_workspace_bytes(N_CAND, N_STEPS)
    ws = torch.zeros(n * wsb, dtype=torch.uint8, device=dev)
    for i, (name, cfg, M, base, inc) in enumerate(cases):
        integ = INTEGRATORS["rect+cum" if i % 2 else "qk21"]
        rc = lib.mpc_episode_generate_step(
            ctypes.byref(cfg), states.data_ptr() + i * SB, N_CAND, N_STEPS, base, integ,
            ws.data_ptr() + i * wsb, wsb, outs.data_ptr() + i * RESULT_BYTES,
            logs.data_ptr() + i * LOG_BYTES, 1, st)
        assert rc == (MPC_ERR_UNSUPPORTED if cfg.enumerate else 0), (name, rc)
    torch.cuda.synchronize()
    got_states = states.cpu().numpy().reshape(n, SB)
    got_outs = outs.cpu().numpy().reshape(n, RESULT_BYTES)
    got_logs = logs.cpu().numpy().reshape(n, LOG_BYTES)
    seen = dict(found=0, stale=0, none=0, refused=0, rounds=0, clamped_v=0, clamped_b=0,
                lds_64k=0)
    for i, (name, cfg, M0, base, inc) in enumerate(cases):
        if cfg.enumerate:
            assert got_states[i].tobytes() == blobs[i], name
            assert (got_outs[i] == LOG_FILL).all() and (got_logs[i] == LOG_FILL).all(), name
            seen["refused"] += 1
            continue
        M = EM.EpisodeModel.from_state(cfg, ES.EpisodeState.from_buffer_copy(blobs[i]))
        V, B, _ = M.sample()
        out = MpcResult.from_buffer_copy(got_outs[i].tobytes())
        assert out.n_steps == N_STEPS, name
        row = EM.Result(out.cost, out.index, out.n_steps, out.v, out.beta,
                        [[out.traj[s][q] for q in range(3)] for s in range(3)])
        rec = M.advance([row])
        assert out.found == rec["found"], name
        want = np.frombuffer(bytes(M.to_state()), dtype=np.uint8)
        assert (got_states[i] == want).all(), (name, inc, _name_state_diff(got_states[i], want))
        assert got_logs[i].tobytes() == bytes(EM.log_struct(rec)), (name, inc)
        seen["found"] += rec["found"]
        seen["stale"] += (not rec["found"]) and out.index >= 0
        seen["none"] += out.index < 0
        seen["rounds"] += 1 + 2 * int(cfg.ratio_v) > 64
        seen["clamped_v"] += len(V) == 64
        seen["clamped_b"] += len(B) == 64
        seen["lds_64k"] += min(64, 1 + 2 * int(cfg.ratio_v)) * min(
            64, 1 + 2 * int(cfg.ratio_beta)) * 16 >= 64 * 1024
    print("layer 2 (generated):", n, "cases", seen)
    assert all(seen.values()), seen


# ----------------------------------------------------------------------------
# layer 3
# ----------------------------------------------------------------------------
FORMS = {
    # name: (DeviceEpisode arguments, integrators)
    "two-launch": (dict(split=True), ("rect+cum", "qk21")),
    "fused": (dict(split=False), ("rect+cum", "qk21")),
    "generated": (dict(generate=True), ("rect+cum", "qk21")),
    "chained SoA": (dict(chain=True), ("rect+cum",)),
    "chained tiled": (dict(chain=True), ("rect+cum",)),
    "run": (dict(), ("rect+cum",)),
}


def _drive(engine, form, cfg, n_steps, integ):
    """STEERED_STEPS steps of a fresh device episode under cfg in one form:
    (log records, EpisodeState, chain_error)."""
    from diplomjourney_amd.episode import DeviceEpisode
    from diplomjourney_amd.expansion import soa_to_tiled
    ep = DeviceEpisode(engine, EC.STEERED_N_CAND, n_steps, integrator=integ, log_capacity=8,
                       **FORMS[form][0])
    ctypes.memmove(ctypes.addressof(ep.cfg), ctypes.addressof(cfg), ctypes.sizeof(cfg))
    ep.reset()
    batches = []
    if form != "generated":
        for j in range(EC.STEERED_STEPS):
            v, b = (torch.as_tensor(a, device=engine.device) for a in
                    EC.steered_batch(n_steps, j))
            batches.append(soa_to_tiled(v, b) if form == "chained tiled" else (v, b))
    if form == "run":
        ep.run(batches)
    else:
        for j in range(EC.STEERED_STEPS):
            ep.step(controls=batches[j] if batches else None)
            # a chained form must take the chained launch, not fall back to expand()
            assert (ep._pending is not None) == form.startswith("chained"), (form, j)
    log = ep.read_log()                   # completes a pending step; raises on a chain error
    err = ep.chain_error()
    state = ES.read_state(ep.state)
    ep.close()
    return log, state, err


@pytest.mark.parametrize("form", list(FORMS))
def test_update_through_every_caller_matches_model(engine, oracle, form):
    """From reset(), steered by the cfg alone (tests/episode_cases.py
    steered_cfgs: events in every sector of turn_target, two events on one p,
    m walking 0 -> 1 -> 2 into an arrival, a stale step without and then with
    a trajectory across a restart, stuck then break under both rules, the step
    limit; horizons 2, 3 and 10, both wheelbase forms): every log record
    equals the model's in every field, doubles by bits — the model advanced
    with the host replica's layer states and cost of the logged index — and
    after the last step the whole head, StaleTraj and EarlyPub equal the
    model's; chain_error stays 0."""
    chained = form in ("chained SoA", "chained tiled", "run")
    # a chained launch's completion of step j writes the next EarlyPub; the last
    # step is completed by the flush (or the run's end), which leaves it
    early_after = range(EC.STEERED_STEPS - 1) if chained else ()
    seen = {}
    runs = 0
    for name, cfg, n_steps in EC.steered_cfgs():
        for integ in FORMS[form][1]:
            where = f"{form}, {integ}, cfg '{name}'"
            log, state, err = _drive(engine, form, cfg, n_steps, integ)
            assert err == 0 and len(log) == EC.STEERED_STEPS, where
            M, recs, traces, _ = EC.walk(cfg, n_steps, integ, form == "generated", logged=log,
                                         early_after=early_after, oracle=oracle)
            for j, (got, want) in enumerate(zip(log, recs)):
                if bytes(got) != bytes(EM.log_struct(want)):
                    fields = {f: (getattr(got, f), want[f]) for f in EM.LOG_FIELDS
                              if bytes(type(got)(**{f: getattr(got, f)}))
                              != bytes(type(got)(**{f: want[f]}))}
                    raise AssertionError(f"{where}, step {j}: (device, model) {fields}")
            bad = [(f, getattr_path(state, f), getattr_path(M.to_state(), f))
                   for f in ES.diff(state, M.to_state())
                   if f.startswith(("h.", "st.", "early."))]
            assert not bad, f"{where}: final state (field, device, model) {bad[:12]}"
            runs += 1
            for tr in traces:
                seen[tr["status"]] = seen.get(tr["status"], 0) + 1
                for s in tr.get("sectors") or ():
                    seen[f"sector {s}"] = seen.get(f"sector {s}", 0) + 1
                seen[f"layer {tr['k']}"] = seen.get(f"layer {tr['k']}", 0) + 1
    print(f"layer 3, {form}: {runs} episodes x {EC.STEERED_STEPS} steps", seen)
    # what the cfgs are there to reach, whatever the form
    P = EM.P
    for need in (P.EVENT, P.ARRIVED, P.STALE | P.STUCK, P.STALE, P.BREAK, P.STUCK,
                 P.STUCK | P.BREAK, P.EVENT | P.LIMIT, "sector 0", "sector 1", "sector 2",
                 "sector 3", "layer 1"):
        assert seen.get(need), (need, seen)
    if form != "generated":        # (its grids do not reach far enough in three steps)
        assert seen.get("layer 2"), seen
