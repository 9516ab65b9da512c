"""The episode model of the GPU update tests (tests/episode_model.py) and its
case table (tests/episode_cases.py) checked on the CPU: the state mirrors
against the compiler's layout, the model against the reference's recorded
model run and against oracle.parity's two episode oracles, its turn_target
against the drop-in's, and the coverage the case table must reach before the
GPU test (tests/test_episode_update_gpu.py) means anything."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import call_problem

import episode_cases as EC
import episode_model as EM
import episode_state as ES


@pytest.fixture(scope="module")
def P(oracle):
    from oracle import parity
    return parity


def _enumerate(V, B, n_steps=3):
    vv = np.repeat(np.array(V, dtype=np.float64), len(B))
    bb = np.tile(np.array(B, dtype=np.float64), len(V))
    return np.tile(vv, (n_steps, 1)), np.tile(bb, (n_steps, 1))


def test_state_mirrors_match_the_compilers_layout():
    """sizeof of the five structs, offsetof of every named field, kEpMaxGrid,
    kPubWords and kStoredWords: the ctypes mirrors against the host build."""
    assert ES.check_layout() == 72
    assert ES.state_bytes() % 128 == 0
    assert ES.EpisodeState.early.offset == 8 * ES.STORED_WORDS


def test_state_round_trip_through_the_mirror():
    from diplomjourney_amd.episode import reference_episode_config
    M = EC.build_case(1, "found1", 1, 3, np.random.default_rng(1))["model"]
    S = M.to_state()
    back = EM.EpisodeModel.from_state(reference_episode_config(), S).to_state()
    assert bytes(back) == bytes(S) and ES.diff(back, S) == []
    S.h.K.inv_den = math.nextafter(S.h.K.inv_den, 2.0)
    S.grid_b[63] = -S.grid_b[63]
    assert ES.diff(S, back) == ["h.K.inv_den", "grid_b[63]"]


def test_model_replays_reference_model_run_as_the_oracle_episode_does(scenario, P):
    """With libm's sin / cos switched in and the reference's config, the model
    passes the golden checks of tests/test_parity_oracle.py on the 151-call
    model run — grids, problem, incumbent, returned state, events, arrival —
    and every one of its records equals OracleMpcEpisode's."""
    from diplomjourney_amd.episode import reference_episode_config
    cfg = reference_episode_config(incumbent0=scenario["first_incumbent"])
    me = EM.EpisodeModel(cfg, sincos=EM.libm_sincos)
    oe = P.OracleMpcEpisode(cfg)
    calls = [c for c in scenario["calls"] if not c["isActual"]][:151]
    assert len(calls) == 151
    events = []
    with ThreadPoolExecutor(max_workers=1) as ex:
        for i, rec in enumerate(calls):
            V, B, seed = me.grids()
            assert (V, B, seed) == oe.grids(), i
            pre = rec["pre"]
            want_V = list(rec["V"])
            if pre["steps_for_slowing"] > 0:
                want_V = [min(want_V) if min(want_V) > 0.4 else 0.4] * len(want_V)
            assert (V, B) == (want_V, list(rec["B"])), i
            prob, inc = me.begin_step()
            oprob, oinc = oe.begin_step()
            assert prob.as_tuple() == call_problem(rec).as_tuple() == oprob.as_tuple(), i
            assert inc == float(pre["optimal_criterion"]) == oinc, i
            assert me.seed == seed and me.step == i
            v, b = _enumerate(V, B)
            row = P.ShardScanner(v, b, 0, 1).scan(ex, prob)
            got, want = me.advance(row, inc), oe.advance(row, oinc)
            assert {k: got[k] for k in want} == want, i
            assert [got[k] for k in ("x", "y", "phi", "v", "beta")] == rec["ret"], i
            if got["status"] & P.EVENT:
                events.append(got["p"])
            assert bool(got["status"] & P.ARRIVED) == (i == 150), i
    assert events == [60, 90, 110]
    assert me.episodes == 2 and me.p == 1 and me.step == 151


# (x_0, y_0, phi_0, x_t, y_t) of an episode that tree_episodes_oracle ends with
# "recursive_error": the target lies behind a robot that starts at rest
STUCK_START = (0.0, 0.0, 0.0, -2.0, 0.0)


def _model_tree_episode(O, start, max_calls):
    """run_math_model.py's loop over the model with cfg.stop_rule 1, as
    oracle.parity.tree_episodes_oracle runs it."""
    from diplomjourney_amd.episode import tree_episode_config
    cfg = tree_episode_config(start)
    M = EM.EpisodeModel(cfg, sincos=EM.libm_sincos)
    recs = []
    if not M.pose_ok(M.x, M.y):           # the loop head's on-target test (:241)
        return recs, "on_target"
    while True:
        if len(recs) == max_calls:
            return recs, "max_calls"
        V, B, _ = M.grids()
        vs, bs = _enumerate(V, B)
        prob, inc = M.begin_step()
        r = O.rollout_argmin(prob, vs, bs, incumbent=inc)[0]
        if not r.found and not M.has_traj:
            return recs, "no_traj"
        row = EM.Result(r.cost, r.index, 3, r.v, r.beta, [list(r.traj[q][:3]) for q in range(3)])
        got = M.advance([row])
        recs.append([got[k] for k in ("x", "y", "phi", "v", "beta")])
        if got["status"] & EM.P.BREAK:
            assert got["status"] & EM.P.STUCK
            return recs, "recursive_error"
        if got["status"] & EM.P.ARRIVED:
            return recs, "on_target"


def test_stop_rule_1_matches_tree_episodes_oracle(P, oracle):
    """cfg.stop_rule 1 (run_math_model.py:266-272: `recursive` counts, the
    second non-moving step ends the episode) against tree_episodes_oracle: the
    scenario's 60-call prefix, and a start whose episode the rule ends."""
    starts = [(0.0, 0.0, 0.0, 2.0, 3.0), STUCK_START]
    want = P.tree_episodes_oracle(starts, 60, 1)
    assert want[0][1] == "max_calls" and want[1][1] == "recursive_error"
    for s, (recs, stop) in zip(starts, want):
        got, gstop = _model_tree_episode(oracle, s, 60)
        assert gstop == stop and got == recs, s


def test_turn_target_equals_the_drop_ins_over_all_sectors():
    """The model's turn_target (device sin / cos) against
    math_model_tree._turn_target (libm): within 4 ulp of |x| + |d| + |R| —
    each trig is faithful (< 1 ulp), each of the two products adds half an ulp
    of a term, each of the two sums half an ulp of a partial sum; sectors by
    interior points and by their boundaries."""
    from diplomjourney_amd import math_model_tree as mmt
    pi = math.pi
    seen = set()
    phis = [2.0, 3.0, 4.0, 4.5, 5.5, 6.0, 7.0, 0.5, -0.75, 1.0, pi / 2, pi, 3 * pi / 2, 2 * pi,
            math.nextafter(pi / 2, 0.0), math.nextafter(3 * pi / 2, 9.0),
            math.nextafter(2 * pi, 9.0), math.nextafter(pi, 9.0)]
    for phi in phis:
        for sign in (-1.0, 1.0):
            for ax, ay, d in ((0.0, 0.0, 2.0), (1.5, -2.25, 2.0), (-30.0, 12.0, 0.25)):
                (tx, ty), sector = EM.turn_target(ax, ay, phi, d, mmt.radius_u_turn, sign,
                                                  EM.device_sincos)
                (lx, ly), lsector = EM.turn_target(ax, ay, phi, d, mmt.radius_u_turn, sign,
                                                   EM.libm_sincos)
                wx, wy = mmt._turn_target(ax, ay, phi, d, int(sign))
                assert (lx, ly) == (wx, wy) and sector == lsector
                seen.add(sector)
                for got, want, a in ((tx, wx, ax), (ty, wy, ay)):
                    bound = 4 * math.ulp(abs(a) + d + mmt.radius_u_turn)
                    assert abs(got - want) <= bound, (phi, sign, ax, ay, d)
    assert seen == {0, 1, 2, 3}
    sector_of = {phi: EM.turn_target(0.0, 0.0, phi, 2.0, 1.0, 1.0, EM.libm_sincos)[1]
                 for phi in phis}
    assert [sector_of[q] for q in (pi / 2, pi, 3 * pi / 2, 2 * pi)] == [0, 0, 1, 2]
    assert sector_of[math.nextafter(pi / 2, 0.0)] == 2 and sector_of[-0.75] == 2
    assert sector_of[math.nextafter(2 * pi, 9.0)] == 3 and sector_of[0.5] == 2


def test_selection_follows_select_index():
    R = EM.Result
    t = [[0.0, 0.0, 0.0]]
    assert EM.select([R(5.0, -1, 1, 0, 0, t), R(3.0, -1, 1, 0, 0, t)]) == (0, False)
    assert EM.select([R(1.0, -1, 1, 0, 0, t), R(9.0, 4, 1, 0, 0, t)]) == (1, True)
    assert EM.select([R(2.0, 7, 1, 0, 0, t), R(2.0, 3, 1, 0, 0, t)]) == (1, True)
    assert EM.select([R(math.nan, 4, 1, 0, 0, t), R(math.inf, 2, 1, 0, 0, t)]) == (1, False)
    assert EM.select([R(math.nan, 0, 1, 0, 0, t), R(0.0, 9, 1, 0, 0, t),
                      R(-0.0, 8, 1, 0, 0, t)]) == (2, True)


@pytest.fixture(scope="module")
def table():
    return EC.case_table()


def test_case_table_reaches_every_outcome(table, P):
    """The preconditions of the GPU test: run by the model alone, the table
    produces every status bit, every status word the code can produce, every
    turn_target sector, every finishing layer, every m transition, every
    restart cause and every log-ring form at least 8 times, and all 12
    (m, found, has_traj) combinations; at most about 4000 launches."""
    assert 3000 <= len(table) <= 4000
    cov = EC.coverage(table)
    print({k: dict(sorted(v.items(), key=str)) for k, v in cov.items()})
    need = {"bit": [P.STALE, P.STUCK, P.BREAK, P.EVENT, P.ARRIVED, P.LIMIT],
            "status": EC.possible_statuses(),
            "sector": [0, 1, 2, 3],
            "layer": [0, 1, 2],
            "m_transition": [(0, 0), (0, 1), (1, 2), (2, 2)],
            "restart": ["break", "stuck_break", "arrived", "limit"],
            "m_found_traj": [(m, f, h) for m in (0, 1, 2) for f in (0, 1) for h in (0, 1)],
            "log_slot": [("cap1", 0), ("cap3", 0), ("cap3", 1), ("cap3", 2), ("null", 2),
                         ("cap0", None)]}
    assert len(need["status"]) == 28 and len(need["m_found_traj"]) == 12
    short = {(kind, key): cov[kind][key] for kind, keys in need.items() for key in keys
             if cov[kind][key] < 8}
    assert not short, short
    assert set(cov["status"]) <= set(need["status"])


def test_steered_cfgs_reach_their_branches_in_a_dry_run(oracle, P):
    """The layer-3 cfgs walked by the model over the host replica alone (the
    host's quotient in place of the device's reciprocal estimate): within six
    steps of a reset they fire events in every sector of turn_target, put two
    events on one p, walk m 0 -> 1 -> 2 into an arrival, take a stale step
    without and then with a trajectory across a restart, get stuck and break
    under both rules, and hit the step limit."""
    seen, finishing = set(), set()
    for name, cfg, n_steps in EC.steered_cfgs():
        M, recs, traces, _ = EC.walk(cfg, n_steps, "rect+cum", False)
        assert M.step == EC.STEERED_STEPS
        for tr in traces:
            seen.add(tr["status"])
            seen.update(f"sector {s}" for s in tr.get("sectors") or ())
            finishing.add((tr["m0"], tr["m1"], tr["k"]))
        if name.startswith("two events"):
            assert traces[0]["sectors"] == [3] and recs[0]["status"] == P.EVENT
        if name.startswith("stale"):
            assert [r["status"] for r in recs[:3]] == [P.STALE | P.STUCK, P.BREAK, P.STALE]
            assert [t["had_traj"] for t in traces[:3]] == [0, 0, 1]
    assert seen >= {P.EVENT, P.ARRIVED, P.STALE | P.STUCK, P.STALE, P.BREAK, P.STUCK,
                    P.STUCK | P.BREAK, P.EVENT | P.LIMIT, "sector 0", "sector 1", "sector 2",
                    "sector 3"}, seen
    assert finishing >= {(0, 0, 0), (0, 1, 0), (1, 2, 1), (2, 2, 2)}, finishing


def test_case_table_axes_all_occur(table):
    """Every value of every axis is in the table, the boundary probes decide
    as intended, and both restart incumbents are taken."""
    from collections import Counter
    seen = Counter((k, v) for c in table for k, v in c["coords"].items())
    axes = dict(m=EC.M_VALUES, winner=EC.WINNERS, has_traj=EC.HAS_TRAJ, n_steps=EC.N_STEPS,
                probe=EC.PROBES, stuck=EC.STUCK, event=EC.EVENTS,
                heading=[h for h, _ in EC.HEADINGS], end=EC.ENDS, restart=EC.RESTARTS,
                log=EC.LOGS, L=EC.WHEELBASES)
    short = {(k, v): seen[(k, v)] for k, vals in axes.items() for v in vals if seen[(k, v)] < 8}
    assert not short, short
    probes = Counter()
    origin = given = 0
    for c in table:
        co = c["coords"]
        M, rec, tr = EC.run_model(c)
        # the probe decides m for m == 0 whenever layer 2 is another layer than the returned one
        if co["m"] == 0 and (co["winner"] in EC.FOUND_WINNERS and co["n_steps"] >= 3
                             or co["winner"] not in EC.FOUND_WINNERS and co["has_traj"]):
            probes[(co["probe"], tr["m1"])] += 1
        if tr["ended"]:
            origin += co["restart"] == "origin" and M.incumbent != 12345.5
            given += co["restart"] == "given" and M.incumbent == 12345.5
    assert set(probes) == {("far", 0), ("inside", 1), ("exact", 1), ("above", 0)}, probes
    assert min(probes.values()) >= 8 and origin >= 8 and given >= 8
