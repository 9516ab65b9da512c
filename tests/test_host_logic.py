"""Host-side logic of the drop-in (config, grids, CoordinateTree index
arithmetic, operator events, cost helper) against the reference's own
outputs.  CPU only."""
import math

import pytest

from diplomjourney_amd import config
from diplomjourney_amd import math_model_tree as mmt
from diplomjourney_amd.CoordinateTree import CoordinateTree


def test_config_matches_reference(units):
    for name, val in units["config"].items():
        ours = getattr(config, name)
        assert ours == val and type(ours) is type(val), name


def test_module_constants(units):
    assert mmt.radius_u_turn == units["consts_mmt"]["radius_u_turn"]


def test_first_incumbent(scenario):
    """optimal_criterion = control_criterion([x_0, y_0, phi_0]) with config's
    target (math_model_tree.py:676)."""
    mmt.reset_state()
    assert mmt.optimal_criterion == scenario["first_incumbent"] == 10000050990.195135


def test_grids_bitwise(units):
    for r in units["grids"]["velocities"]:
        assert mmt.vector_of_velocities(r["in"]) == r["out"], r["in"]
    for r in units["grids"]["betas"]:
        assert mmt.vector_of_beta_angles(r["in"]) == r["out"], r["in"]


def test_grids_from_scenario(scenario):
    """Every call's grid is the reference grid around the previous (v, beta)."""
    for rec in scenario["calls"][:151]:
        if rec["call"] == 0:
            continue
        prev = scenario["calls"][rec["call"] - 1]["ret"]
        assert mmt.vector_of_velocities(prev[3]) == rec["V"]
        assert mmt.vector_of_beta_angles(prev[4]) == rec["B"]


def test_is_on_target(units):
    for r in units["is_on_target"]:
        assert mmt.is_on_target(*r["in"]) == r["out"]


def test_host_cost(units):
    saved = (mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0)
    try:
        for r in units["costs"]:
            mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0 = r["in"][:4]
            assert mmt.control_criterion(r["in"][4:6] + [0.0]) == r["cost"]
    finally:
        mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0 = saved


@pytest.mark.parametrize("entry", range(6))
def test_coordinate_tree_index(units, entry):
    t = units["tree"][entry]
    ct = CoordinateTree(t["S1"], 3, device="cpu")
    assert ct.get_size() == t["size"]
    if "parents" in t:
        got = [ct.get_index_of_parent(j) for j in range(ct.get_size())]
        assert got == t["parents"]
    else:
        assert [ct.get_index_of_parent(j) for j in t["js"]] == t["parents_at"]


def test_coordinate_tree_size_451(units):
    ct = CoordinateTree(451, 3, device="cpu")
    assert ct.get_size() == units["tree"][-1]["size_formula"] == 91_937_703


def test_coordinate_tree_nodes_roundtrip():
    ct = CoordinateTree(4, 3, device="cpu")
    assert ct[0] is None and ct[4 + 3] is None          # unwritten slots read None
    ct[4 + 2] = [1.0, 2.0, 0.5, 0.3, -0.1]               # layer 1, node 2
    assert ct[6] == [1.0, 2.0, 0.5, 0.3, -0.1]
    assert ct[4 + 16 + 5] is None                        # layer 2, never-used node
    with pytest.raises(IndexError):
        ct[4 + 16 + 5] = [0, 0, 0, 0, 0]
    ct.clear()
    assert ct[6] is None
    assert ct.get_index_of_parent(4 + 16 + 2) == [4 + 2, 2]


def test_coordinate_tree_deeper_horizon():
    ct = CoordinateTree(3, 5, device="cpu")
    assert ct.get_size() == 3 + 9 + 27 + 81 + 243
    j = ct.offsets[4] + 1                                 # layer 4, node 1
    assert ct.get_index_of_parent(j) == [ct.offsets[3] + 1, ct.offsets[2] + 1,
                                         ct.offsets[1] + 1, 1]


def test_operator_events(scenario):
    """turn_right (p=60), turn_left (p=90), new_target (p=110) targets and
    the globals they set (math_model_tree.py:118-226, :564-569, :617-624)."""
    calls = scenario["calls"]
    for ev in scenario["events"]:
        ax, ay, aphi, tx, ty, av = ev["args"]
        ret = calls[ev["after_call"]]["ret"]
        assert (ax, ay, aphi) == tuple(ret[:3])
        if ev["p"] == 60:
            assert mmt._turn_target(ax, ay, aphi, 2, -1) == (tx, ty)
        elif ev["p"] == 90:
            assert mmt._turn_target(ax, ay, aphi, 2, +1) == (tx, ty)
        else:
            assert (tx, ty) == (2, 3)
        mmt.reset_state()
        mmt.x_t, mmt.y_t = ev["pre"]["x_t"], ev["pre"]["y_t"]
        mmt.new_target(ax, ay, aphi, tx, ty, av)
        post = ev["post"]
        assert (mmt.x_t, mmt.y_t, mmt.x_0, mmt.y_0) == (post["x_t"], post["y_t"], post["x_0"],
                                                         post["y_0"])
        assert mmt.steps_for_slowing == 10     # slow_down(radians(30)) in new_target
    mmt.reset_state()


def test_slow_down_bands():
    for deg, want in ((5, 0), (30, 10), (45, 10), (60, 20), (90, 20)):
        mmt.slow_down(math.radians(deg))
        assert mmt.steps_for_slowing == want
    mmt.reset_state()


def test_candidate_enumeration_order():
    """k = a*|B| + b: v outer, beta inner (math_model_tree.py:311-317)."""
    v_sc, b_sc = mmt.candidate_controls([0.1, 0.2], [-1.0, 0.0, 1.0], 3, "cpu")
    assert v_sc.shape == (3, 6)
    assert v_sc[0].tolist() == [0.1, 0.1, 0.1, 0.2, 0.2, 0.2]
    assert b_sc[2].tolist() == [-1.0, 0.0, 1.0, -1.0, 0.0, 1.0]


def test_bench_defaults(monkeypatch):
    """bench.py's defaults: config C on one GPU, the chained rect+cum step for
    the episode workloads (B, C, D), rect+rot for E/F/G, 500 timed steps for
    the ~40-us workloads."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    def parse(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()

    a = parse()
    assert (a.workload, a.gpus, a.steps, a.warmup, a.integrator, a.inputs) == (
        "C", 1, 500, 20, "rect+cum", "resident")
    assert not a.no_chain
    assert parse("--workload", "D").integrator == "rect+cum"
    assert parse("--workload", "B").integrator == "rect+cum"
    assert parse("--workload", "E").integrator == "rect+rot"
    f = parse("--workload", "F")
    assert (f.integrator, f.steps) == ("rect+rot", 50)
    assert parse("--integrator", "qk21").integrator == "qk21"
    assert parse("--inputs", "generated").inputs == "generated"
    # a plain run times the steps only; --full adds every other measurement
    assert a.full is False and a.dump_outputs is None
    assert parse("--full").full is True
    assert parse("--dump-outputs", "out").dump_outputs == "out"


def test_bench_episode_outputs(tmp_path):
    """--dump-outputs: the timed steps' log records (the K before the
    snapshot's step count, whatever older steps the ring still holds) and the
    winner record become float64 .npy arrays."""
    import ctypes
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from diplomjourney_amd.abi import MpcEpisodeLog, MpcResult
    cap, k, ns = 8, 3, 4
    ring = (MpcEpisodeLog * cap)()
    for step in (0, 1, 2, 3, 4, 5, 14, 15):      # 14, 15: left by an earlier, longer run
        ring[step % cap] = MpcEpisodeLog(step, 100 + step, step + 1, 1, 1, 0, 0.5 * step,
                                         1.0 * step, 2.0 * step, 3.0 * step, 0.25, -0.5)
    w = MpcResult(cost=2.5, index=105, found=1, n_steps=ns, v=0.25, beta=-0.5)
    for s in range(ns):
        for c in range(3):
            w.traj[s][c] = 10.0 * s + c
    snap = {"steps_enqueued": 6, "log": bytes(ring), "winner": bytes(w)}
    out = bench.episode_outputs(snap, k, ns)
    assert out["step_index"].tolist() == [103, 104, 105]
    assert out["step_cost"].tolist() == [1.5, 2.0, 2.5]
    assert out["step_state"].tolist() == [[s, 2 * s, 3 * s, 0.25, -0.5] for s in (3.0, 4.0, 5.0)]
    assert out["step_status"].tolist() == [[s, s + 1, 1, 1, 0] for s in (3, 4, 5)]
    assert out["winner_index"] == [105] and out["winner_control"] == [0.25, -0.5]
    assert out["winner_trajectory"] == [[10.0 * s + c for c in range(3)] for s in range(ns)]
    # more timed steps than the ring holds: the last `cap` of them
    full = (MpcEpisodeLog * cap)()
    for step in range(12, 20):
        full[step % cap] = MpcEpisodeLog(step, step, 1, 1, 1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    many = bench.episode_outputs({"steps_enqueued": 20, "log": bytes(full), "winner": None},
                                 16, ns)
    assert many["step_index"].tolist() == list(range(12, 20)) and "winner_index" not in many
    bench.dump_outputs(str(tmp_path / "d"), out)
    got = {f: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == sorted(n + ".npy" for n in out)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["winner_trajectory.npy"].shape == (ns, 3)
    assert got["step_index.npy"].tolist() == [103.0, 104.0, 105.0]


def _bench(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK")):
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(repo, "bench.py"), *args], env=env,
                          capture_output=True, text=True, timeout=120, cwd=repo)


def test_bench_gpus_world_size_mismatch_fails():
    """Under a launcher, --gpus must equal WORLD_SIZE: a mismatch exits 2
    before any GPU or CPU-baseline work instead of running a mislabelled line."""
    r = _bench(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr, r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    r = _bench(["--gpus", "1"], {"WORLD_SIZE": "8", "RANK": "3", "LOCAL_RANK": "3"})
    assert r.returncode == 2


def test_bench_gpus_spawns_one_process_per_rank():
    """`python bench.py --gpus N` without a launcher starts N rank processes
    of itself with RANK / LOCAL_RANK / WORLD_SIZE and one shared
    MASTER_ADDR 127.0.0.1:port (the launcher self-test prints each rank's view
    instead of running GPU work)."""
    import json
    r = _bench(["--gpus", "3", "--dist-backend", "gloo", "--print-ranks"])
    assert r.returncode == 0, r.stderr
    ranks = sorted((json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")),
                   key=lambda d: d["rank"])
    assert [d["rank"] for d in ranks] == [0, 1, 2]
    assert all(d["world"] == 3 and d["local_rank"] == d["rank"] for d in ranks)
    assert len({tuple(d["master"]) for d in ranks}) == 1 and ranks[0]["master"][0] == "127.0.0.1"


def test_bench_spawned_rank_failure_fails_the_run():
    """A failing rank fails the spawned run with its status (here every rank
    rejects an inconsistent launch), and no JSON line is printed."""
    r = _bench(["--gpus", "2", "--dist-backend", "gloo", "--print-ranks"],
               {"WORLD_SIZE": "2"}, drop=("RANK", "LOCAL_RANK"))
    assert r.returncode == 0          # under a launcher: WORLD_SIZE matches, no spawn
    r = _bench(["--gpus", "2", "--dist-backend", "gloo", "--workload", "C", "--steps", "4",
                "--cpu-seconds", "0"], {"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
