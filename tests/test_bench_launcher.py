"""bench.py's N > 1 control flow, on CPU: `python bench.py --gpus 2` must start two ranks ITSELF, print one JSON line
with n_gpus == 2, or fail loudly and quickly.  The ranks talk over gloo; tests/bench_stub.py stands in for the device
world (no GPU, no RCCL here), so this covers what a 1-GPU box cannot: the launcher, the unique-id broadcast, the
agreed fallback to torch.distributed when one rank cannot bring the native collective up, the schedule trial, the
deadlines.  (VERDICT r01, next #1.)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(extra_args, extra_env=None, timeout=240, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(BGE_BENCH_STUB="1", **(extra_env or {}))
    t0 = time.time()
    p = subprocess.run([sys.executable, BENCH, "--steps", "5", "--warmup", "2", "--entities", "6400", "--no-cpu"] + extra_args,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode(), time.time() - t0


def test_gpus_2_starts_two_ranks_and_reports_them():
    rc, out, err, _ = _run(["--gpus", "2", "--deadline", "90", "--full"])
    assert rc == 0, err[-2000:]
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out  # exactly ONE line on stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2
    assert line["config"]["entities_per_gpu"] == 6400 and "x 2 GPU" in line["config"]["workload"]
    assert line["config"]["workload"].startswith("subtree64")  # configs[4] is the N > 1 workload
    assert "native RCCL gather" in line["config"]["collective"]  # both ranks brought the (stub) native collective up
    assert set(line["config"]["gather_schedule_trials_ms"]) == {"0", "1"}  # both schedules were tried on every rank
    assert "STUB" in line["data"] and line["value"] == 0.0  # a stub run can never pass for a measurement
    # every N > 1 line carries its own single-GPU anchor on the SAME workload and the median-of-R timing
    solo = line["single_gpu_same_workload"]
    assert solo["unit"] == "entity-updates/s" and "6400 entities, subtree64" in solo["what"] and "before the communicator" in solo["what"]
    assert solo["ms_per_step"] > 0 and solo["kernel_ms_per_launch"] > 0 and solo["ms_per_step_slowest_rank"] >= solo["ms_per_step"] * 0.0
    assert "scaling_efficiency" in line                                  # (None in a stub run: nothing was measured)
    assert line["compute_only_ms_per_step"] > 0 and line["compute_plus_collective_ms_per_step"] > 0
    assert line["repeats"] == 5 and len(line["region_ms"]) == 5 and "median of 5" in line["timing"]
    assert abs(line["ms_per_step"] - sorted(line["region_ms"])[2] / 5) < 1e-9    # the median region / K


def test_a_plain_run_times_exactly_steps_and_dumps_its_outputs(tmp_path):
    import numpy as np
    rc, out, err, _ = _run(["--gpus", "1", "--dump-outputs", str(tmp_path)])
    assert rc == 0, err[-2000:]
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["warmup"] == 2
    assert line["repeats"] == 1 and len(line["region_ms"]) == 1            # one region of exactly --steps steps
    assert abs(line["ms_per_step"] - line["region_ms"][0] / 5) < 1e-9
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert "configs" not in line and "cpu_baseline" not in line and "parity" not in line
    shapes = {"world": (6400, 16), "position": (6400, 3), "rotation_euler": (6400, 3), "linvel": (6400, 3), "entity_id": (6400,)}
    total = 0
    for name, shape in shapes.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.shape == shape and a.dtype in (np.float32, np.float64), (name, a.shape, a.dtype)
        total += a.nbytes
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "entity_id.npy"), np.arange(6400, dtype=np.float64))


def test_dump_sample_is_seeded_and_bounded(tmp_path):
    """A shard larger than DUMP_SAMPLE: the same sorted sample of entity ids in every run, under 64 MB in all."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import bench
    from bench_stub import StubWorld

    class Wl:
        n = 3 * bench.DUMP_SAMPLE
    picks = []
    for k in range(2):
        w = StubWorld()
        w.load(Wl)
        d = tmp_path / str(k)
        bench.dump_outputs(w, str(d), 100, chunk=bench.DUMP_SAMPLE)
        picks.append(np.load(d / "entity_id.npy"))
        assert len(picks[-1]) == bench.DUMP_SAMPLE and np.load(d / "world.npy").shape == (bench.DUMP_SAMPLE, 16)
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    assert np.array_equal(picks[0], picks[1]) and np.all(np.diff(picks[0]) > 0)
    assert picks[0][0] >= 100 and picks[0][-1] < 100 + Wl.n


def test_default_deadline_keeps_the_launcher_inside_the_drivers_limit():
    sys.path.insert(0, ROOT)
    import bench
    assert 3 * bench.parse_args([]).deadline < 600


def test_one_rank_without_the_native_collective_makes_every_rank_fall_back():
    rc, out, err, _ = _run(["--gpus", "2", "--deadline", "90"], {"BGE_BENCH_STUB_FAIL_INIT_RANK": "1"})
    assert rc == 0, err[-2000:]
    line = json.loads(out.strip().splitlines()[-1])
    assert line["n_gpus"] == 2
    assert "torch.distributed.all_gather_into_tensor" in line["config"]["collective"]
    assert "native RCCL init failed" in err and "using torch.distributed for the root gather on every rank" in err


def test_a_hung_rank_fails_the_job_fast_and_names_the_phase():
    rc, out, err, took = _run(["--gpus", "2", "--deadline", "8"], {"BGE_BENCH_STUB_HANG_RANK": "1"}, timeout=120)
    assert rc != 0
    assert out.strip() == ""  # no result line
    assert "DEADLINE" in err and "still in '" in err
    assert "[bench launcher]" in err and "stopping all 2 ranks" in err
    assert took < 60, f"took {took:.0f} s"


def test_world_size_that_disagrees_with_gpus_is_refused():
    rc, out, err, _ = _run(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0"}, drop=())
    assert rc == 2 and out.strip() == ""
    assert "refusing to run" in err


def test_a_failing_child_fails_the_launcher():
    rc, out, err, _ = _run(["--gpus", "2", "--workload", "no_such_workload"])
    assert rc != 0 and out.strip() == ""
    assert "[bench launcher]" in err
