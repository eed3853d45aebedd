"""bench.py's own multi-GPU launch (`--gpus N` without torch.distributed.run): the launch plan, the
WORLD_SIZE mismatch exit and the child processes, on CPU (no GPU call is made by any of these), and
the two tests marked gpu: what a plain run and a --full run print and dump."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(kw)
    return e


def test_launch_plan_one_gpu_runs_in_process():
    assert bench.launch_plan(1, _env()) is None


def test_launch_plan_spawns_one_rank_per_gpu():
    plan = bench.launch_plan(4, _env(), port=29517)
    assert [p["RANK"] for p in plan] == ["0", "1", "2", "3"]
    assert [p["LOCAL_RANK"] for p in plan] == ["0", "1", "2", "3"]
    assert all(p["WORLD_SIZE"] == "4" and p["MASTER_ADDR"] == "127.0.0.1" and p["MASTER_PORT"] == "29517"
               for p in plan)


def test_launch_plan_defers_to_a_matching_launcher():
    assert bench.launch_plan(8, _env(WORLD_SIZE="8", RANK="3", LOCAL_RANK="3")) is None


@pytest.mark.parametrize("gpus,ws", [(8, "1"), (2, "4"), (1, "2")])
def test_launch_plan_rejects_a_mismatched_world(gpus, ws):
    with pytest.raises(bench.LaunchError):
        bench.launch_plan(gpus, _env(WORLD_SIZE=ws))


def test_mismatch_exits_nonzero_before_any_gpu_work():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=_env(WORLD_SIZE="3"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "disagrees" in r.stderr


def test_spawned_ranks_run_and_exit_cleanly():
    # every child gets WORLD_SIZE=2, so it runs main() itself: --help exits 0 before touching torch
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--help"],
                       env=_env(TCI_BENCH_DEVICES="2"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("usage:") == 2


def test_a_failing_rank_fails_the_launch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-such-flag"],
                       env=_env(TCI_BENCH_DEVICES="2"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0


@pytest.mark.parametrize("gpus,visible,rehearsal,ok", [(8, 8, False, True), (8, 7, False, False), (2, 1, False, False),
                                                       (2, 1, True, True), (1, 0, False, False)])
def test_device_count_check(gpus, visible, rehearsal, ok):
    if ok:
        bench.check_devices(gpus, visible, rehearsal)
    else:
        with pytest.raises(bench.LaunchError):
            bench.check_devices(gpus, visible, rehearsal)


def test_too_few_devices_refused_before_any_rank_starts():
    # the parent counts devices (torch.cuda.device_count(): no HIP context) and exits 2; no child runs
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=_env(TCI_BENCH_DEVICES="4"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "needs 8 visible GPU(s), found 4" in r.stderr
    assert "usage:" not in r.stdout


def test_no_gpu_refused_for_one_rank():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=_env(TCI_BENCH_DEVICES="0"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "needs 1 visible GPU(s), found 0" in r.stderr


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (0, 8), (1, 2), (3, 8)])
def test_cpu_baseline_is_in_the_line_at_every_world_size(monkeypatch, rank, world):
    """the CPU baseline legs run on rank 0 at any world size (not only N = 1), so
    every line of a 1/2/4/8-GPU scaling run carries `cpu_baseline` next to the GPU numbers; other
    ranks skip them. The legs themselves are stubbed here (the real ones are exercised on the GPU box)."""
    from types import SimpleNamespace

    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: {"value": 1.0, "unit": "SS evals/s"})
    monkeypatch.setattr(bench, "cpu_fit_config1", lambda *a, **k: {"value": 2.0})
    monkeypatch.setattr(bench, "cpu_baseline_synth", lambda cfg, *a, **k: {"value": float(cfg)})

    class C:
        n_cells = 3

    res = {}
    bench.cpu_legs(res, rank, world, SimpleNamespace(no_cpu_baseline=False, proposals=4, cpu_seconds=1.0), C(),
                   None, None, None, {4: {}, 5: {}})
    if rank == 0:
        assert set(res) == {"cpu_baseline", "cpu_fit_config1", "cpu_baseline_config4", "cpu_baseline_config5"}
        assert res["cpu_baseline"]["host"]["ranks_on_this_host"] == world
    else:
        assert res == {}
    res = {}
    bench.cpu_legs(res, rank, world, SimpleNamespace(no_cpu_baseline=True, proposals=4, cpu_seconds=1.0), C(),
                   None, None, None, {})
    assert res == {}


def test_dump_outputs_writes_float64_and_samples_past_64_mb(tmp_path):
    """--dump-outputs: DIR/ss.npy holds the SS as float64 with 0 on the skipped rows (the kernel's +Inf
    mark there is not a result), DIR/in_bounds.npy the mask as float32; an in-bounds row is written as
    it came, so a wrong Inf or NaN there still shows; per-rank names with several ranks; arrays past
    64 MB in all are cut to a fixed sample of the rows, the same at every call."""
    import numpy as np

    ss, act = np.array([1.5, np.inf, 3.0, np.inf, np.nan]), np.array([1, 0, 1, 1, 1], np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), ss, act, 0, 1)
    got, m = np.load(tmp_path / "a" / "ss.npy"), np.load(tmp_path / "a" / "in_bounds.npy")
    assert got.dtype == np.float64 and m.dtype == np.float32
    assert got.tobytes() == np.array([1.5, 0.0, 3.0, np.inf, np.nan]).tobytes() and m.tolist() == [1, 0, 1, 1, 1]
    bench.dump_outputs(str(tmp_path / "a"), ss, act, 1, 2)
    assert (tmp_path / "a" / "ss_rank1.npy").exists() and (tmp_path / "a" / "in_bounds_rank1.npy").exists()
    big = np.arange(1.0, 5_500_001.0)
    keep = np.arange(big.size) % 3 != 0
    bench.dump_outputs(str(tmp_path / "b"), big, keep, 0, 1)
    bench.dump_outputs(str(tmp_path / "c"), big, keep, 0, 1)
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in ("ss.npy", "in_bounds.npy")) <= 64_000_000
    b, mb = np.load(tmp_path / "b" / "ss.npy"), np.load(tmp_path / "b" / "in_bounds.npy")
    assert b.shape == mb.shape and np.all(np.diff(b[mb == 1]) > 0) and np.all(b[mb == 0] == 0)
    assert np.all((b[mb == 1] - 1) % 3 != 0)                      # mask and values are cut at the same rows
    assert np.array_equal(b, np.load(tmp_path / "c" / "ss.npy"))


PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "results_finite"}


def _run_bench(dump_dir, *extra):
    """One short benchmark process (3 steps, 1 warm-up): its JSON line and the two arrays it dumped."""
    import json

    import numpy as np

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(dump_dir), *extra], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(dump_dir)) == ["in_bounds.npy", "ss.npy"]
    return (json.loads(r.stdout.strip().splitlines()[-1]), np.load(os.path.join(dump_dir, "ss.npy")),
            np.load(os.path.join(dump_dir, "in_bounds.npy")))


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _run_bench(tmp_path_factory.mktemp("plain"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_launch(plain_run):
    """A plain run prints the headline line only (every other leg is behind --full), times exactly
    --steps steps, and --dump-outputs writes the last timed launch's SS: one float64 per row, every one
    finite, positive on the in-bounds rows and 0 on the skipped ones, beside the mask as float32."""
    import numpy as np

    d, a, m = plain_run
    assert set(d) == PLAIN_KEYS
    assert d["steps"] == 3 and d["warmup"] == 1 and d["results_finite"]
    assert d["ms_per_step"] == pytest.approx(d["config"]["timed_region_s"] * 1e3 / 3)
    assert a.dtype == np.float64 and a.shape == (d["config"]["rows_per_launch_per_gpu"],)
    assert m.dtype == np.float32 and m.shape == a.shape and set(np.unique(m)) == {0.0, 1.0}
    assert np.all(np.isfinite(a)) and np.all(a[m == 1] > 0) and np.all(a[m == 0] == 0)


@pytest.mark.gpu
def test_full_adds_the_other_legs_to_the_same_line(plain_run, tmp_path):
    """--full keeps the headline keys and adds the legs its options leave on (here the kernel sweep and
    the drop-in latency; the fits, configs and CPU baselines are switched off to keep the test short).
    The timed steps are the same ones: a second process with the same arguments dumps the same bits."""
    d, a, m = _run_bench(tmp_path, "--full", "--no-cpu-baseline", "--dram-steps", "0", "--no-configs")
    assert set(d) == PLAIN_KEYS | {"kernel_sweep", "kernel_x0_theta", "drop_in_latency", "host_api_pcie_inclusive"}
    assert [s["K"] for s in d["kernel_sweep"]] == [1, 64, 256, 1024]
    assert a.tobytes() == plain_run[1].tobytes() and m.tobytes() == plain_run[2].tobytes()


