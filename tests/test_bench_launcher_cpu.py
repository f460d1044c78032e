"""bench.py's own multi-rank code path, on CPU: `--gpus 2 --backend gloo --dry` must start two ranks by itself
(no external torchrun, no WORLD_SIZE in the environment), rendezvous on 127.0.0.1, shard, all-gather and print ONE
JSON line from rank 0 (BASELINE configs[2] is the same path with 8 ranks on RCCL)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{") and '"metric"' in l]


def test_gpus2_spawns_two_ranks_and_prints_one_line():
    r = _run(["--gpus", "2", "--backend", "gloo", "--dry", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    j = lines[0]
    assert j["n_gpus"] == 2 and j["dry"] is True and j["config"]["global_batch"] == 2048
    assert j["members_per_step"] == 2048 and j["solved_per_step"] == 2048.0
    assert len(j["ms_per_step_by_rank"]) == 2 and j["gather_self_check"] is True
    assert j["scaling"] == "weak" and j["steps"] == 2 and j["warmup"] == 1


def test_single_rank_dry_line():
    r = _run(["--dry", "--backend", "gloo", "--steps", "1", "--warmup", "0", "--batch", "16"])
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_lines(r.stdout)[0]
    assert j["n_gpus"] == 1 and j["config"]["global_batch"] == 16 and j["ms_per_step_by_rank"] is None


def test_mismatched_world_size_is_refused():
    r = _run(["--gpus", "4", "--dry", "--backend", "gloo"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_no_gpu_means_loud_failure_not_a_cpu_number():
    # no device visible to the child, also on a machine that has one
    r = _run(["--steps", "1", "--warmup", "0", "--batch", "4"], env_extra={"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"})
    assert r.returncode != 0
    assert not _json_lines(r.stdout)


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs: the stub's outputs of the last timed step (x = that step's x0) as float npy files, the same from run to run"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import importlib
    problem = importlib.import_module("landing-controller_amd.problem")
    dumps = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        r = _run(["--dry", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--batch", "8", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        j = _json_lines(r.stdout)[0]
        assert j["steps"] == 3 and len(j["ms_by_step_rank0"]) == 3 and j["ms_per_step"] > 0
        assert j["dumped_outputs"]["files"] == sorted(n + ".npy" for n in ("x", "f", "lam_g", "status", "iters", "kkt"))
        dumps.append({n: np.load(str(d / n)) for n in j["dumped_outputs"]["files"]})
    for n, v in dumps[0].items():
        assert v.dtype in (np.float32, np.float64) and v.shape[0] == 8, n
        assert np.array_equal(v, dumps[1][n]), n
    _, X0, _, _ = problem.make_batch(8, 40, 0.6, seed=20211 + 1000 * 2)      # the last timed step's batch (step 2)
    assert np.array_equal(dumps[0]["x.npy"], X0)
    assert dumps[0]["status.npy"].max() == 0 and dumps[0]["iters.npy"].min() == 1


def test_dump_outputs_samples_members_above_the_size_limit(tmp_path):
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(3)
    arrays = {"x": rng.normal(size=(100, 50)), "status": rng.integers(0, 3, size=100).astype(np.int32)}
    limit = 100 * 51 * 8 // 4
    info = bench.write_outputs(str(tmp_path), arrays, np, limit=limit)
    assert info["bytes"] <= limit and "rows.npy" in info["files"]
    rows = np.load(str(tmp_path / "rows.npy")).astype(int)
    x, st = np.load(str(tmp_path / "x.npy")), np.load(str(tmp_path / "status.npy"))
    assert len(rows) == x.shape[0] == st.shape[0] > 0 and np.all(np.diff(rows) > 0)
    assert np.array_equal(x, arrays["x"][rows]) and np.array_equal(st, arrays["status"][rows])
    again = tmp_path / "again"
    bench.write_outputs(str(again), arrays, np, limit=limit)
    assert np.array_equal(np.load(str(again / "rows.npy")), np.load(str(tmp_path / "rows.npy")))
    info = bench.write_outputs(str(tmp_path / "all"), arrays, np)
    assert "rows.npy" not in info["files"] and info["members"] == 100
