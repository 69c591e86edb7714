"""GPU: bench.py's one-line JSON contract (driver-facing), on a tiny run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_contract_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "2", "--full",
                          "--frames-per-step", "4", "--repeats", "3", "--cpu-sample", "2", "--host-path-frames", "2"], capture_output=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, "bench.py must print exactly one line on stdout"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 12 and d["warmup"] == 2
    assert d["unit"] == "Mpts/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] * 1e3 - d["config"]["points_per_step"]) < 1e-2 * d["config"]["points_per_step"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "dense" in c["sample"]
    assert d["cpu_baseline_sparse"]["cores"] == 1 and d["cpu_baseline_all_cores"]["cores"] >= 1
    assert d["rows_extracted"] > 0
    # 12 steps of 4 frames, clean every 3 steps: the steady state (dependant updates) is inside the timed region
    assert d["config"]["points_per_step"] == 4 * 640 * 480 and d["config"]["frames"] == 48
    assert d["repeats"] == 3 and len(d["pass_s"]) == 3 and d["value_min"] <= d["value"] <= d["value_max"]
    assert d["clean_passes"] == 4 and d["counters"]["dep_pairs_tested"] > 0 and d["warnings"] == []
    assert r["traffic"] is None or r["traffic"] > 0
    assert r["kernel_source_sha"] and r["traffic_source"]


def test_bench_steps_and_dumped_outputs(tmp_path):
    """--steps sets the frames of every timed pass, also for a stream that one clean epoch covers (every point is buffered); two runs
    with the same arguments dump the same outputs of the last pass."""
    dumps = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
                              "--repeats", "2", "--cpu-sample", "0", "--host-path-frames", "0", "--dump-outputs", str(tmp_path / run)],
                             capture_output=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        d = json.loads(out.stdout.decode().strip())
        assert d["steps"] == 2 and d["config"]["frames"] == 100
        assert d["counters"]["points_presented"] == 100 * 640 * 480  # of the last pass (clear resets it)
        assert d["counters"]["frames_integrated"] == 2 * 100  # since create: 2 passes of 2 steps x 50 frames, no warm-up
        files = sorted(os.listdir(str(tmp_path / run)))
        dumps.append({f: np.load(str(tmp_path / run / f)) for f in files})
        assert dumps[-1]["sizes.npy"][0] == d["rows_extracted"] > 0
        assert len(dumps[-1]["rows_xyz.npy"]) == min(d["rows_extracted"], 1 << 19)  # bench.DUMP_MAX_ROWS: a sample above it
        assert sum(a.nbytes for a in dumps[-1].values()) <= 64 << 20
    assert sorted(dumps[0]) == sorted(dumps[1])
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, dumps[1][f]), f


def test_bench_plain_run_is_lean_and_dumps_what_full_dumps(tmp_path):
    """A plain run prints the headline line without the figures of the legs only --full runs (per-kernel breakdown, extract,
    host path, CPU baselines); the two dump the same outputs of the last timed pass."""
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "1", "--frames-per-step", "4",
            "--repeats", "2", "--cpu-sample", "2", "--host-path-frames", "2"]
    lines, dumps = {}, {}
    for mode in ("plain", "full"):
        out = subprocess.run(args + ["--dump-outputs", str(tmp_path / mode)] + (["--full"] if mode == "full" else []),
                             capture_output=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        lines[mode] = json.loads(out.stdout.decode().strip())
        dumps[mode] = {f: np.load(str(tmp_path / mode / f)) for f in sorted(os.listdir(str(tmp_path / mode)))}
    p, f = lines["plain"], lines["full"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "repeats", "pass_s", "counters", "roofline"):
        assert k in p, k
    assert p["value"] > 0 and abs(p["ms_per_step"] * p["value"] * 1e3 - p["config"]["points_per_step"]) < 1e-2 * p["config"]["points_per_step"]
    for k in ("extract_s", "write_times", "host_path_mpts", "host_path_frames", "cpu_baseline", "cpu_baseline_sparse", "vs_cpu_baseline"):
        assert k not in p and k in f, k
    assert "kernels" not in p["roofline"] and "compute_integrate" not in p["roofline"] and f["roofline"]["kernels"]["k_integrate"]["calls"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "repeats", "config", "counters", "rows_extracted"):
        assert p[k] == f[k], k
    assert p["rows_extracted"] > 0
    assert sorted(dumps["plain"]) == sorted(dumps["full"])
    for name, a in dumps["plain"].items():
        assert np.array_equal(a, dumps["full"][name]), name


def test_bench_two_ranks_one_line_on_stdout():
    """Launched the way the driver launches N > 1 (one rank per GPU; here both ranks share the one GPU, so the RCCL
    communicator is refused and the ranks agree to fall back to the host-staged transport).  Gloo and RCCL print banners on
    fd 1; stdout must still carry exactly one JSON line, from rank 0."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "12", "--warmup", "2",
                          "--frames-per-step", "4", "--repeats", "2", "--full"],
                         capture_output=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, "stdout must be exactly one line, got %d: %r" % (len(lines), lines[:3])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 12 and d["scaling"] == "weak"
    assert d["config"]["points_per_step"] == 4 * 640 * 480
    assert "host-staged (gloo), 2 ranks" in d["config"]["parallelism"]
    assert "cpu_baseline" not in d  # rank 0 at N = 1 only
    assert d["value"] > 0 and d["rows_extracted"] > 0
