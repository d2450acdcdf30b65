"""bench.py's own line: the plain run (the headline and nothing else) and the outputs it dumps, the `--full` run's
self-check against the oracle and its evidence fields, and -- where the box has two GPUs -- the real RCCL path (one
process per GPU, backend "nccl").  GPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_checks_its_own_output_against_the_oracle():
    """A short `--full` run of the default workload's code path (2 frame pairs): the line carries `check` (max-abs error of the
    timed launches' output against the oracle, must be <= 1e-4), `roofline`, `cpu_baseline`, `traffic_source`, and the
    input sets it rotated over (a 2-frame launch moves 177 MB: eight sets)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--batch", "2", "--steps", "6",
                        "--warmup", "2", "--prewarm", "4", "--no-secondary", "--cpu-seconds", "0.5", "--launch", "eager"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    line = _line(r.stdout)
    assert line["check"]["ok"] and line["check"]["max_abs_err"] <= 1e-4 and line["check"]["frames"] == 2
    assert line["config"]["input_sets"] >= 4
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["frac"] > 0
    assert "traffic_source" in line["roofline"]
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] >= 1
    assert line["n_gpus"] == 1 and line["dtype"] == "f32" and line["vs_baseline"] is None
    c = line["config"]
    assert c["windows"] == 7 and c["launch"] == "eager" and c["window_gpu_us_per_step"] > 0
    assert c["window_ms_min_max"][0] - 1e-3 <= line["ms_per_step"] * 6 <= c["window_ms_min_max"][1] + 1e-3
    assert len(line["roofline"]["first_launches_us"]) == 4


def _plain_run_with_dump(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "6", "--input-sets", "1",
                        "--steps", "5", "--warmup", "2", "--prewarm", "4", "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return _line(r.stdout), {f[:-4]: np.load(os.path.join(str(out_dir), f)) for f in sorted(os.listdir(str(out_dir)))}


def test_plain_run_times_exactly_its_steps_and_dumps_the_last_output(tmp_path, oracle):
    """A plain run: ONE window of exactly --steps steps, the headline fields and nothing measured besides them; with
    --dump-outputs, the last timed step's output (6 frame pairs = 66 MB: the first frame whole plus a seeded sample).  The
    dumped frame is the oracle's result on the same seeded inputs, and a second run with the same arguments writes the
    same files bit for bit."""
    line, files = _plain_run_with_dump(tmp_path / "a")
    assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mpixels/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    c = line["config"]
    assert c["windows"] == 1 and c["input_sets"] == 1 and c["batch_per_gpu"] == 6
    assert abs(c["window_ms_min_max"][0] - line["ms_per_step"] * 5) <= 1e-3
    for key in ("roofline", "cpu_baseline", "check", "secondary", "dist"):
        assert key not in line, key
    assert sorted(files) == ["output_frame0", "output_sample", "output_sample_index"]
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    frame0, sample, index = files["output_frame0"], files["output_sample"], files["output_sample_index"]
    assert frame0.dtype == sample.dtype == np.float32 and index.dtype == np.float64
    assert frame0.shape == (3, 720, 1280) and sample.shape == index.shape and sample.size > 1 << 20
    idx = index.astype(np.int64)
    assert np.all(idx == index) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 6 * 3 * 720 * 1280
    first = idx < frame0.size
    assert first.any() and np.array_equal(sample[first], frame0.reshape(-1)[idx[first]])

    from tools import synth
    t = synth.torch_inputs(torch.device("cuda", 0), 6, 3, 720, 1280, fs=4, flow_kind="smooth", seed=1234)
    x, flow, filt = (t[k][:1].cpu().numpy() for k in ("x", "flow", "filt"))
    del t
    want = oracle.filter_interpolation_forward(x, flow, filt)[0]
    assert float(np.abs(frame0.astype(np.float64) - want).max()) <= 1e-4

    line2, files2 = _plain_run_with_dump(tmp_path / "b")
    assert sorted(files2) == sorted(files)
    for k in files:
        assert files2[k].dtype == files[k].dtype and np.array_equal(files2[k], files[k]), k


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: the lease of this pool has one")
def test_two_ranks_over_rccl():
    """The N > 1 path as the driver launches it: one process per GPU, backend nccl (= RCCL), strong scaling.  The line
    must say what the collective layer saw."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29631", os.path.join(ROOT, "bench.py"),
                        "--full", "--gpus", "2", "--steps", "20", "--warmup", "5", "--prewarm", "20"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    line = _line(r.stdout)
    d = line["dist"]
    assert d["backend"] == "nccl" and d["world_size_seen"] == 2
    assert d["per_rank_items"] == [16, 16] and len(d["per_rank_ms_per_step"]) == 2
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["global_batch"] == 32


def test_collective_layer_on_a_one_rank_rccl_communicator():
    """The lease has one GPU, so the N > 1 path has never met RCCL -- but a communicator of ONE rank is a real RCCL communicator:
    `--dist-single` sends the whole collective layer of the bench line through backend nccl (init with device_id, the int64
    broadcast, the barrier in front of every window, the float64 MAX all-reduce of the window times, the timed barriers, the
    all-gather), on device tensors, as the ranks of an 8-GPU job would."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--dist-single", "--batch", "2", "--steps", "6",
                        "--warmup", "2", "--prewarm", "4", "--windows", "3", "--no-secondary", "--cpu-seconds", "0.5"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    line = _line(r.stdout)
    d = line["dist"]
    assert d["backend"] == "nccl" and d["world_size_seen"] == 1 and d["single_rank_communicator"] is True
    assert d["per_rank_items"] == [2] and len(d["worst_window_ms"]) == 3 and d["barrier_us"] > 0
    assert "rccl_version" in d
    assert line["n_gpus"] == 1 and line["check"]["ok"]                 # (still rank 0 at N = 1: the oracle check runs)


def test_two_ranks_sharing_one_gpu_plumbing():
    """The N > 1 code path end to end on a one-GPU box: two ranks on the same device, gloo standing in for RCCL (which
    refuses two ranks on one device).  Not a measurement -- the line says so in `data` -- but every collective, the shard
    plan, the HIP-graph replay of the rotating input sets and the `dist` record run for real."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29633", os.path.join(ROOT, "bench.py"),
                        "--full", "--gpus", "2", "--share-gpu", "--batch", "8", "--steps", "12", "--warmup", "3", "--prewarm", "6",
                        "--launch", "graph", "--windows", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    line = _line(r.stdout)
    d = line["dist"]
    assert d["backend"] == "gloo" and d["world_size_seen"] == 2 and d["per_rank_items"] == [4, 4]
    assert len(d["per_rank_ms_per_step"]) == 2 and all(t > 0 for t in d["per_rank_ms_per_step"])
    assert "PLUMBING TEST" in line["data"] and line["n_gpus"] == 2 and line["config"]["global_batch"] == 8
    assert line["config"]["launch"] == "hip_graph" and line["config"]["input_sets"] >= 4
    assert line["config"]["windows"] == 3 and len(d["worst_window_ms"]) == 3 and d["barrier_us"] > 0
    assert min(d["worst_window_ms"]) - 1e-3 <= line["ms_per_step"] * 12 <= max(d["worst_window_ms"]) + 1e-3      # the median window
    assert "cpu_baseline" not in line and "check" not in line          # rank 0 at N = 1 only
