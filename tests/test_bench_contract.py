"""bench.py prints ONE JSON line with the driver's contract keys plus `roofline`; `--full` adds `cpu_baseline`,
`other_workloads` and the roofline's bare stream."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}


def _run(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean():
    """A plain run does only what its headline needs: no CPU baselines, no other workloads, no bare stream, and at most
    30 s of the whole process's time outside its warm-up and timed steps."""
    t0 = time.perf_counter()
    j = _run("--steps", "2", "--warmup", "1")
    wall = time.perf_counter() - t0
    assert KEYS <= set(j) and j["steps"] == 2 and j["warmup"] == 1 and j["unit"] == "rays/s"
    assert not {"cpu_baseline", "cpu_baseline_c1", "other_workloads"} & set(j)
    r = j["roofline"]
    assert r["bare_stream"] is None and r["frac_of_bare_stream"] is None and r["fill"]["bare_stream_tbps"] is None
    assert 0.05 < r["frac"] < 0.34 and 1.0 < r["clock_ghz"] < 2.6
    assert wall - 3 * j["ms_per_step"] * 1e-3 < 30.0, (wall, j["ms_per_step"])


@pytest.mark.gpu
def test_render_line_contract():
    j = _run("--steps", "1", "--warmup", "1", "--full")
    assert KEYS <= set(j) and "cpu_baseline" in j
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["warmup"] == 1 and j["higher_is_better"] is True
    assert j["scaling"] == "weak" and j["vs_baseline"] is None and j["data"] == "synthetic" and j["unit"] == "rays/s"
    assert "800x800" in j["config"]["workload"] and "model" not in j["config"]
    r = j["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.05 < r["frac"] < 0.34
    # whole-job rate and the kernel-only rate describe the same launches
    assert abs(j["value"] * r["flop_per_ray"] / 1e12 - r["achieved"]) < 0.1 * r["achieved"]
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "rays/s" and c["cores"] >= 1 and 1.0 < c["value"] < j["value"] / 100
    assert isinstance(c["cpu_model"], str) and c["cpu_model"]
    # round 4: the roofline's side figures are facts of THIS run: the clock held during the timed
    # launches, the kernel's own bare MFMA stream launched on the same device, the L2 -> LDS fill rate as second ceiling
    assert 1.0 < r["clock_ghz"] < 2.6 and 0.3 < r["mfma_busy_derived"] < 1.0
    b = r["bare_stream"]
    assert b["measured"].startswith("in this run") and 800.0 < b["mfma_tflops"] < 2500.0 and 1.0 < b["clock_ghz"] < 2.6
    assert abs(r["frac_of_bare_stream"] - r["mfma_tflops_issued"] / b["mfma_tflops"]) < 1e-9 and 0.5 < r["frac_of_bare_stream"] < 1.05
    f = r["fill"]
    assert abs(f["bytes_per_launch"] - (320000 * 1966080 + 960000 * 2375680)) < 1.0 and 3.0 < f["tbps"] < 12.0
    assert f["bare_stream_tbps"] == b["fill_tbps"]
    # ... and the other rows' workloads ride in the same line (VERDICT r3 missing #3)
    ow = j["other_workloads"]
    assert set(ow) == {"train", "occgrid", "train-occ", "bf16", "bf16_c5", "train-occ_cull-bf16", "occgrid_cull-bf16"}
    for name, w in ow.items():
        assert "error" not in w, (name, w)
        assert w["value"] > 1e4 and w["ms_per_step"] > 0, (name, w)
        if "frac" in w:
            assert 0.02 < w["frac"] < 0.9, (name, w)
    assert ow["occgrid"]["fused_equals_unfused_bitwise"] is True
    # the opt-in bf16 visibility cull: labelled, faster, and the image within the cull's own threshold of the default path
    assert ow["train-occ_cull-bf16"]["cull_precision"] == "bf16" and ow["train-occ"]["cull_precision"] != "bf16"
    assert ow["train-occ_cull-bf16"]["ms_per_step"] < ow["train-occ"]["ms_per_step"]
    c = ow["occgrid_cull-bf16"]
    assert c["ms_per_step"] < c["default_path_ms_same_frame"] and c["max_abs_rgb_vs_default"] < 1e-4


@pytest.mark.gpu
def test_train_line_contract():
    j = _run("--workload", "train", "--steps", "3", "--warmup", "1")
    assert KEYS <= set(j) and j["steps"] == 3 and "trained rays/sec" in j["metric"]
    assert j["config"]["rays_per_step"] == 4096 and j["config"]["parallelism"].startswith("dp1")
    assert 0.0 < j["loss"] < 1.0 and j["value"] > 1e4


@pytest.mark.gpu
def test_occupancy_lines_contract():
    """`--workload occgrid` (the reference's render path in one launch) and `--workload train-occ` (its training loop
    body): contract keys, the sample counts the FLOP figure is built from, and the fused == unfused statement."""
    j = _run("--workload", "occgrid", "--steps", "1", "--warmup", "1")
    assert KEYS <= set(j) and "occupancy-grid" in j["metric"] and j["unit"] == "rays/s"
    c = j["config"]
    assert c["rays_per_step"] == 640000 and 0.4 < c["occupied_cells"] < 0.6 and c["fused_equals_unfused_bitwise"] is True
    assert c["marched_samples_per_ray"] > c["kept_samples_per_ray"] > 10
    assert 0.05 < j["roofline"]["frac"] < 0.34 and j["roofline"]["kernel"] == "k_render_occ"
    t = _run("--workload", "train-occ", "--steps", "3", "--warmup", "1")
    assert KEYS <= set(t) and t["steps"] == 3 and "trained rays/sec (occupancy" in t["metric"]
    assert t["config"]["rays_per_step"] == 4096 and t["config"]["marched_samples_per_ray"] > t["config"]["kept_samples_per_ray"] > 5
    assert 0.0 < t["loss"] < 1.0 and t["value"] > 1e4


@pytest.mark.gpu
def test_dump_outputs(tmp_path):
    """`--dump-outputs DIR`: what the timed path returned in its last step, float32, within 64 MB; the raw launch's
    per-sample outputs as a fixed sample of rays; the training step's loss, colours and updated parameters."""
    j = _run("--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "frame"))
    assert j["steps"] == 2
    rgb, depth = np.load(tmp_path / "frame" / "rgb.npy"), np.load(tmp_path / "frame" / "depth.npy")
    assert rgb.shape == (800, 800, 3) and depth.shape == (800, 800) and rgb.dtype == depth.dtype == np.float32
    assert np.isfinite(rgb).all() and 2.0 <= depth.min() and depth.max() <= 6.0
    _run("--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--raw-launch", "--extras", "--dump-outputs",
         str(tmp_path / "raw"))
    raw = {f[:-4]: np.load(tmp_path / "raw" / f) for f in os.listdir(tmp_path / "raw")}
    assert set(raw) == {"rgb", "depth", "opacity", "weights", "alphas", "trans", "sigmas", "rgbs", "edges", "weights_coarse"}
    assert sum(a.nbytes for a in raw.values()) <= 64 << 20 and all(a.dtype == np.float32 for a in raw.values())
    assert raw["rgb"].shape == (640000, 3) and raw["opacity"].shape == (640000, 1)
    assert raw["weights"].shape == (4096, 192) and raw["rgbs"].shape == (4096, 192, 3) and raw["edges"].shape == (4096, 193)
    assert np.allclose(raw["rgb"], rgb.reshape(-1, 3), rtol=0, atol=1e-5), "the same frame through the raw launch"
    t = _run("--workload", "train", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "train"))
    files = os.listdir(tmp_path / "train")
    assert {"loss.npy", "rgb.npy", "param.sigma.weight.npy"} <= set(files)
    assert abs(float(np.load(tmp_path / "train" / "loss.npy")[0]) - t["loss"]) < 1e-6
    assert np.load(tmp_path / "train" / "rgb.npy").shape == (4096, 3)


def test_dump_helpers(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    x = torch.arange(10000 * 7, dtype=torch.int32).reshape(10000, 7)
    s = bench.sample_rays(x)
    assert s.shape == (4096, 7) and torch.equal(s, bench.sample_rays(x)), "the same rows in every run"
    rows = s[:, 0] // 7
    assert torch.equal(rows, rows.unique()), "distinct rows, in order"
    bench.dump_outputs(str(tmp_path / "d"), {"s": s, "f64": torch.ones(3, dtype=torch.float64)})
    assert np.load(tmp_path / "d" / "s.npy").dtype == np.float32 and np.load(tmp_path / "d" / "f64.npy").dtype == np.float64
    with pytest.raises(RuntimeError, match="64"):
        bench.dump_outputs(str(tmp_path / "big"), {"a": torch.zeros((64 << 20) // 4 + 1)})
    assert not os.path.exists(tmp_path / "big")


def test_full_is_an_option():
    out = _launch("--full", "--dry-run")
    assert out.returncode == 0 and json.loads(out.stdout.splitlines()[-1])["dry_run"], out.stderr[-2000:]


def test_steps_must_be_positive():
    out = _launch("--steps", "0", "--dry-run")
    assert out.returncode != 0 and "--steps" in out.stderr


# ---- the N>1 launcher (CPU: `--dry-run` children join a gloo group instead of touching the GPU)
def _launch(*args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=600, cwd=ROOT, env=e)


def test_self_launch_two_ranks_dry_run():
    """`python bench.py --gpus 2` with no WORLD_SIZE starts 2 fresh ranks, wires RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* and relays exactly rank 0's JSON line."""
    out = _launch("--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run")
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j["dry_run"] and j["n_gpus"] == 2 and j["world"] == 2 and j["rank"] == 0 and j["steps"] == 3
    assert j["max_over_ranks"] == 2.0            # max over ranks of (1 + rank): both ranks joined the group
    assert j["local_ranks_plus_1"] == [1, 2]     # every rank saw its own LOCAL_RANK


def test_self_launch_propagates_rank_failure():
    out = _launch("--gpus", "2", "--dry-run", env={"FSN_BENCH_FAIL_RANK": "1"})
    assert out.returncode != 0 and "rank 1 exited" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")], "no result line from a failed job"


def test_world_size_mismatch_is_an_error():
    out = _launch("--gpus", "4", "--dry-run", env={"WORLD_SIZE": "2", "RANK": "0"})
    assert out.returncode != 0 and "WORLD_SIZE=2" in (out.stderr + out.stdout)


def test_traffic_is_never_stale():
    sys.path.insert(0, ROOT)
    import bench
    t, src = bench.measured_traffic("no-such-mode")
    assert t is None and "note" in src
    t, src = bench.measured_traffic("fp16x3")
    assert (t is None and "note" in src) or src["csrc_sha"] == bench.csrc_sha()
