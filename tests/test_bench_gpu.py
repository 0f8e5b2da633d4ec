"""bench.py's output contract (one JSON line with the driver's keys + roofline; with --full + cpu_baseline) on the tiny
workload."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_contract_line(cuda):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3",
                        "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "rays/s" and d["value"] > 0 and d["vs_baseline"] is None and "workload" in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert (rf["bound"], rf["unit"], rf["peak"]) in (("hbm", "GB/s", 8000.0), ("mfma", "TFLOP/s", 2500.0))
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0 < rf["frac"] < 1
    # the line names the section with the largest per-step time and carries the three longest with their roofs
    assert len(rf["top"]) == 3 and rf["top"][0]["ms"] >= rf["top"][1]["ms"] >= rf["top"][2]["ms"]
    for e in rf["top"]:
        assert e["bound"] in ("hbm", "mfma") and 0 < e["frac"] < 1
        assert all(not isinstance(v, (dict, list)) for v in e.values())
    # (chosen by an instrumented pass before the timed steps; at this tiny size the order of near-equal sections may
    # differ between that pass and the final one, so: one of the three)
    assert any(e["section"] == rf["section"] for e in rf["top"])
    assert len(lines[0]) < 4096


def test_default_bench_line_is_short_flat_and_last(cuda, tmp_path):
    """The line of the --full command (extras, live PMC passes, CPU baseline), only the workload made tiny.  Round 4's
    default line was 22 KB and the driver recorded `parsed: null`; the contract line must stay below 4 KB, be the last
    stdout line, hold scalars only below `config` / `cpu_baseline` / `roofline` (+ its 3-entry `top`), and the full
    record must land in the side file."""
    detail = tmp_path / "bench_detail.json"
    env = dict(os.environ, TNL_BENCH_DETAIL=str(detail))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1",
                        "--full"], capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out_lines = r.stdout.splitlines()
    line = out_lines[-1]
    assert len(line) < 4096 and [l for l in out_lines if l.startswith("{")] == [line]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert all(not isinstance(v, (dict, list)) for v in d["config"].values())
    assert all(not isinstance(v, (dict, list)) for v in d["cpu_baseline"].values())
    assert all(not isinstance(v, (dict, list)) for k, v in d["roofline"].items() if k != "top")
    for k in ("workload", "samples_per_step_per_gpu", "samples_per_sec", "ms_per_step_over_whole_periods",
              "fp32_planes_ms_per_step", "parallelism", "collectives"):
        assert k in d["config"], k
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["host_threads"] >= cb["cores"] and cb["value"] > 0
    full = json.loads(detail.read_text())
    assert full["value"] == d["value"] and "kernels" in full["config"] and "sample" in full["cpu_baseline"]
    # counter traffic of the three longest sections: summed over the section's OWN kernels (round 5's line had 0.014 for
    # the field backward: only k_slab_reduce was matched).  On the tiny workload the planes fit the MALL, so the ratio to
    # the algorithmic bytes only has to be a positive number below 3; bench.py itself warns outside (0.3, 3) at the README sizes
    for e, fe in zip(d["roofline"]["top"], full["roofline"]["top"]):
        assert e["traffic_over_algorithmic"] is not None and 0 < e["traffic_over_algorithmic"] < 3, e
        if e["section"] == "field_bwd":
            assert any(k.startswith("k_field_bwd") for k in fe["traffic_per_kernel"]), fe["traffic_per_kernel"]


def test_plain_bench_run_does_only_the_headline(cuda, tmp_path):
    """Without --full a run sets up, warms up, times its steps and prints the line: the contract's keys and the roofline
    of the section timed inside the steps, nothing that takes runs of its own (no CPU baseline, no whole-period or
    per-section passes, no secondary figures, no live counter traffic) and no side file."""
    detail = tmp_path / "bench_detail.json"
    env = dict(os.environ, TNL_BENCH_DETAIL=str(detail))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out_lines = r.stdout.splitlines()
    line = out_lines[-1]
    assert len(line) < 4096 and [l for l in out_lines if l.startswith("{")] == [line]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["metric"] == "train rays/sec (whole node)" and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f16" and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert "cpu_baseline" not in d and "top" not in d["roofline"] and d["roofline"]["traffic"] is None
    cfg = d["config"]
    assert all(not isinstance(v, (dict, list)) for v in cfg.values())
    for k in ("ms_per_step_over_whole_periods", "fp32_planes_ms_per_step", "no_roi_ms_per_step", "detail",
              "test_render_800x800_4096_steps_ms", "trajectory_512_steps_ms_per_step"):
        assert k not in cfg, k
    # the one section the line names is timed inside the timed steps, and only it
    rf = d["roofline"]
    assert [k for k in cfg if k.startswith("ms_")] == ["ms_" + rf["section"]]
    assert (rf["bound"], rf["unit"], rf["peak"]) in (("hbm", "GB/s", 8000.0), ("mfma", "TFLOP/s", 2500.0))
    assert 0 < rf["frac"] < 1 and rf["avg_launch_ms"] > 0
    assert not detail.exists()


def test_dump_outputs_of_the_last_timed_step(cuda, tmp_path):
    """--dump-outputs DIR: after the timed steps, the last one's loss, renders and updated parameters land in DIR as float32
    .npy files (the large arrays as a seeded sample), 64 MB at most; --steps is the number of timed steps of the line.  Two
    runs with the same arguments write the same arrays: the inputs are seeded and the steps reduce in a fixed order (only
    the loss scalars, summed by float atomics, may differ in the last bits)."""
    import numpy as np
    runs = []
    for k in range(2):
        out = tmp_path / f"dump{k}"
        env = dict(os.environ, TNL_BENCH_DETAIL=str(tmp_path / "bench_detail.json"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "2", "--warmup",
                            "0", "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        assert all(f.suffix == ".npy" for f in out.iterdir())
        runs.append({f.name[:-4]: np.load(f) for f in out.iterdir()})
    files, again = runs
    assert set(files) == set(again)
    for k in files:
        if k in ("loss", "mse", "wavelet_reg"):
            np.testing.assert_allclose(again[k], files[k], rtol=1e-5, atol=0, err_msg=k)
        else:
            assert np.array_equal(again[k], files[k]), k
    need = {"loss", "mse", "wavelet_reg", "image", "weights_sum", "depth", "param.encoder.planes_features",
            "param.encoder.planes_features_wavelet_coefs.1", "param.sigma_net.0.weight", "param.color_net.2.weight",
            "buffer.density_grid"}
    assert need <= set(files), sorted(files)
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["image"].shape == (4096, 3) and files["weights_sum"].shape == (4096,)
    assert files["param.encoder.planes_features"].shape == (3, 16, 64, 64)
    assert files["param.encoder.planes_features_wavelet_coefs.1"].shape == (1 << 20,)      # 3 x 16 x 3 x 128^2: sampled
    for k in ("loss", "mse", "image", "param.encoder.planes_features", "param.encoder.planes_features_wavelet_coefs.1",
              "param.sigma_net.0.weight"):
        assert np.isfinite(files[k]).all(), k
    assert float(files["loss"]) > 0


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_two_ranks_on_one_device(cuda, scaling):
    """The N > 1 code path of bench.py itself (ray shards, slice-sharded dense work, collectives, max-over-ranks
    timing, rank-0 line), launched exactly as the driver does but with both ranks on cuda:0 over gloo -- the only way
    to execute it on a one-GPU box.  RCCL replaces gloo on a real node; the call sequence is the same."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "tiny",
           "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--backend", "gloo", "--same-device", "--scaling", scaling]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["value"] > 0
    assert "dp2" in d["config"]["parallelism"]
    cfg = d["config"]
    assert cfg["rays_per_step_global"] == (4096 if scaling == "strong" else 8192)
    assert cfg["rays_per_step_per_gpu"] * 2 == cfg["rays_per_step_global"]
    assert cfg["collectives"] == "gloo x2"
    assert cfg["wire_reduce_scatter_plane_grad_bytes"] > 0 and cfg["wire_all_gather_planes_bytes"] > 0
    assert len(lines[0]) < 4096
