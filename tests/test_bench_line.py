"""The one JSON line of `python bench.py`, as the driver records it (it keeps the last 8 KB of stdout): the plain run and `--full`."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_default_bench_line_fits_the_drivers_tail_and_names_every_baseline_config():
    sys.path.insert(0, ROOT)
    import bench
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    # the --full invocation with short legs: same code path, same fields (traffic passes off: they are two more child runs)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "5", "--warmup", "1", "--min-seconds", "0.3",
                        "--traffic", "off", "--cpu-scale", "0.03"], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and p.stdout.strip().count("\n") == 0, p.stdout[-2000:]
    assert len(lines[0]) < 8000, len(lines[0])
    d = json.loads(lines[0])
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["frac"] > 0 and "aai_axis_kernel" in d["roofline"]["kernel"]
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0
    assert d["timed"]["step_ms"]["min"] <= d["timed"]["step_ms"]["median"] <= d["timed"]["step_ms"]["max"]
    assert [c["name"] for c in d["configs"]] == [n for n, _ in bench.CONFIG_SET]
    for c in d["configs"]:
        assert c["ms"] > 0 and c["mpix_s"] > 0 and 0 < c["frac"] < 1 and c["kernel"].startswith("aai_"), c
        if "cpu" in c:
            assert c["cpu"][0] > 0 and c["gpu_over_cpu"] > 1, c
    by = {c["name"]: c for c in d["configs"]}
    assert "aai_cell_kernel" in by["cfg3"]["kernel"] and "aai_cell_kernel" in by["cfg5"]["kernel"]
    assert by["cfg4"]["images"] == 64 and by["cfg2"]["dst"] == [2048, 2048] and by["cfg5"]["dst"] == [23170, 23170]


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_only():
    """`bench.py --gpus 1 --steps N --warmup W` without --full: the headline fields, nothing that takes runs of its own (no rocprofv3
    passes, no CPU baselines, no configs block, no per-step pass), and at most 30 s of the whole process outside its N + W steps."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    n, w = 20, 3
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", str(w)],
                       capture_output=True, text=True, env=env, timeout=600)
    wall = time.monotonic() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout)
    assert d["unit"] == "Mpixels/s (output)" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["value"] > 0
    assert d["steps"] == n and d["warmup"] == w and d["timed"]["steps_timed"] == n and d["ms_per_step"] > 0
    assert abs(d["value"] - 4 * 2048 * 2048 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-6 * d["value"]
    assert "aai_axis_kernel" in d["roofline"]["kernel"] and "measured by this run" not in (d["roofline"]["traffic_source"] or "")
    assert not {"cpu_baseline", "configs", "configs_note", "cfg4"} & set(d) and "step_ms" not in d["timed"], sorted(d)
    assert wall - (n + w) * d["ms_per_step"] * 1e-3 <= 30.0, wall


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the batch the timed path computed, as float32 DIR/dst.npy, here config 1 (2 images of 512 x 512 ->
    256 x 256); image b is the seeded synthetic image b + 1, so the dump must match the CPU oracle on it."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle import pyoracle as po
    if not po.have_oracle():
        po.build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg1", "--batch", "2", "--steps", "3", "--warmup", "1",
                        "--traffic", "off", "--configs", "off", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout)
    assert d["timed"]["steps_timed"] == 3 and d["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["dst.npy"]
    dst = np.load(os.path.join(tmp_path, "dst.npy"))
    assert dst.dtype == np.float32 and dst.shape == (2, 256, 256)
    for b in range(2):
        gold = po.oracle_run(po.MODE_EXACT, po.synth_image(512, 512, b + 1).astype(np.float64), 2.0, 1.0, (255.5, 255.5), 0.0).dst
        err = np.abs(dst[b] - gold) / np.maximum(np.abs(gold), 1e-3)
        assert err.max() <= 1e-5, (b, float(err.max()))
