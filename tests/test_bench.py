"""bench.py's own options: --dump-outputs writes what the timed path returned in its last timed step, and a plain run
prints the headline without the --full extras (roofline, cpu_baseline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_and_a_fixed_sample_past_the_limit(tmp_path):
    u8 = np.arange(6 * 5 * 3, dtype=np.uint8).reshape(6, 5, 3)
    f64 = np.linspace(0.0, 1.0, 90).reshape(6, 5, 3)
    bench.dump_outputs(str(tmp_path / "all"), {"u8": u8, "f64": f64})
    a, b = np.load(tmp_path / "all" / "u8.npy"), np.load(tmp_path / "all" / "f64.npy")
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (6, 5, 3)
    assert np.array_equal(a, u8.astype(np.float32)) and np.array_equal(b, f64.astype(np.float32))
    limit = 2 * 4096 + 200                                      # 200 bytes for the data of two 360-byte arrays
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), {"u8": u8, "f64": f64}, limit=limit)
    names = ("u8.npy", "f64.npy")
    assert sum(os.path.getsize(tmp_path / "s1" / n) for n in names) <= limit
    for n in names:
        s1, s2 = np.load(tmp_path / "s1" / n), np.load(tmp_path / "s2" / n)
        assert s1.ndim == 1 and 0 < s1.size < 90 and np.array_equal(s1, s2)
    s = np.load(tmp_path / "s1" / "u8.npy")
    assert np.all(np.diff(s) > 0) and np.isin(s, u8.reshape(-1)).all()          # elements of the output, in index order


@pytest.mark.gpu
@pytest.mark.parametrize("route", [[], ["--via-multi"]], ids=["mi_ctx", "mi_multi"])
def test_plain_run_dumps_the_last_timed_step(tmp_path, gpu_ctx, route):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` (and through mi_multi_*): the headline fields, no --full extras,
    and the images of the last timed step (seed 1 + 2) equal mi_render's of the same scene and seed."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--spp", "16",
                          "--dump-outputs", str(tmp_path), *route], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "Msamples/s" and rec["dtype"] == "f32"
    assert rec["higher_is_better"] is True and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(1920 * 1080 * 16 / rec["ms_per_step"] / 1e3, rel=1e-9)
    assert "roofline" not in rec and "cpu_baseline" not in rec
    f32, u8 = np.load(tmp_path / "image_f32.npy"), np.load(tmp_path / "image_u8.npy")
    assert f32.dtype == u8.dtype == np.float32 and f32.shape == u8.shape == (1080, 1920, 3)
    sc = bench.make_scene("cfg2")
    sc.camera.aa_sample_count = 16
    gpu_ctx.upload(sc.flatten())
    ref32, ref8, _, _ = gpu_ctx.render(sc.camera, seed=3)
    assert np.array_equal(f32, ref32, equal_nan=True) and np.array_equal(u8, ref8.astype(np.float32))
    # the timed form (no signatures: dead tiles skipped) against the form the oracle tests pin (signatures: every sample traced)
    sig32, sig8, _, _ = gpu_ctx.render(sc.camera, seed=3, want_sig=True)
    assert np.array_equal(f32, sig32) and np.array_equal(u8, sig8.astype(np.float32))
