"""bench.py's multi-GPU launch paths on the one-GPU test box (VERDICT r3 item
1): the in-process row-band group (gs_create with num_gpus: ncclCommInitAll,
one host thread per band) runs with no launcher and emits a valid line.  At
--gpus 1 that is `--gather` (RCCL over one device); the same code path serves
--gpus N on an N-GPU node.  One subprocess per case, one at a time."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args, timeout=240):
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=timeout, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_in_process_group_over_rccl():
    d = _bench("--full", "--gather", "--n", "200000", "--steps", "60", "--warmup", "20", "--profile-frames", "6",
               "--no-cpu-baseline")
    assert d["n_gpus"] == 1
    assert d["value"] > 0 and d["unit"] == "frames/s"
    assert d["frame_check"]["last_timed_frame_equals_blocking_render"]
    gr = d["group"]
    assert gr["mode"] == "group"
    assert gr["world"] == 1
    assert gr["rccl_comm_ranks"] == 1  # ncclCommCount of the one-device communicator
    assert gr["timed_frames"] >= 6
    assert len(gr["band_ms"]) == 1 and gr["band_ms"][0] > 0
    assert gr["gather_ms"][0] >= 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["frac"] > 0 and r["alg_bytes_per_launch"] > 0
    # the group's stats carry the kernels its band renderer launched (a
    # one-band group renders the whole frame: the two-pixel blend), so the
    # line's PMC lookup asks for the right kernels
    assert r["traffic_kernels"] == ["gs_blend_px2"], r


def test_bench_refuses_more_gpus_than_visible():
    """--gpus N with fewer devices: a clear error before any frame."""
    import torch

    n = torch.cuda.device_count()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1), "--steps", "2"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode != 0
    assert "HIP device" in out.stderr


def test_bench_single_gpu_line_reports_end_to_end():
    """The one-GPU line: `value` from the device-resident frames, and beside it
    the end-to-end rate with every frame's BGR8 read back to pinned host
    memory (the reference's timer includes its readback)."""
    d = _bench("--full", "--n", "200000", "--steps", "60", "--warmup", "20", "--profile-frames", "6",
               "--e2e-frames", "30", "--no-cpu-baseline")
    assert d["n_gpus"] == 1 and d["value"] > 0
    e = d["end_to_end"]
    assert e["frames"] == 30 and 0 < e["frames_per_s"]
    assert d["roofline"]["traffic_kernels"] == ["gs_blend_px2"]


def test_bench_plain_line_and_dumped_outputs(built, tmp_path):
    """A plain run: --steps sets the timed frames, the line carries the
    headline fields and ms_per_step and none of --full's passes, and
    --dump-outputs writes the last timed frame: bit for bit the frame a
    blocking render of the same seeded scene gives (odd step count: the last
    step lands on the first of the three renderers in flight)."""
    import numpy as np

    from gaussian_splat_ipu_amd import camera, scene
    from gaussian_splat_ipu_amd.splatter import GpuSplatter
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    d = _bench("--gpus", "1", "--n", "200000", "--steps", "7", "--warmup", "3", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 7 and d["warmup"] == 3 and d["full"] is False
    assert d["value"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] == pytest.approx(1e3 / d["value"], rel=1e-3)
    for k in ("frame_check", "end_to_end", "kernels", "roofline", "cpu_baseline", "frame_latency_ms"):
        assert k not in d
    out = {k: np.load(tmp_path / f"{k}.npy") for k in d["dumped_outputs"]}
    assert sorted(out) == ["bgr", "histogram", "rgba"]
    assert out["bgr"].dtype == np.float32 and out["rgba"].dtype == np.float32 and out["histogram"].dtype == np.float64
    assert sum(v.nbytes for v in out.values()) <= 64_000_000

    g, bb = scene.prepare_scene(scene.synthetic(scene.SynthSpec(n=200_000, seed=1, sh_degree=3)))
    view, proj = camera.headless(bb, 1920, 1080)
    with GpuSplatter(g, TiledFramebuffer(1920, 1080, 16, 16), device=0) as s:
        s.set_view_wire(view)
        s.set_projection_wire(proj)
        s.update_focal_lengths(camera.FOV_DEFAULT, 1.0)
        s.execute()
        np.testing.assert_array_equal(out["bgr"], s.get_frame_buffer().astype(np.float32))
        np.testing.assert_array_equal(out["rgba"].view(np.uint32), s.get_rgba().view(np.uint32))
        np.testing.assert_array_equal(out["histogram"], s.get_histogram().astype(np.float64))
