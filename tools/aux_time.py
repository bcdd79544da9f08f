#!/usr/bin/env python3
"""What the auxiliary pass costs (gs_aux_device: the re-binning of the last
frame + gs_aux_blend_kernel), next to the frame it describes.

On one renderer, after a warm-up, alternating windows of --iters iterations of

    A: gs_render + gs_sync            (a blocking frame)
    B: gs_render + gs_aux_device      (the same frame, then its aux planes)

are timed, --repeats times interleaved (A B A B ...); B - A is the cost of
the pass per frame, re-binning included.  Prints one JSON line per workload:
config 3 (1M Gaussians, 1920x1080, 16x16 tiles) and config 5's scene and size
(8M clustered Gaussians, 3840x2160, its orbit camera).

    python tools/aux_time.py [--iters 200] [--repeats 3] [--only c3|c5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(name):
    import numpy as np

    from gaussian_splat_ipu_amd import camera, scene

    if name == "c5":
        src = scene.load_ply(os.path.join(ROOT, "tests", "golden", "point_cloud_12.ply"))
        centres = np.stack([src["x"], src["y"], src["z"]], 1)
        ply = scene.synthetic(scene.SynthSpec(n=8_000_000, seed=8, sh_degree=0, cluster_xyz=centres,
                                              cluster_sigma=0.02))
        W, H = 3840, 2160
    else:
        ply = scene.synthetic(scene.SynthSpec(n=1_000_000, seed=1, sh_degree=3))
        W, H = 1920, 1080
    g, bb = scene.prepare_scene(ply)
    view, proj = camera.headless(bb, W, H)
    views = [camera.orbit_view(k) for k in range(120)] if name == "c5" else [view]
    return g, proj, views, W, H


def measure(name, iters, repeats, warmup):
    from gaussian_splat_ipu_amd import camera
    from gaussian_splat_ipu_amd._lib import check, lib
    from gaussian_splat_ipu_amd.splatter import GpuSplatter
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    g, proj, views, W, H = workload(name)
    L = lib()
    with GpuSplatter(g, TiledFramebuffer(W, H, 16, 16), device=0) as s:
        s.set_projection_wire(proj)
        s.update_focal_lengths(camera.FOV_DEFAULT, 1.0)
        h = s.handle
        pf, pu, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        k = [0]

        def frame():
            if len(views) > 1:
                s.set_view_wire(views[k[0] % len(views)])
                k[0] += 1
            check(L.gs_render(h), "gs_render")

        def loop_a(count):
            t0 = time.perf_counter()
            for _ in range(count):
                frame()
                check(L.gs_sync(h), "gs_sync")
            return (time.perf_counter() - t0) / count * 1e6

        def loop_b(count):
            t0 = time.perf_counter()
            for _ in range(count):
                frame()
                check(L.gs_aux_device(h, C.byref(pf), C.byref(pu), C.byref(n)), "gs_aux_device")
            return (time.perf_counter() - t0) / count * 1e6

        s.set_view_wire(views[0])
        loop_a(warmup)
        loop_b(max(warmup // 4, 8))
        a, b = [], []
        for _ in range(repeats):
            a.append(loop_a(iters))
            b.append(loop_b(iters))
        st = s.stats()
    a.sort()
    b.sort()
    med = lambda v: v[len(v) // 2]  # noqa: E731
    return {
        "workload": name, "width": W, "height": H, "gaussians": int(g.shape[0]), "iters": iters,
        "pairs_binned": st["n_pairs_binned"], "max_list": st["max_list"],
        "frame_us": [round(x, 1) for x in a], "frame_plus_aux_us": [round(x, 1) for x in b],
        "frame_us_median": round(med(a), 1), "frame_plus_aux_us_median": round(med(b), 1),
        "aux_us_median": round(med(b) - med(a), 1),
        "aux_us_spread": [round(b[0] - a[-1], 1), round(b[-1] - a[0], 1)],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--only", choices=["c3", "c5"], default=None)
    a = ap.parse_args()
    for name in ([a.only] if a.only else ["c3", "c5"]):
        print(json.dumps(measure(name, a.iters, a.repeats, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
