"""References for the auxiliary planes (include/gsplat.h, "auxiliary planes"),
both built on the unchanged CPU oracle:

1. ``substitution``: the oracle composites colour[0:3] like it composites
   anything, so a copy of the scene with colour = (clip z, 1, 0) renders
   (depth_sum, coverage) into the R and G channels with the oracle's own bits.
2. ``restate``: a numpy restatement of renderTile's walk (oracle/gs_oracle.cpp,
   or_blend) for all six planes: per tile a loop over its depth-sorted list,
   float32 element-wise arithmetic over the tile's pixels, the exponential
   taken from the oracle (or_expf).  Its depth_sum and coverage are checked
   against (1) bit for bit (test_aux_reference.py).

``reference(name)`` computes a shape's scene, frame and both references once
per process.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PC12 = os.path.join(GOLDEN, "point_cloud_12.ply")
F32 = np.float32
PICK_NONE = 0xFFFFFFFF
PLANES = ("depth_sum", "coverage", "depth_median", "weight_max", "count", "pick")

# name: (width, height, tile width, tile height, fxy[1], every n-th Gaussian of point_cloud_12)
SHAPES = {
    "a": (96, 64, 16, 16, 1.0, 10),    # whole 16x16 tiles, a list longer than 2048
    "b": (100, 50, 32, 20, 0.1, 10),   # partial tiles both ways, 640-pixel tiles, no power of two
    "big": (160, 90, 16, 16, 1.0, 1),  # the whole scene: a list of 27 201 (substitution only)
}


def clip_z_colours(g, f):
    """(projection, scene copy with colour[0:3] = (clip z, 1, 0)); the opacity
    logit colour[3] stays: the projection reads it."""
    from oracle import oracle as O

    p = O.project(g, f)
    a = np.ascontiguousarray(g).view(F32).reshape(-1, 16).copy()
    z = np.where(p["rendered"] != 0, p["clip_z"], 0).astype(F32)
    z = np.nan_to_num(z, nan=0.0, posinf=0.0, neginf=0.0)
    a[:, 4] = z
    a[:, 5] = 1
    a[:, 6] = 0
    return p, a


def substitution(g, f):
    """(projection, depth_sum, coverage) with the oracle's own blend."""
    from oracle import oracle as O

    p, a = clip_z_colours(g, f)
    rgba = O.render(a, f)["rgba"]
    return p, np.ascontiguousarray(rgba[..., 0]), np.ascontiguousarray(rgba[..., 1])


def restate(p, f):
    """The six planes of the whole frame f (H x W each) from the projection p,
    plus ``stopped`` (the pixels whose walk ended at T' < 1e-4) and
    ``max_list``."""
    from oracle import oracle as O

    vexp = np.vectorize(O.expf, otypes=[F32])
    W, H, TW, TH = f.width, f.height, f.tile_w, f.tile_h
    ts, lst = O.bin_lists(p, f)
    tiles_x = -(-W // TW)
    out = {
        "depth_sum": np.zeros((H, W), F32),
        "coverage": np.zeros((H, W), F32),
        "depth_median": np.zeros((H, W), F32),
        "weight_max": np.zeros((H, W), F32),
        "count": np.zeros((H, W), np.uint32),
        "pick": np.full((H, W), PICK_NONE, np.uint32),
        "stopped": np.zeros((H, W), bool),
    }
    for t in range(len(ts) - 1):
        tx, ty = t % tiles_x, t // tiles_x
        ys, xs = np.mgrid[ty * TH:min((ty + 1) * TH, H), tx * TW:min((tx + 1) * TW, W)]
        px, py = xs.ravel().astype(F32), ys.ravel().astype(F32)
        n = px.size
        T = np.ones(n, F32)
        d, a_, m, wm = (np.zeros(n, F32) for _ in range(4))
        have_m = np.zeros(n, bool)
        c = np.zeros(n, np.uint32)
        pk = np.full(n, PICK_NONE, np.uint32)
        done = np.zeros(n, bool)
        for k in range(ts[t], ts[t + 1]):
            gi = lst[k]
            q = p[gi]
            con = q["conic"]
            if con[3] == 0:
                continue
            dx = (q["mean2d"][0] - px).astype(F32)
            dy = (q["mean2d"][1] - py).astype(F32)
            power = (F32(-0.5) * (con[0] * dx * dx + con[2] * dy * dy) - con[1] * dx * dy).astype(F32)
            act = ~done & ~(power > 0)
            if not act.any():
                continue
            v = np.zeros(n, F32)
            v[act] = con[3] * vexp(power[act])
            alpha = np.where(v < F32(0.99), v, F32(0.99)).astype(F32)
            act &= ~(alpha < F32(1.0) / F32(255.0))
            tT = (T * (F32(1) - alpha)).astype(F32)
            stop = act & (tT < F32(0.0001))
            done |= stop
            act &= ~stop
            z = q["clip_z"]
            w = (alpha * T).astype(F32)
            d = np.where(act, (d + (z * alpha) * T).astype(F32), d)
            a_ = np.where(act, (a_ + (F32(1) * alpha) * T).astype(F32), a_)
            better = act & ((c == 0) | (w > wm))
            wm = np.where(better, w, wm)
            pk = np.where(better, np.uint32(gi), pk)
            newmed = act & ~have_m & (T >= F32(0.5)) & (tT < F32(0.5))
            m = np.where(newmed, z, m)
            have_m |= newmed
            c = c + act.astype(np.uint32)
            T = np.where(act, tT, T)
        sl = (ys.ravel(), xs.ravel())
        for key, val in (("depth_sum", d), ("coverage", a_), ("depth_median", m), ("weight_max", wm), ("count", c),
                         ("pick", pk), ("stopped", done)):
            out[key][sl] = val
    out["max_list"] = int(np.diff(ts).max()) if len(ts) > 1 else 0
    return out


def fractions(r):
    """The reference's own content: what a parity test asserts before it
    compares, so that it cannot pass on an empty frame."""
    return {
        "covered": float((r["count"] > 0).mean()),
        "two": float((r["count"] >= 2).mean()),
        "median": float((r["depth_median"] != 0).mean()),
        "stopped": float(r["stopped"].mean()),
        "max_list": r["max_list"],
    }


@functools.lru_cache(maxsize=None)
def scene_of(every):
    from gaussian_splat_ipu_amd import scene

    g, bb = scene.prepare_scene(scene.load_ply(PC12))
    return np.ascontiguousarray(g[::every]), bb


@functools.lru_cache(maxsize=None)
def reference(name, with_restatement=True):
    """dict(g, bb, view, proj, frame, shape, sub=(depth_sum, coverage), planes)."""
    from gaussian_splat_ipu_amd import camera
    from oracle import oracle as O

    W, H, TW, TH, sd, every = SHAPES[name]
    g, bb = scene_of(every)
    view, proj = camera.headless(bb, W, H)
    f = O.make_frame(view, proj, W, H, TW, TH, camera.FOV_DEFAULT, sd)
    p, dsum, cov = substitution(g, f)
    return {
        "g": g, "bb": bb, "view": view, "proj": proj, "frame": f, "shape": (W, H, TW, TH, sd),
        "sub": (dsum, cov),
        "planes": restate(p, f) if with_restatement else None,
    }
