"""Branches of the frame path that the parity scenes never take with data
that could tell right from wrong, each against the CPU oracle bit for bit:
mean w != 1 (the projection's w loads, the band cull's "never culled" record),
tile grids past 256 columns or rows (no 8-bit rectangles), past 40 960 tiles
(no wide emit, so no pair cull) and past 81 920 tiles (forced global binning),
power-of-two fxy[1] other than 1 (the exact divisions by shifts), SH degrees 1
and 2, and fields of view other than the default (the 1.3 tan(fov / 2) clamp).

Unless noted the scene is scene.synthetic with 20 000 Gaussians at 640x360,
16x16 tiles.  Every test first asserts on the oracle that the frame has the
content the branch needs.
"""
import numpy as np
import pytest

import listscene
from test_gpu_parity import _assert_parity, _frame_pair, assert_same_bits

pytestmark = pytest.mark.gpu

W0, H0 = 640, 360


def _synthetic(n=20000, seed=7, sh_degree=0, stretch_x=1.0):
    """(ply, g, bb): the seeded scene, its bounding box stretched along x, the
    screen's horizontal (the headless camera keeps its vertical field of view
    and takes the horizontal one from the frame's aspect ratio: a box of the
    frame's shape fills a frame 257 tiles wide and 3 high, or 3 wide and 257
    high, so every tile column or row has lists)."""
    from gaussian_splat_ipu_amd import scene

    d = scene.SynthSpec()
    ply = scene.synthetic(scene.SynthSpec(
        n=n, seed=seed, sh_degree=sh_degree,
        bb_min=(d.bb_min[0] * stretch_x,) + tuple(d.bb_min[1:]), bb_max=(d.bb_max[0] * stretch_x,) + tuple(d.bb_max[1:])))
    g, bb = scene.prepare_scene(ply)
    return ply, g, bb


def _a16(g):
    return np.ascontiguousarray(g).view(np.float32).reshape(-1, 16)


def _band(W, H, TW, TH, band_count, band_index):
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    ty0, ty1, _, _ = TiledFramebuffer(W, H, TW, TH).band_rows(band_count)[band_index]
    return ty0, ty1


def _assert_band_projection(s, g, f):
    """A band's readback records (all but the rectangle, which the oracle
    gives relative to the band): every live Gaussian, culled or not."""
    from oracle import oracle as O

    p, gp = O.project(g, f), s.get_projected()
    live = _a16(g)[:, 15] > 0
    assert_same_bits(gp[live, 0:2], p["mean2d"][live], "mean2d")
    assert_same_bits(gp[live, 2:6], p["conic"][live], "conic")
    assert_same_bits(gp[live, 6], p["clip_z"][live], "clip z")
    assert_same_bits(gp[live, 7], p["radius"][live], "radius")


# ---------------------------------------------------------------- mean w != 1
def _assert_w_content(sc, g=None):
    from oracle import oracle as O

    g = sc["g"] if g is None else g
    f = O.make_frame(sc["view"], sc["proj"], W0, H0, 16, 16, sc["fov"], 1.0)
    st = O.render(g, f, want_rgba=False)["stats"]
    assert st["n_rendered"] > 1000 and st["n_pairs"] > 10000, st
    p = O.project(g, f)
    ok = (p["rendered"] != 0) & (p["rect"][:, 0] <= p["rect"][:, 2])
    assert {0.5, 1.0, 2.0} == set(np.unique(_a16(g)[ok, 3]).tolist())


@pytest.mark.parametrize("host", ["whole", "band0", "band1"])
def test_mean_w_not_one(built, host):
    """Mean w drawn from {0.5, 1, 2}: a whole frame, and the two bands of a
    2-way split with the band cull (a Gaussian with w != 1 is never culled)."""
    sc = listscene.w_scene()
    _assert_w_content(sc)
    if host == "whole":
        s, f = _frame_pair(sc["g"], sc["view"], sc["proj"], W0, H0, 16, 16, 1.0)
        _assert_parity(s, f, sc["g"])
    else:
        from gaussian_splat_ipu_amd.splatter import GpuSplatter
        from gaussian_splat_ipu_amd.tiles import TiledFramebuffer
        from oracle import oracle as O

        band = int(host[-1])
        s = GpuSplatter(sc["g"], TiledFramebuffer(W0, H0, 16, 16), device=0, band_index=band, band_count=2,
                        band_cull=True)
        s.set_view_wire(sc["view"])
        s.set_projection_wire(sc["proj"])
        s.update_focal_lengths(sc["fov"], 1.0)
        s.execute()
        f = O.make_frame(sc["view"], sc["proj"], W0, H0, 16, 16, sc["fov"], 1.0, band=_band(W0, H0, 16, 16, 2, band))
        ref = _assert_parity(s, f, sc["g"], check_proj=False, band_culled=True)
        assert ref["stats"]["n_pairs"] > 3000
        assert s.stats()["n_rendered"] < ref["stats"]["n_rendered"]  # (the cull is at work)
        _assert_band_projection(s, sc["g"], f)
    s.close()


def test_mean_w_not_one_with_sh(built):
    """... and with the view-dependent colour of degree 3 (the projection
    that evaluates SH reads the means' w too)."""
    from gaussian_splat_ipu_amd import scene
    from oracle import oracle as O

    sc = listscene.w_scene(3)
    dc, rest = scene.sh_arrays(sc["ply"])
    gsh = _a16(O.sh_colours(sc["g"], dc, rest, 3, sc["view"]))
    assert not np.array_equal(gsh[:, 4:7], sc["g"][:, 4:7])
    _assert_w_content(sc, gsh)
    s, f = _frame_pair(sc["g"], sc["view"], sc["proj"], W0, H0, 16, 16, 1.0)
    s.set_sh(dc, rest, 3)
    s.execute()
    _assert_parity(s, f, gsh)
    s.close()


# ---------------------------------------------------------------- tile grids
def _grid_scene(W, H, TW, TH, reach=None):
    """The scene stretched to the frame's shape and its camera; with
    ``reach`` = (axis, tile) one Gaussian near that tile column / row is
    enlarged until its rectangle starts before the tile and ends on it."""
    from gaussian_splat_ipu_amd import camera
    from oracle import oracle as O

    _, g, bb = _synthetic(stretch_x=(W / H) / (W0 / H0))
    view, proj = camera.headless(bb, W, H)
    a = _a16(g).copy()
    f = O.make_frame(view, proj, W, H, TW, TH, camera.FOV_DEFAULT, 1.0)
    if reach is not None:
        axis, tile = reach
        p = O.project(a, f)
        ok = (p["rendered"] != 0) & (p["rect"][:, 0] <= p["rect"][:, 2])
        edge = tile * (TW, TH)[axis]
        i = int(np.flatnonzero(ok)[np.argmin(np.abs(p["mean2d"][ok, axis] - edge))])
        a[i, 12:15] = a[:, 12:15].max() + 0.5
        a[i, 7] = 0.9
        r = O.project(a, f)["rect"][i]
        assert r[axis] < tile and r[axis + 2] == tile, r
    return a, view, proj, f


def _assert_spread(f, a, axis, first_past):
    """Every sixteenth of the grid along ``axis`` has lists, and so have the
    tile columns / rows from ``first_past`` on."""
    from oracle import oracle as O

    tiles_x, tiles_y = -(-f.width // f.tile_w), -(-f.height // f.tile_h)
    hist = O.render(a, f, want_rgba=False)["hist"].reshape(tiles_y, tiles_x)
    along = hist.sum(axis=axis).astype(np.int64)  # per column (axis 0) or per row (axis 1)
    assert all(part.sum() > 0 for part in np.array_split(along, 16)), along
    if first_past is not None:
        assert along[first_past:].sum() > 0, along[first_past:]


@pytest.mark.parametrize("W,H,T,host", [
    (4096, 48, 16, "whole"), (4112, 48, 16, "whole"), (4112, 48, 16, "reach"), (2056, 32, 8, "whole"),
    (48, 4112, 16, "whole"), (48, 4112, 16, "band1")])
def test_tile_grid_256_257(built, W, H, T, host):
    """256 and 257 tile columns (16x16 and 8x8 tiles) and 257 tile rows: past
    256 the binning keeps 32-bit rectangles.  "reach": one Gaussian whose
    rectangle ends on tile column 256.  Band 1 of two of the tall frame has
    129 rows (8-bit rectangles again) of a 257-row grid."""
    from oracle import oracle as O

    axis = 0 if W > H else 1
    n_tiles = -(-(W, H)[axis] // T)
    a, view, proj, f = _grid_scene(W, H, T, T, reach=(0, 256) if host == "reach" else None)
    _assert_spread(f, a, axis, 256 if n_tiles > 256 else None)
    if host == "band1":
        s, fb = _frame_pair(a, view, proj, W, H, T, T, 1.0, band_count=2, band_index=1)
        assert O.render(a, fb, want_rgba=False)["stats"]["n_pairs"] > 1000
        _assert_parity(s, fb, a, check_proj=False)
    else:
        s, _ = _frame_pair(a, view, proj, W, H, T, T, 1.0)
        st = s.stats()
        assert st["n_pairs_binned"] < st["n_pairs"]  # (the pair cull is on)
        _assert_parity(s, f, a)
    s.close()


def test_more_than_40960_tiles(built):
    """2056x1280 at 8x8: 41 120 tiles, past the wide emit's LDS cursors: the
    chunked binning without the pair cull (every pair of the reference lists
    is binned)."""
    a, view, proj, f = _grid_scene(2056, 1280, 8, 8)
    _assert_spread(f, a, 0, 256)
    s, _ = _frame_pair(a, view, proj, 2056, 1280, 8, 8, 1.0)
    st = s.stats()
    assert st["n_tiles"] == 257 * 160 and st["bin_global"] == 0
    assert st["n_pairs_binned"] == st["n_pairs"] > 100000, st
    _assert_parity(s, f, a)
    s.close()


def test_more_than_81920_tiles(built):
    """2624x2000 at 8x8: 82 000 tiles, past one CU's LDS histogram: the
    global-atomic binning although the flag was not set."""
    a, view, proj, f = _grid_scene(2624, 2000, 8, 8)
    _assert_spread(f, a, 0, 256)
    s, _ = _frame_pair(a, view, proj, 2624, 2000, 8, 8, 1.0)
    st = s.stats()
    assert st["n_tiles"] == 328 * 250 and st["bin_global"] == 1, st
    _assert_parity(s, f, a)
    s.close()


# ---------------------------------------------------------------- fxy[1] a power of two other than 1
@pytest.mark.parametrize("cov_cache", [-1, 0])
@pytest.mark.parametrize("host", ["whole", "band1"])
@pytest.mark.parametrize("scale_div", [0.5, 2.0, 0.25])
def test_power_of_two_scale_divisor(built, test_hook, scale_div, host, cov_cache):
    """fxy[1] in {0.5, 2, 0.25}: the log-scales' division done as an exact
    multiplication (with 1.0 a multiplication mistaken for a division is
    invisible), with the cached 3D covariances and without them, a whole
    frame and band 1 of two with the band cull."""
    from gaussian_splat_ipu_amd import camera
    from gaussian_splat_ipu_amd.splatter import GpuSplatter
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer
    from oracle import oracle as O

    test_hook("cov_cache", cov_cache)
    _, g, bb = _synthetic()
    view, proj = camera.headless(bb, W0, H0)
    if host == "whole":
        s, f = _frame_pair(g, view, proj, W0, H0, 16, 16, scale_div)
        ref = _assert_parity(s, f, g)
    else:
        s = GpuSplatter(g, TiledFramebuffer(W0, H0, 16, 16), device=0, band_index=1, band_count=2, band_cull=True)
        s.set_view_wire(view)
        s.set_projection_wire(proj)
        s.update_focal_lengths(camera.FOV_DEFAULT, scale_div)
        s.execute()
        f = O.make_frame(view, proj, W0, H0, 16, 16, camera.FOV_DEFAULT, scale_div, band=_band(W0, H0, 16, 16, 2, 1))
        ref = _assert_parity(s, f, g, check_proj=False, band_culled=True)
        assert s.stats()["n_rendered"] < ref["stats"]["n_rendered"]  # (the cull is at work)
        _assert_band_projection(s, g, f)
    assert ref["stats"]["n_pairs"] > 3000
    s.close()


# ---------------------------------------------------------------- SH degrees 1 and 2
@pytest.mark.parametrize("degree", [1, 2])
def test_sh_degree(built, degree):
    """Degrees 1 and 2 of the view-dependent colour, one renderer, two views."""
    from gaussian_splat_ipu_amd import camera, scene
    from oracle import oracle as O

    ply, g, bb = _synthetic(sh_degree=3)
    dc, rest = scene.sh_arrays(ply)
    view, proj = camera.headless(bb, W0, H0)
    s, _ = _frame_pair(g, view, proj, W0, H0, 16, 16, 1.0)
    s.set_sh(dc, rest, degree)
    seen = []
    for v in (view, camera.orbit_view(20)):
        gsh = O.sh_colours(g, dc, rest, degree, v)
        seen.append(_a16(gsh)[:, 4:7].copy())
        s.set_view_wire(v)
        s.execute()
        ref = _assert_parity(s, O.make_frame(v, proj, W0, H0, 16, 16, camera.FOV_DEFAULT, 1.0), gsh)
        assert ref["stats"]["n_pairs"] > 10000
    # the colours depend on the degree and on the view
    assert not np.array_equal(seen[0], seen[1])
    assert not np.array_equal(seen[0], _a16(O.sh_colours(g, dc, rest, 3, view))[:, 4:7])
    assert not np.array_equal(seen[0], _a16(g)[:, 4:7])
    s.close()


# ---------------------------------------------------------------- field of view
@pytest.mark.parametrize("deg", [20.0, 70.0])
def test_field_of_view(built, deg):
    """fov of 20 and 70 degrees (camera and focal lengths).  At 20 degrees
    some rendered Gaussians lie outside 1.3 tan(fov / 2) in x or y: the
    projection's clamped branch."""
    from gaussian_splat_ipu_amd import camera
    from oracle import oracle as O

    fov = camera.radians(deg)
    _, g, bb = _synthetic()
    view, proj = camera.headless(bb, W0, H0, fov)
    f = O.make_frame(view, proj, W0, H0, 16, 16, fov, 1.0)
    if deg == 20.0:
        p = O.project(g, f)
        ok = (p["rendered"] != 0) & (p["rect"][:, 0] <= p["rect"][:, 2])
        a = _a16(g).astype(np.float64)
        mvp = np.asarray(proj, np.float64).reshape(4, 4) @ np.asarray(view, np.float64).reshape(4, 4)
        t = np.c_[a[:, 0:3], np.ones(len(a))] @ mvp.T
        lim = 1.3 * np.tan(0.5 * fov)
        out = ok & ((np.abs(t[:, 0] / t[:, 2]) > lim * 1.001) | (np.abs(t[:, 1] / t[:, 2]) > lim * 1.001))
        assert out.sum() > 10, out.sum()
    s, _ = _frame_pair(g, view, proj, W0, H0, 16, 16, 1.0, fov=fov)
    ref = _assert_parity(s, f, g)
    assert ref["stats"]["n_pairs"] > 10000
    s.close()
