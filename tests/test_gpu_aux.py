"""GPU parity of the auxiliary planes (gs_read_aux32f, gs_read_aux_ids,
gs_aux_device, gs_read_aux_pixel; gs_aux_blend_kernel) against the references
of tests/auxref.py: floats bit for bit, counts and picks exactly.

Shapes (tests/auxref.py SHAPES): (a) 96x64, 16x16 tiles -- 24 whole tiles, a
list of 3 082 (> 2 048: the big-list sort); (b) 100x50, 32x20 tiles -- partial
tiles both ways, 640 pixels per tile (three pixel groups per workgroup), no
power-of-two divisions; "big" 160x90 with the whole scene -- a list of 27 201,
lazy on the second frame.  Every parity test first asserts on the reference
that the frame has content.
"""
import ctypes as C

import numpy as np
import pytest

import auxref
from test_gpu_parity import assert_same_bits

pytestmark = pytest.mark.gpu

PATH_BLEND_SORT, PATH_LAZY, PATH_BIN_DIRECT = 2, 8, 128
FLOATS = ("depth_sum", "coverage", "depth_median", "weight_max")
IDS = ("count", "pick")


def _splatter(r, **kw):
    from gaussian_splat_ipu_amd import camera
    from gaussian_splat_ipu_amd.splatter import GpuSplatter
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    W, H, TW, TH, sd = r["shape"]
    s = GpuSplatter(r["g"], TiledFramebuffer(W, H, TW, TH), device=0, **kw)
    s.set_view_wire(r["view"])
    s.set_projection_wire(r["proj"])
    s.update_focal_lengths(camera.FOV_DEFAULT, sd)
    return s


def _assert_content(name, planes):
    fr = auxref.fractions(planes)
    print(name, fr)
    if name == "a":
        assert fr["covered"] >= 0.25 and fr["two"] >= 0.15 and fr["median"] >= 0.15 and fr["stopped"] >= 0.08, fr
        assert fr["max_list"] > 2048, fr
    else:
        assert min(fr["covered"], fr["two"], fr["median"], fr["stopped"]) >= 0.05, fr


def _assert_planes(aux, planes, what="", rows=None):
    """aux (get_aux()) against the reference planes (their rows `rows`)."""
    for k in FLOATS + IDS:
        want = planes[k] if rows is None else rows(planes[k])
        if k in FLOATS:
            assert_same_bits(aux[k], want, f"{what} {k}")
        else:
            assert aux[k].dtype == np.uint32
            np.testing.assert_array_equal(aux[k], want, err_msg=f"{what} {k}")


def _frame_outputs(s):
    st = {k: v for k, v in s.stats().items() if k != "paths"}  # (a second frame may take other launches)
    return s.get_rgba(), s.get_frame_buffer(), s.get_histogram(), st


def _assert_outputs_equal(a, b, what):
    assert_same_bits(a[0], b[0], f"{what}: RGBA")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: BGR8")
    np.testing.assert_array_equal(a[2], b[2], err_msg=f"{what}: histogram")
    assert a[3] == b[3], (what, a[3], b[3])


def _assert_frame_is_the_oracles(s, r, band=None):
    from gaussian_splat_ipu_amd import camera
    from oracle import oracle as O

    W, H, TW, TH, sd = r["shape"]
    f = O.make_frame(r["view"], r["proj"], W, H, TW, TH, camera.FOV_DEFAULT, sd, band=band)
    ref = O.render(r["g"], f)
    assert_same_bits(s.get_rgba(), ref["rgba"], "RGBA")
    np.testing.assert_array_equal(s.get_frame_buffer(), ref["bgr"])
    np.testing.assert_array_equal(s.get_histogram(), ref["hist"])
    st = s.stats()
    assert st["n_pairs"] == ref["stats"]["n_pairs"] and st["max_list"] == ref["stats"]["max_list"]
    return f


@pytest.mark.parametrize("input_order", [False, True])
@pytest.mark.parametrize("name", ["a", "b"])
def test_whole_frame_parity(built, name, input_order):
    """All six planes; pick holds input indices under either device order."""
    r = auxref.reference(name)
    _assert_content(name, r["planes"])
    with _splatter(r, input_order=input_order) as s:
        s.execute()
        _assert_planes(s.get_aux(), r["planes"], name)
        dsum, cov = r["sub"]  # (the oracle's own composite of the substituted colours)
        aux = s.get_aux()
        assert_same_bits(aux["depth_sum"], dsum, "depth_sum, substitution")
        assert_same_bits(aux["coverage"], cov, "coverage, substitution")
        # get_depth: expected = depth_sum / coverage, NaN where nothing contributes
        d = s.get_depth()
        none = r["planes"]["count"] == 0
        assert np.isnan(d[none]).all() and (d[~none] < 0).all()
        assert_same_bits(d[~none], (dsum[~none] / cov[~none]).astype(np.float32), "expected depth")
        assert_same_bits(s.get_depth("median"), r["planes"]["depth_median"], "median depth")


def test_big_and_lazy_lists(built):
    """The whole scene at 160x90: 85 502 pairs, a list of 27 201.  The first
    frame sorts it inside the tile-sort launch, the second takes the lazy
    big-list path (sorted prefixes, the continuation), which leaves the lists
    unsorted in memory: the pass bins and sorts them again either way."""
    r = auxref.reference("big", False)
    dsum, cov = r["sub"]
    assert (cov > 0).mean() > 0.25
    with _splatter(r) as s:
        for k in range(2):
            s.execute()
            st = s.stats()
            assert st["max_list"] > 20000
            if k == 1:
                assert st["paths"] & PATH_LAZY, st["paths"]
            aux = s.get_aux()
            assert_same_bits(aux["depth_sum"], dsum, f"frame {k} depth_sum")
            assert_same_bits(aux["coverage"], cov, f"frame {k} coverage")
            assert ((aux["count"] > 0) == (cov > 0)).all()
        _assert_frame_is_the_oracles(s, r)


@pytest.mark.parametrize("interleaved", [False, True])
def test_bands_and_direct_binning(built, interleaved):
    """Two row bands of shape (a) (the sort in the blend, then direct binning,
    which needs the band cull's projection): each band's planes are its rows
    of the whole frame's, before and after the direct frames, and the frame
    after the pass is still the oracle's."""
    from gaussian_splat_ipu_amd import dist as gdist

    r = auxref.reference("a")
    _assert_content("a", r["planes"])
    for band in range(2):
        with _splatter(r, band_index=band, band_count=2, band_interleaved=interleaved, band_cull=True) as s:
            rows = lambda p: gdist.extract_band(p, s.fb, 2, band, interleaved)  # noqa: E731
            s.execute()
            assert s.stats()["paths"] & PATH_BLEND_SORT
            _assert_planes(s.get_aux(), r["planes"], f"band {band}", rows)
            for _ in range(4):
                s.execute()
                if s.stats()["paths"] & PATH_BIN_DIRECT:
                    break
            assert s.stats()["paths"] & PATH_BIN_DIRECT, s.stats()["paths"]
            _assert_planes(s.get_aux(), r["planes"], f"band {band} after a direct frame", rows)
            s.execute()
            if interleaved:
                # the oracle renders contiguous bands: compare with the whole frame's rows
                from oracle import oracle as O
                from gaussian_splat_ipu_amd import camera

                W, H, TW, TH, sd = r["shape"]
                ref = O.render(r["g"], O.make_frame(r["view"], r["proj"], W, H, TW, TH, camera.FOV_DEFAULT, sd))
                assert_same_bits(s.get_rgba(), rows(ref["rgba"]), "RGBA")
                np.testing.assert_array_equal(s.get_frame_buffer(), rows(ref["bgr"]))
                hist = ref["hist"].reshape(s.fb.tiles_down, s.fb.tiles_across)
                np.testing.assert_array_equal(s.get_histogram(), hist[s.fb.interleaved_tile_rows(2, band)].reshape(-1))
            else:
                ty0, ty1, _, _ = s.fb.band_rows(2)[band]
                _assert_frame_is_the_oracles(s, r, band=(ty0, ty1))
            _assert_planes(s.get_aux(), r["planes"], f"band {band}, last frame", rows)


def test_non_interference_under_poison(built, test_hook):
    """Every device buffer starts as 0xA5 bytes: the pass changes nothing a
    frame readback returns, reads nothing no stage wrote, and leaves the next
    frame and gs_read_bins as they were."""
    from gaussian_splat_ipu_amd import camera
    from oracle import oracle as O

    test_hook("debug_poison", 1)
    r = auxref.reference("a")
    _assert_content("a", r["planes"])
    W, H, TW, TH, sd = r["shape"]
    f = O.make_frame(r["view"], r["proj"], W, H, TW, TH, camera.FOV_DEFAULT, sd)
    rts, rlst = O.bin_lists(O.project(r["g"], f), f)
    with _splatter(r) as s:
        s.execute()
        before = _frame_outputs(s)
        ts, lst = s.get_bins()
        aux = s.get_aux()
        _assert_outputs_equal(_frame_outputs(s), before, "after get_aux")
        _assert_planes(aux, r["planes"], "poisoned")
        ts2, lst2 = s.get_bins()
        for got_ts, got_lst in ((ts, lst), (ts2, lst2)):
            np.testing.assert_array_equal(got_ts.astype(np.int64), rts)
            np.testing.assert_array_equal(got_lst, rlst)
        _assert_planes(s.get_aux(), r["planes"], "poisoned, after get_bins")
        s.execute()
        _assert_outputs_equal(_frame_outputs(s), before, "the next frame")
        _assert_frame_is_the_oracles(s, r)
        _assert_planes(s.get_aux(), r["planes"], "poisoned, next frame")


def test_invalidation_and_frames_in_flight(built):
    """The planes follow the frames: those of frame 1, then -- after a change
    of view and three frames enqueued without a sync -- those of the last."""
    from gaussian_splat_ipu_amd import camera
    from oracle import oracle as O

    r = auxref.reference("a")
    W, H, TW, TH, sd = r["shape"]
    view1 = camera.orbit_view(7)
    f1 = O.make_frame(view1, r["proj"], W, H, TW, TH, camera.FOV_DEFAULT, sd)
    planes1 = auxref.restate(O.project(r["g"], f1), f1)
    assert auxref.fractions(planes1)["covered"] >= 0.05  # (the other view shows the scene too)
    assert not np.array_equal(planes1["count"], r["planes"]["count"])
    with _splatter(r) as s:
        s.set_view_wire(view1)
        s.execute()
        _assert_planes(s.get_aux(), planes1, "frame 1")
        s.set_view_wire(r["view"])
        for _ in range(3):
            s.execute_async()
        _assert_planes(s.get_aux(), r["planes"], "after three frames in flight")
        _assert_frame_is_the_oracles(s, r)


def test_fast_exp_renderer_has_exact_planes(built):
    """GS_FLAG_FAST_EXP changes the colour frame's exponential only: the
    planes take the exact one."""
    r = auxref.reference("a")
    _assert_content("a", r["planes"])
    with _splatter(r, fast_exp=True) as s:
        s.execute()
        _assert_planes(s.get_aux(), r["planes"], "fast_exp")


def test_single_pixel_and_errors(built):
    """pick(x, y) equals the planes at ten seeded pixels (an uncovered one and
    one of a partial edge tile among them); a call before any frame and a
    pixel outside the frame are refused."""
    from gaussian_splat_ipu_amd._lib import GS_EINVAL, GsError

    r = auxref.reference("b")
    _assert_content("b", r["planes"])
    p = r["planes"]
    W, H, TW, TH, _ = r["shape"]
    empty = np.argwhere(p["count"] == 0)[0]
    edge = np.argwhere((p["count"] > 0) & ((np.arange(W)[None, :] >= W // TW * TW) |
                                           (np.arange(H)[:, None] >= H // TH * TH)))[0]
    rng = np.random.default_rng(12)
    pix = [tuple(empty), tuple(edge)] + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(8)]
    with _splatter(r) as s:
        with pytest.raises(GsError) as e:  # before any frame
            s.get_aux()
        assert e.value.status == GS_EINVAL and "no frame" in str(e.value)
        s.execute()
        for y, x in pix:
            got = s.pick(x, y)
            for k in FLOATS:
                assert_same_bits(np.float32(got[k]), p[k][y, x], f"pixel ({x}, {y}) {k}")
            assert (got["count"], got["pick"]) == (p["count"][y, x], p["pick"][y, x]), (x, y, got)
        y, x = empty
        assert s.pick(x, y)["pick"] == s.PICK_NONE and s.pick(x, y)["count"] == 0
        for x, y in ((W, 0), (0, H)):
            with pytest.raises(GsError) as e:
                s.pick(x, y)
            assert e.value.status == GS_EINVAL and "outside" in str(e.value)


def test_errors_of_bands_lattice_and_groups(built):
    """A pixel outside a row band, a lattice renderer and a row-band group
    (a group's aux frame is not provided) are refused with GS_EINVAL."""
    from gaussian_splat_ipu_amd._lib import GS_EINVAL, GsError
    from gaussian_splat_ipu_amd.splatter import GpuSplatter
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    ra = auxref.reference("a")
    with _splatter(ra, band_index=1, band_count=2) as s:  # rows 32..63
        s.execute()
        assert s.pick(5, 40)["count"] == ra["planes"]["count"][40, 5]
        with pytest.raises(GsError) as e:
            s.pick(5, 31)
        assert e.value.status == GS_EINVAL and "outside" in str(e.value)
    with _splatter(ra, lattice=True) as s:
        with pytest.raises(GsError) as e:
            s.get_aux()
        assert e.value.status == GS_EINVAL and "lattice" in str(e.value)
    Wa, Ha, TWa, THa, _ = ra["shape"]
    with GpuSplatter(ra["g"], TiledFramebuffer(Wa, Ha, TWa, THa), num_gpus=1, device_ids=[0]) as s:
        s.set_view_wire(ra["view"])
        s.set_projection_wire(ra["proj"])
        s.execute()
        for call in (s.get_aux, s.aux_device, lambda: s.pick(0, 0)):
            with pytest.raises(GsError) as e:
                call()
            assert e.value.status == GS_EINVAL and "group" in str(e.value)


def test_device_pointers(built):
    """gs_aux_device: the planes on the device equal the read-backs, and a
    second call on the same frame returns the same pointers."""
    r = auxref.reference("a")
    W, H = r["shape"][:2]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    with _splatter(r) as s:
        s.execute()
        pf, pu, n = s.aux_device()
        assert pf and pu and n == W * H
        f = np.empty((H, W, 4), np.float32)
        u = np.empty((H, W, 2), np.uint32)
        assert hip.hipMemcpy(f.ctypes.data, pf, f.nbytes, 2) == 0  # (hipMemcpyDeviceToHost)
        assert hip.hipMemcpy(u.ctypes.data, pu, u.nbytes, 2) == 0
        aux = s.get_aux()
        for i, k in enumerate(FLOATS):
            assert_same_bits(f[..., i], aux[k], k)
        for i, k in enumerate(IDS):
            np.testing.assert_array_equal(u[..., i], aux[k])
        assert s.aux_device() == (pf, pu, n)
        _assert_planes(aux, r["planes"], "device planes")
