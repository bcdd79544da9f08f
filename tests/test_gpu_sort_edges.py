"""The tile sorts at their thresholds: the scenes of tests/listscene.py (a
list of exactly L keys on either side of every length at which the sorts take
another path; runs of equal depth of 2, 15, 16, 17, 64 and 300 keys at the
lists' ends and across the segment, prefix and window boundaries; lists whose
longest run is exactly 15, 16 and 17, either side of kTieRun) through every
host of the sort, each frame against the CPU oracle bit for bit.
tests/test_listscene.py shows on the oracle that a swap of two adjacent list
entries at any of those indices changes the frame, so a sort that misplaces
one key cannot pass here.
"""
import numpy as np
import pytest

import auxref
import listscene
from test_gpu_parity import assert_same_bits

pytestmark = pytest.mark.gpu

PATH_BLEND_SORT, PATH_BLEND_PX2, PATH_LAZY, PATH_BIG_LISTS, PATH_BIN_DIRECT = 2, 4, 8, 16, 128
SCENES = ["lengths", "ties"]


def _splatter(sc, **kw):
    from gaussian_splat_ipu_amd.splatter import GpuSplatter
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    s = GpuSplatter(sc["g"], TiledFramebuffer(sc["W"], sc["H"], *sc["tile"]), device=0, **kw)
    s.set_view_wire(sc["view"])
    s.set_projection_wire(sc["proj"])
    s.update_focal_lengths(sc["fov"], 1.0)
    return s


def _assert_frame(s, ref, what, band_culled=False):
    """The renderer's last frame against the oracle's (listscene.reference)."""
    want, st = ref["render"], s.stats()
    print(what, {k: st[k] for k in ("paths", "n_big_tiles", "cont_lists", "cont_full_sorts", "bin_global")})
    if band_culled:  # (a band-culled renderer counts only the Gaussians it projected)
        assert st["n_rendered"] <= want["stats"]["n_rendered"], what
    else:
        assert st["n_rendered"] == want["stats"]["n_rendered"], what
    assert st["n_pairs"] == want["stats"]["n_pairs"], what
    assert st["max_list"] == want["stats"]["max_list"], what
    ts, lst = s.get_bins()
    np.testing.assert_array_equal(ts.astype(np.int64), ref["ts"], err_msg=what)
    np.testing.assert_array_equal(lst, ref["lst"], err_msg=what)
    np.testing.assert_array_equal(s.get_histogram(), want["hist"], err_msg=what)
    assert_same_bits(s.get_rgba(), want["rgba"], f"{what}: RGBA f32 framebuffer")
    np.testing.assert_array_equal(s.get_frame_buffer(), want["bgr"], err_msg=what)
    return st


@pytest.mark.parametrize("name", SCENES)
def test_whole_frame_three_frames(built, name):
    """One profiled renderer, 16x16 tiles.  Frame 1: the sort launch sorts
    every class of list, two-pixel blend lanes.  Frame 2: the big-list
    launches with lazy prefixes; late pixels of the serpentine outlive the
    prefix and the window, so lists continue and some are sorted in full.
    Frame 3: the same launches again, on the counters frame 2 left."""
    ref = listscene.reference(name)
    with _splatter(ref["scene"], profile=True) as s:
        s.execute()
        st = _assert_frame(s, ref, f"{name} frame 1")
        assert st["paths"] & PATH_BLEND_PX2 and not st["paths"] & (PATH_BIG_LISTS | PATH_LAZY), st["paths"]
        assert st["n_big_tiles"] == sum(L > 2048 for _, _, L, _ in ref["scene"]["spec"])
        s.execute()
        st = _assert_frame(s, ref, f"{name} frame 2")
        assert st["paths"] & PATH_BIG_LISTS and st["paths"] & PATH_LAZY, st["paths"]
        assert st["cont_lists"] > 0 and st["cont_full_sorts"] > 0, st
        s.execute()
        st = _assert_frame(s, ref, f"{name} frame 3")
        assert st["paths"] & PATH_BIG_LISTS and st["paths"] & PATH_LAZY, st["paths"]


@pytest.mark.parametrize("name", SCENES)
def test_whole_frame_global_binning(built, name):
    """bin_global: frame 2 takes the big-list sample sort in full (no lazy
    prefixes)."""
    ref = listscene.reference(name)
    with _splatter(ref["scene"], bin_global=True) as s:
        s.execute()
        st = _assert_frame(s, ref, f"{name} global frame 1")
        assert st["bin_global"] == 1 and not st["paths"] & PATH_BIG_LISTS
        s.execute()
        st = _assert_frame(s, ref, f"{name} global frame 2")
        assert st["paths"] & PATH_BIG_LISTS and not st["paths"] & PATH_LAZY, st["paths"]


@pytest.mark.parametrize("name", SCENES)
def test_whole_frame_32x20_tiles(built, name):
    """32x20 tiles: big lists without lazy lists or two-pixel lanes."""
    ref = listscene.reference(name, 32, 20)
    with _splatter(ref["scene"]) as s:
        s.execute()
        st = _assert_frame(s, ref, f"{name} 32x20 frame 1")
        assert not st["paths"] & (PATH_BLEND_PX2 | PATH_LAZY | PATH_BIG_LISTS), st["paths"]
        s.execute()
        st = _assert_frame(s, ref, f"{name} 32x20 frame 2")
        assert st["paths"] & PATH_BIG_LISTS and not st["paths"] & (PATH_BLEND_PX2 | PATH_LAZY), st["paths"]


@pytest.mark.parametrize("name", SCENES)
def test_whole_frame_input_order(built, name):
    """The Gaussians in input order on the device (no Morton order)."""
    ref = listscene.reference(name)
    with _splatter(ref["scene"], input_order=True) as s:
        s.execute()
        _assert_frame(s, ref, f"{name} input order")


def _band_frames(name, band, cull, want_direct):
    from gaussian_splat_ipu_amd.tiles import TiledFramebuffer

    sc = listscene.scene(name)
    ty0, ty1, _, _ = TiledFramebuffer(sc["W"], sc["H"], 16, 16).band_rows(2)[band]
    ref = listscene.reference(name, 16, 16, (ty0, ty1))
    big = ref["render"]["stats"]["max_list"] > 2048
    assert big == (name != "short")  # (a big list in either band of the two scenes)
    with _splatter(sc, band_index=band, band_count=2, band_cull=cull) as s:
        for k in (1, 2, 3):
            s.execute()
            st = _assert_frame(s, ref, f"{name} band {band} cull {cull} frame {k}", band_culled=cull)
            assert st["paths"] & PATH_BLEND_SORT, st["paths"]
            if k > 1 and big:  # (the big-list launches, lazy prefixes, next to the sort in the blend)
                assert st["paths"] & PATH_BIG_LISTS and st["paths"] & PATH_LAZY, st["paths"]
        if want_direct:
            assert st["paths"] & PATH_BIN_DIRECT, st["paths"]


@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("band", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_two_bands_three_frames(built, name, band, cull):
    """Bands 0 and 1 of a 2-way split (spec tiles in both), with and without
    the band cull: the sort inside the blend's workgroups on every frame;
    frames 2 and 3 sort the lists > 2048 keys in the big-list launches."""
    _band_frames(name, band, cull, want_direct=False)


@pytest.mark.parametrize("band", [0, 1])
def test_two_bands_direct_binning(built, band):
    """The direct binning as a host of the sort (gs_blend_direct sorts each
    tile from its fixed segment): the lists up to 2048 keys of both scenes,
    band-culled bands, frame 3."""
    _band_frames("short", band, True, want_direct=True)


@pytest.mark.xfail(strict=True, reason="choose_direct (gs_renderer.hip) refuses lazy frames, and a 16x16-tile band "
                   "whose last frame had a list > 2048 keys is lazy from its second frame on: such a band never "
                   "bins directly (frame 3: paths = 59, BIN_AGG | BLEND_SORT | LAZY | BIG_LISTS | PROJ_BAND)")
@pytest.mark.parametrize("band", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_band_with_big_lists_bins_directly_on_frame_3(built, name, band):
    """Frame 3 of a band-culled band of the two scenes must show
    GS_PATH_BIN_DIRECT.  It does not: see the reason.  The frames themselves
    are the oracle's (test_two_bands_three_frames)."""
    _band_frames(name, band, True, want_direct=True)


@pytest.mark.parametrize("name", SCENES)
def test_aux_planes(built, name):
    """get_aux() after whole-frame frames 1 and 2 (the second leaves the lazy
    lists unsorted in memory) against tests/auxref.py: the six planes of the
    restatement, depth_sum and coverage also against the oracle's own
    composite of the substituted colours."""
    from test_gpu_aux import _assert_planes

    ref = listscene.reference(name)
    planes = auxref.restate(ref["proj"], ref["frame"])
    _, dsum, cov = auxref.substitution(ref["scene"]["g"], ref["frame"])
    fr = auxref.fractions(planes)
    assert fr["covered"] > 0.02 and fr["two"] > 0.02 and fr["max_list"] > 2048, fr
    with _splatter(ref["scene"]) as s:
        for k in (1, 2):
            s.execute()
            if k == 2:
                assert s.stats()["paths"] & PATH_LAZY
            aux = s.get_aux()
            _assert_planes(aux, planes, f"{name} frame {k}")
            assert_same_bits(aux["depth_sum"], dsum, f"{name} frame {k} depth_sum, substitution")
            assert_same_bits(aux["coverage"], cov, f"{name} frame {k} coverage, substitution")
