"""CPU checks of tests/listscene.py on the oracle, for every scene that
tests/test_gpu_sort_edges.py renders: the lists have exactly the stated
lengths and runs of equal depth, and -- what keeps the GPU tests from being
blind -- a swap of two adjacent list entries at every boundary index changes
the blended frame.  The oracle's projection of these scenes (and of the
w != 1 scene of tests/test_gpu_branches.py) is pinned by tests/pyref.py.
"""
import ctypes as C

import numpy as np
import pytest

import listscene
import pyref

SCENES = [("lengths", 16, 16), ("ties", 16, 16), ("lengths", 32, 20), ("ties", 32, 20), ("short", 16, 16)]
BOUNDARIES = (62, 63, 64, 126, 127, 128, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024, 2046, 2047, 2048,
              2558, 2559, 2560, 4094, 4095, 4096)
_FP = C.POINTER(C.c_float)


def _runs_of(z):
    """[(start, length)] of the maximal groups of adjacent equal values."""
    cut = np.flatnonzero(np.concatenate(([True], z[1:] != z[:-1], [True])))
    return [(int(a), int(b - a)) for a, b in zip(cut[:-1], cut[1:])]


def _tile_lists(ref):
    sc = ref["scene"]
    tiles_x = sc["W"] // sc["tile"][0]
    return {(tx, ty): (int(ref["ts"][ty * tiles_x + tx]), L, runs) for tx, ty, L, runs in sc["spec"]}


def _blend(ref, lst):
    from oracle import oracle as O

    sc = ref["scene"]
    g = np.ascontiguousarray(sc["g"])
    lst = np.ascontiguousarray(lst, np.uint32)
    rgba = np.zeros((sc["H"], sc["W"], 4), np.float32)
    rc = O.lib().or_blend(g.ctypes.data_as(_FP), ref["proj"].ctypes.data, C.byref(ref["frame"]),
                          ref["ts"].ctypes.data_as(C.POINTER(C.c_int64)), lst.ctypes.data_as(C.POINTER(C.c_uint32)),
                          rgba.ctypes.data_as(_FP), 0)
    assert rc == 0
    return rgba


@pytest.mark.parametrize("name,tw,th", SCENES)
def test_exact_lists_and_runs(built, name, tw, th):
    ref = listscene.reference(name, tw, th)
    sc, p, ts, lst = ref["scene"], ref["proj"], ref["ts"], ref["lst"]
    n = sc["g"].shape[0]
    assert n == sum(L for _, _, L, _ in sc["spec"])
    tiles_x, tiles_y = sc["W"] // tw, sc["H"] // th
    assert tiles_x % 2 == 1 and tiles_y % 2 == 1
    # every Gaussian is rendered, in one tile, with the radius the placement assumes
    assert (p["rendered"] != 0).all()
    r = p["rect"]
    assert (r[:, 0] == r[:, 2]).all() and (r[:, 1] == r[:, 3]).all()
    assert (p["radius"] == 3).all()
    want = np.zeros(tiles_x * tiles_y, np.int64)
    for tx, ty, L, _ in sc["spec"]:
        want[ty * tiles_x + tx] = L
    np.testing.assert_array_equal(np.diff(ts), want)
    st = ref["render"]["stats"]
    assert st["max_list"] == max(L for _, _, L, _ in sc["spec"])
    assert (st["max_list"] <= 2048) == (name == "short")
    assert st["n_rendered"] == n and st["n_pairs"] == n
    np.testing.assert_array_equal(ref["render"]["hist"], want)
    # spec tiles lie in both bands of a 2-way split
    half = -(-tiles_y // 2)
    assert {ty < half for _, ty, _, _ in sc["spec"]} == {True, False}
    # the intended runs, and the list order (clip z, input index)
    two_binades = False
    for (tx, ty), (s, L, runs) in _tile_lists(ref).items():
        ids = lst[s:s + L]
        z = p["clip_z"][ids]
        assert (z < 0).all() and (np.diff(z) >= 0).all()
        got = _runs_of(z)
        for a, m in got:
            assert (np.diff(ids[a:a + m].astype(np.int64)) > 0).all(), "a run follows its input indices"
        if runs == "ulp":
            lens = [m for _, m in got]
            d = np.diff(np.unique(z).view(np.int32))
            assert max(lens) >= 2 and (np.abs(d) == 1).any(), (lens, d)  # ties, and keys one ulp apart
            continue
        assert [m for _, m in got] == ([1] * L if runs is None else list(runs)), (tx, ty, L)
        if L > 2048:  # (clip z < 0: frexp's exponent is the binade)
            e = np.frexp(z)[1]
            two_binades |= e.min() != e.max()
    if name == "lengths":
        assert two_binades, "no big list spans two binades of clip z"
        assert sorted(L for _, _, L, _ in sc["spec"]) == sorted(listscene.LENGTHS)


def _swap_indices(L, z):
    ks = {0, L - 2} | {k for k in BOUNDARIES if 0 <= k <= L - 2}
    for a, m in _runs_of(z):
        if m >= 2:
            ks |= {a, a + (m - 2) // 2, a + m - 2}
    return sorted(k for k in ks if 0 <= k <= L - 2)


@pytest.mark.parametrize("name,tw,th", SCENES)
def test_adjacent_swaps_change_the_frame(built, name, tw, th):
    """Mutation sensitivity: for every target tile, entries (k, k + 1) of its
    list swapped, for k at the list's ends, around every threshold of the
    sorts and at the first, a middle and the last pair of every tie run.
    Each swap must change at least one RGBA bit of the tile (one blend serves
    one swap of every tile: the tiles are independent)."""
    ref = listscene.reference(name, tw, th)
    sc, p, lst = ref["scene"], ref["proj"], ref["lst"]
    base = _blend(ref, lst)
    # the unedited lists blend to the oracle's frame
    np.testing.assert_array_equal(base.view(np.uint32), ref["render"]["rgba"].view(np.uint32))
    todo = {}
    for (tx, ty), (s, L, _) in _tile_lists(ref).items():
        if L >= 2:
            todo[tx, ty] = (s, _swap_indices(L, p["clip_z"][lst[s:s + L]]))
    total, undetected = 0, []
    for rnd in range(max(len(ks) for _, ks in todo.values())):
        edit = lst.copy()
        done = []
        for cell, (s, ks) in todo.items():
            if rnd < len(ks):
                k = s + ks[rnd]
                edit[k], edit[k + 1] = lst[k + 1], lst[k]
                done.append((cell, ks[rnd]))
        out = _blend(ref, edit)
        for (tx, ty), k in done:
            a = out[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].view(np.uint32)
            b = base[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].view(np.uint32)
            total += 1
            if (a == b).all():
                undetected.append((tx, ty, k))
    print(f"{name} {tw}x{th}: {total} swaps, {len(undetected)} undetected")
    assert total > 100 and not undetected, undetected


def _assert_pyref_projection(a, view, proj, W, H, tw, th, fov, scale_div):
    from oracle import oracle as O

    got = O.project(a, O.make_frame(view, proj, W, H, tw, th, fov, scale_div))
    want = pyref.project(a, view, proj, W, H, tw, th, fov, scale_div)
    for i, r in enumerate(want):
        assert got["rendered"][i] == r["rendered"], i
        np.testing.assert_array_equal(got["mean2d"][i].view(np.uint32), np.float32(r["mean2d"]).view(np.uint32))
        np.testing.assert_array_equal(got["conic"][i].view(np.uint32), np.float32(r["conic"]).view(np.uint32))
        assert got["clip_z"][i] == r["clip_z"] and got["radius"][i] == r["radius"], i
        if r["rect"] is not None:
            assert tuple(got["rect"][i]) == r["rect"], i
        elif got["rendered"][i]:
            assert got["rect"][i][0] > got["rect"][i][2], i
    return got


@pytest.mark.parametrize("name,tw,th", [SCENES[0], SCENES[1], SCENES[2], SCENES[4]])
def test_projection_matches_python_restatement(built, name, tw, th):
    """A 300-Gaussian sub-scene (evenly spaced input indices, which the
    shuffle spreads over the tiles): tests/pyref.py's float32 restatement
    gives the oracle's projection records bit for bit."""
    sc = listscene.scene(name, tw, th)
    g = sc["g"]
    pick = np.linspace(0, g.shape[0] - 1, 300).astype(np.int64)
    _assert_pyref_projection(g[pick], sc["view"], sc["proj"], sc["W"], sc["H"], tw, th, sc["fov"], 1.0)


def test_w_scene_projection_matches_python_restatement(built):
    """The scene with mean w in {0.5, 1, 2} (tests/test_gpu_branches.py): the
    oracle's arithmetic on it is pinned by nothing else.  Every 40th Gaussian
    (500), all three w among the rendered ones."""
    sc = listscene.w_scene()
    a = sc["g"][::40]
    got = _assert_pyref_projection(a, sc["view"], sc["proj"], sc["W"], sc["H"], 16, 16, sc["fov"], 1.0)
    ok = (got["rendered"] != 0) & (got["rect"][:, 0] <= got["rect"][:, 2])
    assert set(np.unique(a[ok, 3]).tolist()) == {0.5, 1.0, 2.0}
