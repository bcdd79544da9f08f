"""Deterministic scenes whose tile lists have exactly the stated lengths and
runs of equal depth, so that a test can put a list on either side of every
threshold of the tile sorts (tests/test_listscene.py checks the construction
on the CPU oracle, tests/test_gpu_sort_edges.py renders the scenes).

``build(spec, ...)``: ``spec`` is a list of ``(tile_x, tile_y, L, runs)``.
Tile (tile_x, tile_y) receives a list of exactly L Gaussians and no other tile
receives anything.  ``runs`` is

* ``None``: L distinct depths;
* a list of group lengths in list order that sums to L: each group is one
  exactly equal clip z (1 = a depth of its own), see ``partition``;
* ``"ulp"``: L consecutive float32 world z around the value at which the
  product with the projection's z scale crosses 1.0 -- below it consecutive
  z give clip z one ulp apart, above it pairs of them collide.

Camera: the view only translates along z (by -2) and the projection is a
glm-style perspective (near 1, far 100), so clip z depends on world z alone.
The oracle renders clip z < 0 (a distance d < ~1.98) and its radii grow as
clip z nears 0; d stays in [1.05, 1.5] (the "ulp" tile: d ~ 1.02), where
log-scales of -8 give a radius of 3 px.  A tile's Gaussians, in list order
(depth, then input index), sit along a serpentine walk over the tile's
interior, 4.25 px from its edges: neighbours in the list are neighbours on
screen and share pixels, so a swap of two adjacent list entries changes the
blended tile.
"""
import functools
import math

import numpy as np

F32 = np.float32
FOV = float(F32(40.0) * F32(0.01745329251994329576923690768489))  # (camera.FOV_DEFAULT)
NEAR, FAR = 1.0, 100.0
D_MIN, D_MAX = 1.05, 1.5
MARGIN = 4.25
LOG_SCALE = -8.0

VIEW = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2, 0, 0, 0, 1])


def projection(W, H, fov=FOV):
    t = math.tan(0.5 * fov)
    n, f = NEAR, FAR
    return np.float32([1.0 / (W / H * t), 0, 0, 0, 0, 1.0 / t, 0, 0,
                       0, 0, -(f + n) / (f - n), -2.0 * f * n / (f - n), 0, 0, -1, 0])


def clip_z(zw, proj):
    """Clip z of world z (float32 array) as the frame path rounds it:
    mvp = proj * view, then row 2 of mvp * (x, y, z, 1)."""
    m22, m23 = F32(proj[10]), F32(proj[11])
    mvp23 = F32(F32(m22 * F32(-2.0)) + m23)
    zw = np.asarray(zw, F32)
    return (F32(0.0) + ((m22 * zw).astype(F32) + mvp23).astype(F32)).astype(F32)


def partition(L, placed):
    """Group lengths for a list of L: ``placed`` = {list index: run length},
    every other entry a depth of its own."""
    out, at = [], 0
    for start in sorted(placed):
        assert start >= at, (start, at)
        out += [1] * (start - at) + [placed[start]]
        at = start + placed[start]
    assert at <= L, (at, L)
    return out + [1] * (L - at)


def _walk(k, L, x0, y0, tw, th):
    """The k-th of L points of the serpentine walk over tile (x0, y0)'s
    interior: th - 8 rows (8 for 16x16, 12 for 32x20), alternating direction,
    y advancing along the walk.  Neighbours are at most 0.02 rows apart (a
    short list sits around the walk's middle), so they always share a pixel."""
    rows = th - 8
    step = min(rows / L, 0.02)
    t = rows / 2 + (np.asarray(k, np.float64) - (L - 1) / 2) * step
    row = np.minimum(np.floor(t), rows - 1)
    fr = t - row
    fr = np.where(row.astype(np.int64) % 2 == 1, 1.0 - fr, fr)
    px = x0 + MARGIN + (tw - 2 * MARGIN) * fr
    py = y0 + MARGIN + (th - 2 * MARGIN) * t / rows
    return px, py


def build(spec, tile_w, tile_h, W, H, seed, input_shuffle=True):
    """-> (g[n, 16] float32, view16, proj16, fov).  Row layout: mean 0:4,
    rgb + opacity 4:8, quaternion wxyz 8:12, log-scales 12:15, gid 15."""
    assert W % tile_w == 0 and H % tile_h == 0
    tiles_x, tiles_y = W // tile_w, H // tile_h
    assert tiles_x % 2 == 1 and tiles_y % 2 == 1
    cells = [(tx, ty) for tx, ty, _, _ in spec]
    for i, (tx, ty) in enumerate(cells):
        assert 0 < tx < tiles_x - 1 and 0 < ty < tiles_y - 1
        for ux, uy in cells[:i]:
            assert max(abs(tx - ux), abs(ty - uy)) >= 2, "target tiles touch"
    rng = np.random.default_rng(seed)
    proj = projection(W, H)
    n = sum(L for _, _, L, _ in spec)
    index = rng.permutation(n) if input_shuffle else np.arange(n)
    g = np.zeros((n, 16), np.float32)
    at = 0
    for tx, ty, L, runs in spec:
        idx = index[at:at + L]
        at += L
        if isinstance(runs, str):
            assert runs == "ulp"
            zc = F32(1.0) / np.abs(F32(proj[10]))  # |m22| * zc ~ 1.0
            zw = np.empty(L, F32)
            zw[L // 2] = zc
            for i in range(L // 2 + 1, L):
                zw[i] = np.nextafter(zw[i - 1], F32(2.0))
            for i in range(L // 2 - 1, -1, -1):
                zw[i] = np.nextafter(zw[i + 1], F32(0.0))
        else:
            groups = [1] * L if runs is None else list(runs)
            assert sum(groups) == L and min(groups) >= 1, (L, runs)
            G = len(groups)
            d = D_MIN + (D_MAX - D_MIN) * (np.arange(G) + rng.uniform(0.25, 0.75, G)) / G
            zw = np.repeat((2.0 - d).astype(F32), groups)
        zw = zw[rng.permutation(L)]  # depth order is not input order
        # list order: (clip z, input index)
        order = np.lexsort((idx, clip_z(zw, proj)))
        rank = np.empty(L, np.int64)
        rank[order] = np.arange(L)
        px, py = _walk(rank, L, tx * tile_w, ty * tile_h, tile_w, tile_h)
        dist = 2.0 - zw.astype(np.float64)
        g[idx, 0] = ((px / W) * 2.0 - 1.0) * dist / float(proj[0])
        g[idx, 1] = ((py / H) * 2.0 - 1.0) * dist / float(proj[5])
        g[idx, 2] = zw
    g[:, 3] = 1.0
    g[:, 4:7] = rng.uniform(0.0, 1.0, (n, 3))
    g[:, 7] = rng.uniform(0.01, 0.04, n)
    g[:, 8] = 1.0
    g[:, 12:15] = LOG_SCALE
    g[:, 15] = np.arange(n) + 1
    return g, VIEW.copy(), proj, FOV


# ---------------------------------------------------------------- the scenes of test_gpu_sort_edges.py
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049,
           2559, 2560, 2561, 4095, 4096, 4097, 6145)

# (L, {list index: run length}); runs at the list's start and end, across ~512,
# ~1024, 2047/2048, 2560 and 4096
TIE_LISTS = [
    (200, {0: 2, 20: 15, 50: 16, 80: 17, 110: 64, 198: 2}),
    (1500, {0: 16, 100: 2, 200: 15, 300: 17, 400: 64, 900: 300, 1483: 17}),
    (3000, {0: 15, 1016: 16, 1100: 2, 1200: 64, 2040: 17, 2300: 300, 2985: 15}),
    (5000, {0: 17, 1000: 64, 1900: 300, 2553: 15, 4090: 16, 4500: 2, 4936: 64}),
]
# One run of kTieRun keys or more sends the whole list to be sorted again, so
# in the lists above the runs of 15 to 17 never decide anything.  These have a
# longest run of exactly 15, 16 and 17, one list per class of the sort: 15 is
# put in order in place, 16 and 17 take the second sort.
TIE_LISTS += [(200, {0: m, 90: min(m, 15), 200 - m: m}) for m in (15, 16, 17)]
TIE_LISTS += [(1500, {0: m, 520 - m: m, 1000: min(m, 15), 1500 - m: m}) for m in (15, 16, 17)]
TIE_LISTS += [(3000, {0: m, 1032 - m: m, 2056 - m: m, 3000 - m: m}) for m in (15, 16, 17)]
SINGLE_DEPTH = (64, 1024, 2049, 3000)
TWO_DEPTH = 2600
ULP = 64


def _cells(tiles_x, tiles_y):
    return [(tx, ty) for ty in range(1, tiles_y, 2) for tx in range(1, tiles_x, 2)]


def lengths_spec():
    """(spec, tiles_x, tiles_y): one tile per LENGTHS value, no ties; 38 212
    Gaussians on a 15 x 9 grid (target tiles in tile rows 1, 3, 5, 7)."""
    cells = _cells(15, 9)
    # the longest lists are not next to each other in tile order
    order = np.random.default_rng(1).permutation(len(LENGTHS))
    return [(cells[i][0], cells[i][1], LENGTHS[j], None) for i, j in enumerate(order)], 15, 9


def ties_spec():
    """(spec, tiles_x, tiles_y): the lists with runs of equal depth; 32 601
    Gaussians on a 15 x 9 grid (target tiles in tile rows 1, 3 and 5)."""
    lists = [(L, partition(L, placed)) for L, placed in TIE_LISTS]
    lists += [(L, [L]) for L in SINGLE_DEPTH]
    lists += [(TWO_DEPTH, [TWO_DEPTH // 2, TWO_DEPTH // 2]), (ULP, "ulp")]
    cells = _cells(15, 9)
    order = np.random.default_rng(2).permutation(len(lists))
    return [(cells[i][0], cells[i][1]) + lists[j] for i, j in enumerate(order)], 15, 9


def short_spec():
    """(spec, tiles_x, tiles_y): the lists of both scenes that one workgroup
    sorts (<= 2048 keys), for the hosts a band with a longer list never
    reaches (the direct binning: such a band's later frames are lazy); 18 002
    Gaussians on a 17 x 9 grid."""
    lists = [(L, None) for L in LENGTHS if L <= 2048]
    lists += [(L, partition(L, placed)) for L, placed in TIE_LISTS if L <= 2048]
    lists += [(64, [64]), (1024, [1024]), (ULP, "ulp")]
    cells = _cells(17, 9)
    order = np.random.default_rng(3).permutation(len(lists))
    return [(cells[i][0], cells[i][1]) + lists[j] for i, j in enumerate(order)], 17, 9


SPECS = {"lengths": lengths_spec, "ties": ties_spec, "short": short_spec}


@functools.lru_cache(maxsize=None)
def scene(name, tile_w=16, tile_h=16):
    """dict(spec, g, view, proj, fov, W, H, tile): the named scene at a tile
    size, built once per process."""
    spec, tiles_x, tiles_y = SPECS[name]()
    W, H = tiles_x * tile_w, tiles_y * tile_h
    g, view, proj, fov = build(spec, tile_w, tile_h, W, H, seed={"lengths": 21, "ties": 22, "short": 23}[name])
    return {"spec": spec, "g": g, "view": view, "proj": proj, "fov": fov, "W": W, "H": H, "tile": (tile_w, tile_h)}


def oracle_frame(sc, band=None):
    from oracle import oracle as O

    return O.make_frame(sc["view"], sc["proj"], sc["W"], sc["H"], sc["tile"][0], sc["tile"][1], sc["fov"], 1.0,
                        band=band)


@functools.lru_cache(maxsize=None)
def reference(name, tile_w=16, tile_h=16, band=None):
    """The oracle's outputs for the whole frame (or the tile rows ``band`` =
    (ty0, ty1)), computed once per process and left unchanged:
    dict(scene, frame, proj (records), ts, lst, render)."""
    from oracle import oracle as O

    sc = scene(name, tile_w, tile_h)
    f = oracle_frame(sc, band)
    p = O.project(sc["g"], f)
    ts, lst = O.bin_lists(p, f)
    return {"scene": sc, "frame": f, "proj": p, "ts": ts, "lst": lst, "render": O.render(sc["g"], f)}


@functools.lru_cache(maxsize=None)
def w_scene(sh_degree=0):
    """The synthetic scene of the branch tests (20 000 Gaussians, 640x360)
    with mean w drawn from {0.5, 1, 2}: dict(g, ply, view, proj, fov, W, H)."""
    from gaussian_splat_ipu_amd import camera, scene as gscene

    ply = gscene.synthetic(gscene.SynthSpec(n=20000, seed=7, sh_degree=sh_degree))
    g, bb = gscene.prepare_scene(ply)
    a = np.ascontiguousarray(g).view(np.float32).reshape(-1, 16).copy()
    a[:, 3] = np.random.default_rng(31).choice(np.float32([0.5, 1.0, 2.0]), a.shape[0])
    view, proj = camera.headless(bb, 640, 360)
    return {"g": a, "ply": ply, "view": view, "proj": proj, "fov": camera.FOV_DEFAULT, "W": 640, "H": 360}
