"""The product's PLY reader (gs_ply_load, csrc/host/gs_scene.cpp) against the
reference's own parser: its vendored happly.h, called as
splat::fillPlyProperties calls it (src/splat/file_io.cpp:57-77) by
oracle/ref_ply_dump.cpp.  Every one of the 14 properties of every data file
the reference ships must come out bit for bit the same.

Self-contained: the inputs are stored under tests/golden/ (point_cloud_12.ply
in full; of point_cloud_9 / 10 / 11, 1.7 - 3.0 MB each, the header and the
first 4096 vertices: the reader treats every vertex alike, and 272 KiB of
them span several of its read buffers), and what the reference's parser reads
from those stored files is recorded in tests/golden/ref_ply_parser.json
(vertex count, SHA-256 of each property's float32 array; written by
tools/make_ref_ply_golden.py).  Where build() has compiled the reference's
parser (oracle/_ref/ply_dump, only next to a reference checkout) the test also
runs it on the same stored file, value for value.  CPU only."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

TOOL = os.path.join(ROOT, "oracle", "_ref", "ply_dump")
PROPS = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
         "rot_0", "rot_1", "rot_2", "rot_3"]
# (test id, stored file, read from a copy elsewhere): a fixed list, the same
# ids on every machine.  This module used to collect its cases from what it
# found at collection time: beside a reference checkout its four data files and
# the stored point_cloud_12.ply, two equal names that pytest numbered
# point_cloud_12.ply0 (the reference's copy) and point_cloud_12.ply1 (the
# stored one), and elsewhere point_cloud_12.ply alone.  All of those ids stay;
# ...ply0 still reads a second copy of the same bytes at another path.
CASES = [("point_cloud_9.ply", "point_cloud_9_head.ply", False),
         ("point_cloud_10.ply", "point_cloud_10_head.ply", False),
         ("point_cloud_11.ply", "point_cloud_11_head.ply", False),
         ("point_cloud_12.ply", "point_cloud_12.ply", False),
         ("point_cloud_12.ply0", "point_cloud_12.ply", True),
         ("point_cloud_12.ply1", "point_cloud_12.ply", False)]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ref_ply_parser.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("stored,copied", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_ply_reader_matches_the_reference_parser(built, recorded, tmp_path, stored, copied):
    import shutil

    from gaussian_splat_ipu_amd import scene

    path = os.path.join(GOLDEN, stored)
    if copied:
        path = str(shutil.copy(path, tmp_path / "a second copy.ply"))
    rec = recorded[stored]
    ply = scene.load_ply(path)
    assert len(ply) == rec["vertices"]
    for name in PROPS:
        got = np.ascontiguousarray(ply[name], np.float32)
        assert hashlib.sha256(got.tobytes()).hexdigest() == rec["sha256"][name], name
    if not os.path.exists(TOOL):
        return  # (no reference checkout at build time: the recorded answer stands alone)
    dump = tmp_path / "ref.bin"
    subprocess.run([TOOL, path, str(dump)], check=True)
    raw = dump.read_bytes()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    ref = np.frombuffer(raw[8:], np.float32).reshape(len(PROPS), n)
    assert len(ply) == n
    for k, name in enumerate(PROPS):
        got = np.asarray(ply[name], np.float32)
        np.testing.assert_array_equal(got.view(np.uint32), ref[k].view(np.uint32), err_msg=name)
