"""Writes the PLY-reader fixtures of tests/test_ref_ply.py and tests/test_host.py:

    python tools/make_ref_ply_golden.py --ref-data <reference checkout>/data

For each data file the reference ships (point_cloud_9 .. 12) it stores under
tests/golden/:

- point_cloud_<k>_head.ply: the file's own header with the vertex count set
  to HEAD, and the first HEAD vertices' bytes unchanged (the whole files are
  1.7 - 3.0 MB each; point_cloud_12.ply is stored in full already);
- ref_ply_parser.json: what the reference's own parser (oracle/_ref/ply_dump,
  `make -C oracle ref-tools`) reads from each stored file: the vertex count and
  the SHA-256 of each of the 14 properties' float32 arrays.

Needs the reference checkout (the parser is compiled from its happly.h); the
tests need only the stored files.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOOL = os.path.join(ROOT, "oracle", "_ref", "ply_dump")
PROPS = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
         "rot_0", "rot_1", "rot_2", "rot_3"]
# 4096 vertices x 68 B = 272 KiB: several of any reader's buffers, every
# property column, well under the size limit of a committed file
HEAD = 4096


def head_of(src: str, dst: str, n_keep: int) -> int:
    """Copy src's header (vertex count replaced) and its first n_keep vertices."""
    raw = open(src, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines(keepends=True)
    assert lines[1].strip() == "format binary_little_endian 1.0", lines[1]
    n_props = sum(1 for ln in lines if ln.startswith("property float "))
    assert n_props == sum(1 for ln in lines if ln.startswith("property ")), "float properties only"
    n_full = None
    for i, ln in enumerate(lines):
        if ln.startswith("element vertex "):
            n_full = int(ln.split()[2])
            lines[i] = f"element vertex {n_keep}\n"
    assert n_full is not None and n_full >= n_keep
    assert len(raw) - end == n_full * n_props * 4, "vertex element only"
    with open(dst, "wb") as fh:
        fh.write("".join(lines).encode("ascii"))
        fh.write(raw[end:end + n_keep * n_props * 4])
    return n_full


def parser_record(path: str) -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "ref.bin")
        subprocess.run([TOOL, path, dump], check=True)
        raw = open(dump, "rb").read()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    cols = np.frombuffer(raw[8:], np.float32).reshape(len(PROPS), n)
    return {"vertices": n, "sha256": {p: hashlib.sha256(cols[k].tobytes()).hexdigest() for k, p in enumerate(PROPS)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-data", required=True, help="the reference checkout's data/ directory")
    a = ap.parse_args()
    if not os.path.exists(TOOL):
        sys.exit("oracle/_ref/ply_dump is not built: make -C oracle ref-tools")
    rec = {}
    for k in (9, 10, 11):
        name = f"point_cloud_{k}_head.ply"
        full = head_of(os.path.join(a.ref_data, f"point_cloud_{k}.ply"), os.path.join(GOLDEN, name), HEAD)
        rec[name] = {"source": f"point_cloud_{k}.ply", "source_vertices": full,
                     **parser_record(os.path.join(GOLDEN, name))}
    src12 = os.path.join(a.ref_data, "point_cloud_12.ply")
    assert open(src12, "rb").read() == open(os.path.join(GOLDEN, "point_cloud_12.ply"), "rb").read()
    r12 = parser_record(os.path.join(GOLDEN, "point_cloud_12.ply"))
    rec["point_cloud_12.ply"] = {"source": "point_cloud_12.ply", "source_vertices": r12["vertices"], **r12}
    with open(os.path.join(GOLDEN, "ref_ply_parser.json"), "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
