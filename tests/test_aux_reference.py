"""The auxiliary planes' references agree with each other, and the C ABI's aux
entry points exist (no device needed).

tests/auxref.py restates renderTile's walk in numpy for the six planes; its
depth_sum and coverage must equal, bit for bit, what the unchanged oracle
composites when the scene's colours are replaced by (clip z, 1, 0).
"""
import ctypes as C

import numpy as np
import pytest

import auxref


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_equals_the_oracle_with_substituted_colours(built, name):
    r = auxref.reference(name)
    dsum, cov = r["sub"]
    fr = auxref.fractions(r["planes"])
    print(name, fr)
    assert fr["covered"] > 0.05 and fr["two"] > 0.05, fr  # (not an empty frame)
    assert _same_bits(r["planes"]["depth_sum"], dsum)
    assert _same_bits(r["planes"]["coverage"], cov)
    # the other planes' own consistency
    p = r["planes"]
    none = p["count"] == 0
    assert (p["pick"][none] == auxref.PICK_NONE).all() and (p["pick"][~none] < r["g"].shape[0]).all()
    assert (p["weight_max"][none] == 0).all() and (p["weight_max"][~none] > 0).all()
    assert (p["depth_sum"][~none] < 0).all() and (p["depth_median"] <= 0).all()


def test_aux_entry_points_refuse_a_null_handle(built):
    """The four calls are exported, and each returns GS_EINVAL with a message
    for a null handle before it touches a device."""
    from gaussian_splat_ipu_amd import _lib

    L = _lib.lib()
    buf = (C.c_float * 4)()
    ids = (C.c_uint32 * 2)()
    pf, pu, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    px = _lib.AuxPixel()
    assert C.sizeof(px) == 24
    calls = {
        "gs_read_aux32f": lambda: L.gs_read_aux32f(None, buf, 4),
        "gs_read_aux_ids": lambda: L.gs_read_aux_ids(None, ids, 2),
        "gs_aux_device": lambda: L.gs_aux_device(None, C.byref(pf), C.byref(pu), C.byref(n)),
        "gs_read_aux_pixel": lambda: L.gs_read_aux_pixel(None, 0, 0, C.byref(px)),
    }
    for name, call in calls.items():
        assert hasattr(L, name)
        assert call() == _lib.GS_EINVAL, name
        assert name in _lib.last_error(), (name, _lib.last_error())
