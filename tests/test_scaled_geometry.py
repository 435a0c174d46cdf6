"""Scaled decode, host side (no GPU): hipjpegGetScaledImageSize against the sizes libjpeg-turbo reported for every file and denominator of
tests/golden/manifest_scaled.json, the refusal of denominators other than 1, 2, 4, 8, and the shapes the Python API allocates."""
import ctypes as C

import pytest

from helpers import scaled_goldens as S
from nvimagecodec_amd import _native
from nvimagecodec_amd import lowlevel as L


def _size(w, h, denom):
    sw, sh = C.c_int32(-1), C.c_int32(-1)
    st = _native.load().hipjpegGetScaledImageSize(w, h, denom, C.byref(sw), C.byref(sh))
    return st, sw.value, sh.value


def test_scaled_size_equals_the_library_for_every_manifest_entry():
    checked = 0
    for e in S.FILES:
        try:
            info = L.get_image_info(S.jpeg(e))
        except _native.HipJpegError:
            assert all(s.get("refused") for s in e["scales"].values()), e["name"]  # (more than 10 blocks per MCU: the parser declines too)
            continue
        assert _size(info["width"], info["height"], 1) == (0, info["width"], info["height"])
        for denom in S.DENOMS:
            s = e["scales"][str(denom)]
            if s.get("refused"):
                continue
            assert _size(info["width"], info["height"], denom) == (0, s["width"], s["height"]), (e["name"], denom)
            assert L.scaled_image_size(info["width"], info["height"], denom) == (s["width"], s["height"])
            checked += 1
    assert checked > 900  # 310 files x 3 denominators, less the library's refusals


def test_sizes_of_the_issue():
    for (w, h), want in {(130, 70): [(65, 35), (33, 18), (17, 9)], (7, 5): [(4, 3), (2, 2), (1, 1)], (1, 1): [(1, 1)] * 3,
                         (65535, 65535): [(32768, 32768), (16384, 16384), (8192, 8192)]}.items():
        assert [L.scaled_image_size(w, h, d) for d in S.DENOMS] == want


@pytest.mark.parametrize("denom", [0, -1, 3, 5, 6, 7, 16, 1 << 30])
def test_bad_denominators_are_refused(denom):
    assert _size(130, 70, denom) == (S.INVALID_ARGUMENT, -1, -1)
    with pytest.raises(_native.HipJpegError):
        L.scaled_image_size(130, 70, denom)


def test_bad_arguments_are_refused():
    lib = _native.load()
    w = C.c_int32()
    assert lib.hipjpegGetScaledImageSize(130, 70, 2, None, C.byref(w)) == S.INVALID_ARGUMENT
    assert lib.hipjpegGetScaledImageSize(130, 70, 2, C.byref(w), None) == S.INVALID_ARGUMENT
    assert _size(0, 70, 2)[0] == S.INVALID_ARGUMENT and _size(130, -1, 2)[0] == S.INVALID_ARGUMENT


def test_allocated_shapes():
    e = S.by_name("h130x70_420_opt_q75")
    g = S.by_name("t33x17_gray_base")
    jpegs = [S.jpeg(e), S.jpeg(e), S.jpeg(g), S.jpeg(e), b"no jpeg", S.jpeg(e)]
    scales = [1, 2, 4, 8, 2, 3]
    assert L.output_shapes(jpegs, "rgb", None, scales) == [(70, 130, 3), (35, 65, 3), (5, 9, 3), (9, 17, 3), None, None]
    assert L.output_shapes(jpegs[:4], "rgb_planar", None, scales[:4]) == [(3, 70, 130), (3, 35, 65), (3, 5, 9), (3, 9, 17)]
    assert L.output_shapes(jpegs[:4], "y", None, scales[:4]) == [(70, 130), (35, 65), (5, 9), (9, 17)]
    # a region is in scaled-picture coordinates; orientations from 5 on swap the sides of what is left
    transforms = [None, ((3, 2, 60, 30), 1), (None, 6), ((0, 0, 17, 9), 8)]
    assert L.output_shapes(jpegs[:4], "rgb", transforms, scales[:4]) == [(70, 130, 3), (28, 57, 3), (9, 5, 3), (17, 9, 3)]
    assert L.output_shapes(jpegs[:2], "rgb") == [(70, 130, 3)] * 2  # no scales: as before
