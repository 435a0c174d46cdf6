"""Lossless turns on the host route: hipjpegTranscodeHost with an orientation.  The file that comes out must hold the picture that
tests/helpers/transform_model.py derives from the DCT identities (status, size, luma factors, coefficients, tables), and -- as a witness
that "orientation k" means "brought upright for EXIF value k" -- decode to the turned pixels of the source.

Pixels.  A vertical mirror (orientation 4) of a gray or 4:4:4 source decodes to EXACTLY the mirrored pixels: jidctint's column pass
comes first, and its even / odd butterflies turn the sign change of the odd vertical frequencies into the mirrored column, rounding
included.  The same was expected of orientations 2 and 3 and does not hold: there the column pass sees whole columns negated, its
rounding (add half, shift right) is not odd, and the row pass inherits differences of up to 2 levels -- so those cases are in the
bounded check.  For them, for transposing turns (the two passes change roles) and for subsampled sources (the fancy upsampler's
alternating rounding bias does not mirror) a few levels are legitimate: measured over the decode goldens that turn without trimming
(a cut edge gives the upsampler another neighbour) the largest difference is PIXEL_BOUND = 4 levels.  The two 3x5 goldens are left out
of the pixel checks: in a picture of less than one block libjpeg's vertical upsampling takes context rows that its horizontal edge rule
does not have, transposed files of them differ by up to 30 levels from the transposed pixels, and Pillow decodes those files exactly
as the oracle does; their coefficients are checked against the model like everyone's.  The control: on a picture without symmetry a
neighbouring orientation is off by more than ten times the bound."""
import functools

import numpy as np
import pytest

import oracle
from helpers import transcode_cases as T
from helpers import transform_model as M
from helpers.geometry import upright
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

_DECODE = T.golden_files("decode")
ORIENTATIONS = range(2, 9)
PIXEL_BOUND = 4  # levels; measured, see the docstring


def _status(data, **kw):
    try:
        return T.SUCCESS, lowlevel.transcode_host(data, **kw)
    except N.HipJpegError as e:
        return e.status, None


@functools.lru_cache(maxsize=None)
def _pixels(i):
    return oracle.decode(_DECODE[i][1])


@pytest.mark.parametrize("trim", [False, True], ids=["perfect", "trim"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_every_decode_golden_turns_into_the_models_picture(orientation, trim):
    succeeded = 0
    for name, data in _DECODE:
        want = M.expected(data, orientation, trim)
        st, out = _status(data, optimized_huffman=True, orientation=orientation, trim=trim)
        assert st == want["status"], (name, N.STATUS_NAMES.get(st, st))
        if st == T.SUCCESS:
            M.check_file(out, want)
            succeeded += 1
    print(f"orientation {orientation} {'trim' if trim else 'perfect'}: {succeeded} of {len(_DECODE)} succeed")
    assert len(_DECODE) == 127 and succeeded >= (100 if trim else 38)


@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_bytes_do_not_depend_on_the_targets_route(orientation):
    for name, data in _DECODE[::4]:
        st, turned = _status(data, orientation=orientation, trim=True)
        if st != T.SUCCESS:
            continue
        assert lowlevel.transcode_host(data, progressive=True, orientation=orientation, trim=True) == lowlevel.transcode_host(turned, progressive=True), name
        assert lowlevel.transcode_host(data, optimized_huffman=True, restart_interval=3, orientation=orientation, trim=True) == \
            lowlevel.transcode_host(turned, optimized_huffman=True, restart_interval=3), name


def test_orientation_1_is_todays_file_and_turns_compose():
    aligned = 0
    for name, data in _DECODE:
        plain = lowlevel.transcode_host(data)
        assert lowlevel.transcode_host(data, orientation=1) == plain and lowlevel.transcode_host(data, orientation=0, trim=True) == plain, name
        info = oracle.read_info(data)
        hs, vs = M.luma_factors(info)
        if hs == 4 or info["width"] % (8 * hs) or info["height"] % (8 * vs):
            continue
        aligned += 1
        there = lowlevel.transcode_host(data, orientation=6)
        assert lowlevel.transcode_host(there, orientation=8) == plain, name
        assert lowlevel.transcode_host(lowlevel.transcode_host(data, orientation=2), orientation=2) == plain, name
        T.same_picture(data, lowlevel.transcode_host(there, orientation=8))
    assert aligned >= 30


def _exact_case(i, orientation):
    info = oracle.read_info(_DECODE[i][1])
    return orientation == 4 and (info["ncomp"] == 1 or (info["hmax"], info["vmax"]) == (1, 1))


def _less_than_a_block(i):
    info = oracle.read_info(_DECODE[i][1])
    return min(info["width"], info["height"]) < 8


def test_vertical_mirrors_of_gray_and_444_decode_to_the_mirrored_pixels_exactly():
    checked, orientation = 0, 4
    for i, (name, data) in enumerate(_DECODE):
        if not _exact_case(i, orientation) or _less_than_a_block(i):
            continue
        st, out = _status(data, orientation=orientation, trim=True)
        if st != T.SUCCESS:
            continue
        got = oracle.decode(out)
        kept = _pixels(i)[:got.shape[0], :got.shape[1]]
        assert np.array_equal(got, upright(kept, orientation)), name
        checked += 1
    assert checked >= 10


def _pixel_difference(i, orientation):
    """max |decode(turned file) - turned decode(source)| of a golden that turns without trimming, or None"""
    st, out = _status(_DECODE[i][1], orientation=orientation)
    if st != T.SUCCESS:
        return None
    return int(np.abs(oracle.decode(out).astype(np.int32) - upright(_pixels(i), orientation).astype(np.int32)).max())


def test_other_turns_decode_to_the_turned_pixels_within_the_measured_bound():
    worst, cases = 0, 0
    for orientation in ORIENTATIONS:
        for i in range(len(_DECODE)):
            if _exact_case(i, orientation) or _less_than_a_block(i):
                continue
            d = _pixel_difference(i, orientation)
            if d is not None:
                worst, cases = max(worst, d), cases + 1
    print(f"bounded pixel check: {cases} cases, largest difference {worst} levels")
    assert cases >= 300 and worst <= PIXEL_BOUND


def test_the_neighbouring_orientation_is_far_off():
    rgb = synth_image(64, 64, seed=41)
    rgb[:24, :40] //= 3  # no symmetry: a dark corner
    for sub in ("444", "420", "422"):
        src = oracle.encode(rgb, sub, 90)
        pixels = oracle.decode(src)
        for orientation in range(1, 9):
            got = oracle.decode(lowlevel.transcode_host(src, orientation=orientation)).astype(np.int32)
            assert np.abs(got - upright(pixels, orientation)).max() <= PIXEL_BOUND
            for wrong in (orientation % 8 + 1, (orientation - 2) % 8 + 1):
                assert np.abs(got - upright(pixels, wrong)).max() >= 10 * PIXEL_BOUND, (sub, orientation, wrong)


def test_from_exif():
    picked = [d for _, d in _DECODE if oracle.read_info(d)["hmax"] <= 2][:3]
    for k, data in enumerate(picked):
        for value in range(0, 10):
            for little_endian in (False, True):
                tagged = M.with_segment(data, M.exif_segment(value, little_endian))
                want = value if 1 <= value <= 8 else 1
                assert M.read_exif_orientation(tagged) == want and lowlevel.exif_orientation(tagged) == want
                a = _status(tagged, optimized_huffman=True, from_exif=True, trim=True)
                assert a == _status(data, optimized_huffman=True, orientation=want, trim=True), (k, value, little_endian)
                assert a[0] == T.SUCCESS
    data = picked[0]
    assert lowlevel.exif_orientation(data) == M.read_exif_orientation(data) == 1
    assert lowlevel.transcode_host(data, from_exif=True) == lowlevel.transcode_host(data)
    # another tag, an APP1 that is not EXIF, and the first Exif segment wins
    other = M.with_segment(data, M.exif_segment(6, True, tag=0x0111))
    xmp = M.with_segment(M.with_segment(data, M.exif_segment(5, False)), b"\xff\xe1\x00\x08http:/")
    two = M.with_segment(M.with_segment(data, M.exif_segment(3, True)), M.exif_segment(8, False))
    for f, want in ((other, 1), (xmp, 5), (two, 8)):
        assert lowlevel.exif_orientation(f) == M.read_exif_orientation(f) == want
    for _, d in _DECODE:
        assert lowlevel.exif_orientation(d) == M.read_exif_orientation(d)


def test_refusals():
    import ctypes
    data = _DECODE[0][1]
    a = np.frombuffer(data, dtype=np.uint8)
    out, n = np.empty(len(data) * 2 + 65536, dtype=np.uint8), ctypes.c_size_t()
    for field in (1, N.TRANSCODE_TRIM | 1, 9, 15, 16, 1 << 18, 1 << 30, -1, N.TRANSCODE_ORIENTATION_FROM_EXIF | 6, N.TRANSCODE_TRIM | 9):
        p = N.TranscodeParams(0, 0, 0, field)
        assert N.load().hipjpegTranscodeHost(a.ctypes.data, a.size, ctypes.byref(p), out.ctypes.data, out.size, ctypes.byref(n)) == 1, field
    for field in (0, 2, 8, N.TRANSCODE_TRIM | 8, N.TRANSCODE_ORIENTATION_FROM_EXIF | N.TRANSCODE_TRIM):
        p = N.TranscodeParams(0, 0, 0, field)
        assert N.load().hipjpegTranscodeHost(a.ctypes.data, a.size, ctypes.byref(p), out.ctypes.data, out.size, ctypes.byref(n)) in (T.SUCCESS, T.UNSUPPORTED), field
    wide = oracle.encode(synth_image(64, 32, seed=5), "411", 85)
    assert _status(wide, orientation=5)[0] == T.UNSUPPORTED and _status(wide, orientation=6, trim=True)[0] == T.UNSUPPORTED
    assert _status(wide, orientation=2)[0] == T.SUCCESS
    ragged = oracle.encode(synth_image(33, 47, seed=4), "420", 88)
    assert _status(ragged, orientation=3)[0] == T.UNSUPPORTED
    st, cut = _status(ragged, orientation=3, trim=True)
    info = oracle.read_info(cut)
    assert st == T.SUCCESS and (info["width"], info["height"]) == (32, 32)
    assert oracle.read_info(lowlevel.transcode_host(ragged, orientation=5))["width"] == 47  # no mirror, no size rule
    narrow = oracle.encode(synth_image(9, 40, seed=6), "420", 88)  # a mirrored axis shorter than one iMCU
    assert _status(narrow, orientation=2, trim=True)[0] == T.UNSUPPORTED and _status(narrow, orientation=4, trim=True)[0] == T.SUCCESS
