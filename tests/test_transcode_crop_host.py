"""Drop chroma, crop and copy metadata on the host route: hipjpegTranscodeHostRegion.  Every result is held against
tests/helpers/crop_model.py (status, size, luma factors, coefficients over the real area, tables; the marker segments and the EXIF patch),
and pixels witness the convention: a cropped file decodes to the region of the source's pixels, a GRAYSCALE file to the luma plane.

Pixels of a crop.  Without fancy upsampling the cropped file decodes EXACTLY to decode(source)[y0:y1, x0:x1] for every sampling: the
region starts on an iMCU, so every output sample comes from the same chroma sample through the same arithmetic.  With fancy upsampling
that still holds for gray and 4:4:4 sources; in a subsampled one the triangle filter takes the neighbouring chroma sample, which at the
outermost row and column of the cropped picture no longer exists (libjpeg replicates the edge instead), so the border may differ -- by
up to 30 levels here -- and only the interior [1:-1, 1:-1] is asserted."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import oracle
from helpers import crop_model as C
from helpers import transcode_cases as T
from helpers import transform_model as M
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

_DECODE = T.golden_files("decode")


def _status(data, **kw):
    try:
        return T.SUCCESS, lowlevel.transcode_host(data, **kw)
    except N.HipJpegError as e:
        return e.status, None


@functools.lru_cache(maxsize=None)
def _croppable():
    """[(name, data, region)] of the decode goldens the recipe fits"""
    out = []
    for name, data in _DECODE:
        try:
            region = C.recipe_region(data)
        except Exception:
            region = None
        if region is not None:
            out.append((name, data, region))
    return out


def _img(w, h, sub, seed, q=88):
    return oracle.encode(synth_image(w, h, seed=seed), sub, q)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_every_decode_golden_crops_into_the_models_picture(orientation):
    succeeded = 0
    for name, data, region in _croppable():
        want = C.expected(data, orientation, trim=True, region=region)
        st, out = _status(data, optimized_huffman=True, orientation=orientation, trim=orientation != 1, region=region)
        assert st == want["status"], (name, N.STATUS_NAMES.get(st, st))
        if st == T.SUCCESS:
            M.check_file(out, want)
            succeeded += 1
    print(f"orientation {orientation}: {succeeded} of {len(_croppable())} croppable goldens succeed ({len(_DECODE)} goldens)")
    if orientation == 1:
        assert succeeded >= 75


def test_cropped_files_decode_to_the_region_of_the_sources_pixels():
    checked = subsampled = 0
    for name, data, region in _croppable():
        st, out = _status(data, region=region)
        if st != T.SUCCESS:
            continue
        x0, y0, x1, y1 = region
        info = oracle.read_info(data)
        assert np.array_equal(oracle.decode(out, fancy=False), oracle.decode(data, fancy=False)[y0:y1, x0:x1]), name
        got, want = oracle.decode(out), oracle.decode(data)[y0:y1, x0:x1]
        if info["ncomp"] == 1 or (info["hmax"], info["vmax"]) == (1, 1):
            assert np.array_equal(got, want), name
        else:  # the border has lost its neighbour across the cut (see the docstring)
            assert np.array_equal(got[1:-1, 1:-1], want[1:-1, 1:-1]), name
            subsampled += 1
        checked += 1
    print(f"pixel witness: {checked} cropped files, {subsampled} of them subsampled")
    assert checked >= 75 and subsampled >= 20


def test_grayscale():
    checked = 0
    for name, data in _DECODE:
        info = oracle.read_info(data)
        want = C.expected(data, grayscale=True)
        st, out = _status(data, grayscale=True)
        assert st == want["status"], name
        if info["ncomp"] == 1 and st == T.SUCCESS:
            assert out == lowlevel.transcode_host(data), name  # nothing to drop
        if info["ncomp"] != 3 or st != T.SUCCESS:
            continue
        M.check_file(out, want)
        gi = oracle.read_info(out)
        assert gi["ncomp"] == 1 and (gi["width"], gi["height"]) == (info["width"], info["height"])
        pixels = oracle.decode(out, oracle.FMT_GRAY)
        assert np.array_equal(pixels, oracle.decode_planes(data)[0][:info["height"], :info["width"]]), name
        assert np.array_equal(pixels, oracle.decode(data, oracle.FMT_GRAY)), name
        checked += 1
    print(f"grayscale: {checked} three-component goldens")
    assert checked >= 50


def _with_other_cr_table(jpeg):
    """The file with component 3 on a quantization table of its own (table 2: the chroma table with one entry changed)"""
    b = bytearray(jpeg)
    segs = C.header_segments(jpeg)
    dqt = [s for m, s in segs if m == 0xDB]
    tables = b"".join(s[4:] for s in dqt)
    chroma = next(tables[i:i + 65] for i in range(0, len(tables), 65) if tables[i] == 1)
    extra = bytearray(chroma)
    extra[0], extra[5] = 2, extra[5] + 1
    sof = bytes(b).index(b"\xff\xc0")
    assert b[sof + 9] == 3 and b[sof + 18] == 1
    b[sof + 18] = 2
    return bytes(b[:sof]) + b"\xff\xdb" + struct.pack(">H", 67) + bytes(extra) + bytes(b[sof:])


def test_grayscale_waives_the_chroma_rules_only():
    src = _img(48, 40, "420", 51)
    odd = _with_other_cr_table(src)
    assert not T.header_eligible(odd) and C.gray_eligible(odd, oracle.decode_coefficients(odd)[1])
    assert _status(odd)[0] == T.UNSUPPORTED
    st, out = _status(odd, grayscale=True)
    assert st == T.SUCCESS and out == lowlevel.transcode_host(src, grayscale=True)
    # an RGB-labelled stream (Adobe transform 0 and no JFIF) stays refused
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert src[2:20] == C.JFIF_APP0
    rgb = src[:2] + adobe + src[2 + 18:]
    assert lowlevel.get_image_info(rgb)["color_model"] == 2
    assert _status(rgb)[0] == T.UNSUPPORTED and _status(rgb, grayscale=True)[0] == T.UNSUPPORTED
    # from GRAYSCALE on the iMCU is 8x8
    assert _status(src, region=(8, 8, 40, 40))[0] == T.UNSUPPORTED
    st, out = _status(src, region=(8, 8, 40, 40), grayscale=True)
    assert st == T.SUCCESS
    M.check_file(out, C.expected(src, region=(8, 8, 40, 40), grayscale=True))
    assert np.array_equal(oracle.decode(out, oracle.FMT_GRAY), oracle.decode(src, oracle.FMT_GRAY)[8:40, 8:40])


def test_expand():
    src = _img(80, 64, "420", 52)
    assert _status(src, region=(21, 13, 70, 50))[0] == T.UNSUPPORTED
    st, out = _status(src, region=(21, 13, 70, 50), expand=True)
    assert st == T.SUCCESS and out == lowlevel.transcode_host(src, region=(16, 0, 70, 50))
    want = C.expected(src, region=(21, 13, 70, 50), expand=True)
    assert (want["width"], want["height"]) == (54, 50)
    M.check_file(out, want)
    assert lowlevel.transcode_host(src, region=(16, 16, 70, 50), expand=True) == lowlevel.transcode_host(src, region=(16, 16, 70, 50))


def test_invalid_regions_and_the_whole_picture():
    for sub in ("gray", "444", "420"):
        src = _img(50, 37, sub, 53)
        for region in ((-8, 0, 16, 16), (0, -8, 16, 16), (16, 0, 16, 8), (32, 0, 16, 8), (0, 16, 8, 16), (0, 0, 51, 37), (0, 0, 50, 38),
                       (48, 0, 0, 0), (0, 0, 0, 16), (0, 0, 16, 0)):
            assert _status(src, region=region)[0] == C.INVALID_ARGUMENT == C.expected(src, region=region)["status"], (sub, region)
            assert _status(src, region=region, expand=True, grayscale=True, orientation=6, trim=True)[0] == C.INVALID_ARGUMENT
        for kw in T.TARGETS.values():
            plain = lowlevel.transcode_host(src, **kw)
            assert lowlevel.transcode_host(src, region=(0, 0, 50, 37), **kw) == plain
            assert lowlevel.transcode_host(src, region=(0, 0, 0, 0), **kw) == plain and lowlevel.transcode_host(src, region=None, **kw) == plain
    for name, data in _DECODE[::5]:
        info = oracle.read_info(data)
        assert _status(data, optimized_huffman=True, region=(0, 0, info["width"], info["height"])) == _status(data, optimized_huffman=True), name


@pytest.mark.parametrize("orientation", range(2, 9))
def test_a_crop_then_a_turn_is_the_one_call_and_bytes_do_not_depend_on_the_targets_route(orientation):
    composed = 0
    for name, data, region in _croppable()[::3]:
        st, both = _status(data, orientation=orientation, trim=True, region=region)
        if st != T.SUCCESS:
            continue
        cropped = lowlevel.transcode_host(data, region=region)
        assert lowlevel.transcode_host(cropped, orientation=orientation, trim=True) == both, name
        for kw in (T.TARGETS["progressive"], dict(optimized_huffman=True, restart_interval=3)):
            assert lowlevel.transcode_host(data, orientation=orientation, trim=True, region=region, **kw) == lowlevel.transcode_host(both, **kw), name
        composed += 1
    assert composed >= 15


def test_flag_bits():
    data = _DECODE[0][1]
    a = np.frombuffer(data, dtype=np.uint8)
    out, n = np.empty(len(data) * 2 + 65536, dtype=np.uint8), ctypes.c_size_t()

    def call(field, region=None):
        p = N.TranscodeParams(0, 0, 0, field)
        r = ctypes.byref(N.TranscodeRegion(*region)) if region else None
        return N.load().hipjpegTranscodeHostRegion(a.ctypes.data, a.size, ctypes.byref(p), r, out.ctypes.data, out.size, ctypes.byref(n))

    assert (N.TRANSCODE_GRAYSCALE, N.TRANSCODE_CROP_EXPAND, N.TRANSCODE_COPY_MARKERS) == (0x80000, 0x100000, 0x200000)
    for field in (1, N.TRANSCODE_TRIM | 1, 9, 15, 16, 1 << 18, 1 << 30, -1, N.TRANSCODE_ORIENTATION_FROM_EXIF | 6, N.TRANSCODE_TRIM | 9,
                  1 << 22, 1 << 15, N.TRANSCODE_GRAYSCALE | 1, N.TRANSCODE_COPY_MARKERS | 9, N.TRANSCODE_CROP_EXPAND | (1 << 18),
                  N.TRANSCODE_GRAYSCALE | N.TRANSCODE_ORIENTATION_FROM_EXIF | 2):
        assert call(field) == C.INVALID_ARGUMENT, field
        assert call(field, (0, 0, 8, 8)) == C.INVALID_ARGUMENT, field
    every = N.TRANSCODE_GRAYSCALE | N.TRANSCODE_CROP_EXPAND | N.TRANSCODE_COPY_MARKERS | N.TRANSCODE_TRIM
    for field in (N.TRANSCODE_GRAYSCALE, N.TRANSCODE_CROP_EXPAND, N.TRANSCODE_COPY_MARKERS, every | 6, every | N.TRANSCODE_ORIENTATION_FROM_EXIF):
        assert call(field) in (T.SUCCESS, T.UNSUPPORTED), field
    # the old entry point is the NULL-region case
    p = N.TranscodeParams(1, 0, 0, 0)
    assert N.load().hipjpegTranscodeHost(a.ctypes.data, a.size, ctypes.byref(p), out.ctypes.data, out.size, ctypes.byref(n)) == 0
    old = out[:n.value].tobytes()
    assert N.load().hipjpegTranscodeHostRegion(a.ctypes.data, a.size, ctypes.byref(p), None, out.ctypes.data, out.size, ctypes.byref(n)) == 0
    assert out[:n.value].tobytes() == old


# ---------------------------------------------------------------------------------------------- markers
def _segment(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


ICC = [b"ICC_PROFILE\0" + bytes([k + 1, 2]) + bytes((k * 7 + i * 13) & 0xFF for i in range(65533 - 14)) for k in range(2)]
JFXX = _segment(0xE0, b"JFXX\0\x10" + bytes(9))
XMP = _segment(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x/>")
ADOBE = _segment(0xEE, b"Adobe\0\x64\0\0\0\0\x01")
COM = _segment(0xFE, b"a comment \xff\xd8 with marker-like bytes")


def _tagged(base, value, little_endian, progressive=False):
    """`base` (the writer's own output: SOI, JFIF APP0, ...) with a full set of metadata behind its APP0; fill bytes in front of COM"""
    assert base[2:20] == C.JFIF_APP0
    extra = JFXX + M.exif_segment(value, little_endian) + M.exif_segment(3, not little_endian) + XMP + _segment(0xE2, ICC[0]) + \
        _segment(0xE2, ICC[1]) + ADOBE + b"\xff\xff\xff" + COM
    out = base[:20] + extra + base[20:]
    if progressive:  # an APP segment behind the first scan is not header metadata
        second = out.index(b"\xff\xda", out.index(b"\xff\xda") + 2)
        dht = out.rindex(b"\xff\xc4", 0, second)
        out = out[:dht] + _segment(0xE5, b"late") + out[dht:]
    return out


@pytest.mark.parametrize("little_endian", [False, True], ids=["MM", "II"])
def test_markers_are_copied_and_the_exif_orientation_follows_the_turn(little_endian):
    plain = lowlevel.transcode_host(_img(64, 48, "420", 54))
    prog = lowlevel.transcode_host(plain, progressive=True)
    for source, late in ((_tagged(plain, 6, little_endian), False), (_tagged(prog, 6, little_endian, True), True)):
        assert lowlevel.exif_orientation(source) == M.read_exif_orientation(source) == 6
        assert len(C.header_segments(source)) >= 12
        for target, kw in T.TARGETS.items():
            assert lowlevel.transcode_host(source, **kw) == lowlevel.transcode_host(plain, **kw)  # without the flag: today's bytes
            for turn_kw, turned in ((dict(), False), (dict(orientation=6), True), (dict(from_exif=True), True), (dict(orientation=2, region=(16, 16, 48, 48)), True),
                                    (dict(region=(16, 16, 48, 48), grayscale=True), False)):
                out = lowlevel.transcode_host(source, copy_markers=True, **turn_kw, **kw)
                bare = lowlevel.transcode_host(source, **turn_kw, **kw)
                want = C.copied_segments(source, turned)
                assert len(want) == 8 and not any(b"late" in s for s in want)
                assert C.app_and_com_segments(out) == [C.JFIF_APP0] + want, (target, turn_kw)
                # right behind the writer's APP0, in front of the first DQT; the rest of the file is the file without metadata
                blob = b"".join(want)
                assert out[:20] == bare[:20] and out[20:20 + len(blob)] == blob and out[20 + len(blob):] == bare[20:]
                assert out[20 + len(blob):22 + len(blob)] == b"\xff\xdb"
                T.same_picture(bare, out)
                value = 1 if turned else 6
                assert lowlevel.exif_orientation(out) == M.read_exif_orientation(out) == value, (target, turn_kw)
                # the patched segment differs from the source's in the two value bytes only
                src_exif, out_exif = M.exif_segment(6, little_endian), want[1]
                diff = [i for i in range(len(src_exif)) if src_exif[i] != out_exif[i]]
                assert len(out_exif) == len(src_exif) and (diff == ([4 + 6 + 18 + (0 if little_endian else 1)] if turned else []))
                assert want[2] == M.exif_segment(3, not little_endian)  # the second Exif segment is left alone
        assert (b"late" in source) == late


def test_exif_segments_that_cannot_be_patched_are_copied_as_they_are():
    plain = lowlevel.transcode_host(_img(32, 32, "444", 55))
    whole = M.exif_segment(5, True)
    cases = [M.exif_segment(6, False, tag=0x0111),                         # no orientation tag
             _segment(0xE1, whole[4:4 + 6 + 8 + 2 + 6]),                   # the IFD's only entry is cut short
             _segment(0xE1, whole[4:4 + 6 + 8]),                           # no IFD at all
             _segment(0xE1, b"Exif\0\0II\x2a\0\xff\xff\xff\x7f" + bytes(8)),  # the IFD offset points far outside
             _segment(0xE1, b"Exif\0\0XX\0\x2a" + bytes(20)),              # no byte order
             _segment(0xE1, b"Exif\0\0")]
    for seg in cases:
        source = plain[:20] + seg + M.exif_segment(8, True) + plain[20:]
        assert lowlevel.exif_orientation(source) == M.read_exif_orientation(source) == 1
        out = lowlevel.transcode_host(source, copy_markers=True, orientation=6)
        assert C.app_and_com_segments(out) == [C.JFIF_APP0, seg, M.exif_segment(8, True)] == [C.JFIF_APP0] + C.copied_segments(source, True)
        assert lowlevel.exif_orientation(out) == 1
    # a file without metadata: the flag changes nothing
    assert lowlevel.transcode_host(plain, copy_markers=True, orientation=6) == lowlevel.transcode_host(plain, orientation=6)


def test_pillow_reads_the_icc_profile_back():
    import io
    try:
        from PIL import Image
    except ImportError:  # no Pillow here: the segment lists above are the check
        return
    plain = lowlevel.transcode_host(_img(64, 48, "420", 54))
    source = _tagged(plain, 6, True)
    profile = Image.open(io.BytesIO(source)).info["icc_profile"]
    assert profile == ICC[0][14:] + ICC[1][14:]
    for kw in (dict(), dict(orientation=6, progressive=True), dict(region=(16, 16, 64, 48), grayscale=True, optimized_huffman=True)):
        im = Image.open(io.BytesIO(lowlevel.transcode_host(source, copy_markers=True, **kw)))
        im.load()
        assert im.info["icc_profile"] == profile
