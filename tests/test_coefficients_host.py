"""Coefficient tensors on the host (no GPU): hipjpegGetCoefficientInfo, hipjpegDecodeCoefficientsHost, hipjpegEncodeCoefficientsHost.
Reading is pinned against the oracle's coefficients and tables, writing against hipjpegTranscodeHost's files (which
tests/test_transcode_host.py pins against libjpeg-turbo's) and, for edited pictures, against the oracle's reading of the file."""
import ctypes
import functools
import glob
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import sampling_goldens as SG
from helpers import transcode_cases as T
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")
INVALID_ARGUMENT = 1
SENTINEL = -21846  # 0xAAAA


@functools.lru_cache(maxsize=None)
def _goldens():
    files = [(d + "/" + n, b) for d in ("decode", "cmyk", "gamut") for n, b in T.golden_files(d)]
    files += [("sampling/" + e["name"], SG.jpeg(e)) for e in SG.ENTRIES]
    return tuple(files)


@functools.lru_cache(maxsize=None)
def _read(name):
    return lowlevel.decode_coefficients_host(dict(_goldens())[name])


def _golden(name):
    return dict(_goldens())["decode/" + name]


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
    except N.HipJpegError as e:
        return e.status
    return 0


def _zigzag():
    order = sorted(range(64), key=lambda p: (p // 8 + p % 8, p // 8 if (p // 8 + p % 8) % 2 else p % 8))
    assert order[:6] == [0, 1, 8, 16, 9, 2] and order[-3:] == [55, 62, 63]
    return np.array(order)


# ---------------------------------------------------------------- 1. read
def test_read_matches_the_oracle():
    assert len(_goldens()) > 250
    for name, data in _goldens():
        info, coefs = _read(name)
        want, tables = oracle.decode_coefficients(data)
        hdr = lowlevel.get_image_info(data)
        assert (info["width"], info["height"], info["num_components"], info["color_model"]) == \
            (hdr["width"], hdr["height"], hdr["num_components"], hdr["color_model"]), name
        assert info["h"] == hdr["h"] and info["v"] == hdr["v"], name
        area = T.real_area(data)
        assert list(zip(info["blocks_h"], info["blocks_w"])) == area, name
        assert lowlevel.coefficient_info(data)["blocks_w"] == info["blocks_w"]
        for c, (rh, rw) in enumerate(area):
            assert coefs[c].shape == (rh, rw, 8, 8) and coefs[c].dtype == np.int16
            assert np.array_equal(coefs[c].reshape(rh, rw, 64), want[c][:rh, :rw]), (name, c)
            assert np.array_equal(info["qtables"][c], tables[c]), (name, c)


def test_damaged_and_foreign_files_keep_the_decoders_statuses():
    with open(os.path.join(GOLDEN, "damaged", "padding_block_damage.jpg"), "rb") as f:
        damaged = f.read()
    whole = _golden("s64x48_420_base_q90")
    for data in (damaged, whole[: len(whole) * 2 // 3], whole[:100], b"not a jpeg at all"):
        info = None
        try:
            info = lowlevel.coefficient_info(data)
        except N.HipJpegError as e:
            assert e.status == _status(lowlevel.entropy_decode_host, data)
            continue
        out = [np.full((bh, bw, 8, 8), SENTINEL, dtype=np.int16) for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
        st = _status(lowlevel.decode_coefficients_host, data, out)
        assert st != 0 and st == _status(lowlevel.entropy_decode_host, data)
        assert all((o == SENTINEL).all() for o in out)  # a failing image writes nothing


# ---------------------------------------------------------------- 2. pitch
@pytest.mark.parametrize("name", ["s50x37_420_base_q90", "s17x13_gray_prog_q50", "s33x65_422_base_q50"])
def test_pitch(name):
    data = _golden(name)
    info, tight = _read("decode/" + name)
    padded = [np.full((bh, bw + 3, 8, 8), SENTINEL, dtype=np.int16) for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
    lowlevel.decode_coefficients_host(data, padded)
    for p, t, bw in zip(padded, tight, info["blocks_w"]):
        assert np.array_equal(p[:, :bw], t) and (p[:, bw:] == SENTINEL).all()
    for kw in T.TARGETS.values():
        assert lowlevel.encode_coefficients_host(info, padded, **kw) == lowlevel.encode_coefficients_host(info, tight, **kw)


# ---------------------------------------------------------------- 3. write
def test_write_matches_the_transcode():
    written = refused_header = refused_range = 0
    for name, data in _goldens():
        info, coefs = _read(name)
        header, both = T.expected_eligible(data)
        if name.startswith("cmyk/") or (name.startswith("sampling/") and info["num_components"] == 3 and
                                        any((info["h"][c], info["v"][c]) != (1, 1) for c in (1, 2))):
            assert not header, name  # four components, chroma not 1x1: the header rule
        for kw in T.TARGETS.values():
            if both:
                assert lowlevel.encode_coefficients_host(info, coefs, **kw) == lowlevel.transcode_host(data, **kw), (name, kw)
            else:
                assert _status(lowlevel.encode_coefficients_host, info, coefs, **kw) == T.UNSUPPORTED, (name, kw)
                assert _status(lowlevel.transcode_host, data, **kw) == T.UNSUPPORTED, (name, kw)
        written += both
        refused_header += not header
        refused_range += header and not both and name.startswith("gamut/")  # the out-of-range files: the range rule alone
    assert written > 150 and refused_header > 60 and refused_range > 0


# ---------------------------------------------------------------- 4. an edit survives
@pytest.mark.parametrize("name", ["s64x48_420_base_q90", "s50x37_gray_prog_q50"])
def test_an_edit_survives(name):
    from PIL import Image
    info, coefs = _read("decode/" + name)
    zz = _zigzag()
    edited = []
    for c in coefs:
        e = c.reshape(c.shape[0], c.shape[1], 64).copy()
        e[:, :, zz[10:]] = 0
        e[:, :, 0] += 1
        edited.append(np.ascontiguousarray(e.reshape(c.shape)))
    ql, qc = oracle.quality_tables(50)
    new_info = dict(info, qtables=[ql] + [qc] * (info["num_components"] - 1))
    for kw in T.TARGETS.values():
        out = lowlevel.encode_coefficients_host(new_info, edited, **kw)
        got, tables = oracle.decode_coefficients(out)
        for c, e in enumerate(edited):
            rh, rw = e.shape[:2]
            assert np.array_equal(got[c][:rh, :rw], e.reshape(rh, rw, 64)), (kw, c)
            assert np.array_equal(tables[c], new_info["qtables"][c]), (kw, c)
        assert Image.open(io.BytesIO(out)).size == (info["width"], info["height"])


# ---------------------------------------------------------------- 5. argument rules
def _call(info, coefs, orientation=0, restart_interval=0, capacity=None, pointers=None, pitches=None):
    """hipjpegEncodeCoefficientsHost itself -> (status, needed or written size)"""
    ci = lowlevel._info_struct(info)
    P = N.CoefficientPlanes()
    for c, a in enumerate(coefs):
        P.coef[c] = a.ctypes.data if pointers is None else pointers[c]
        P.pitch_blocks[c] = a.shape[1] if pitches is None else pitches[c]
    p = N.TranscodeParams(0, 0, restart_interval, orientation)
    n = ctypes.c_size_t(0)
    cap = 1 << 20 if capacity is None else capacity
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    st = N.load().hipjpegEncodeCoefficientsHost(ctypes.byref(ci), ctypes.byref(P), ctypes.byref(p), out.ctypes.data if cap else None, cap, ctypes.byref(n))
    return st, n.value


def test_argument_rules():
    info, coefs = _read("decode/s64x48_420_base_q90")
    coefs = [c.copy() for c in coefs]
    assert _call(info, coefs)[0] == 0
    # INVALID_ARGUMENT
    for o in (1, 2, 6, N.TRANSCODE_TRIM, N.TRANSCODE_GRAYSCALE, N.TRANSCODE_COPY_MARKERS, N.TRANSCODE_ORIENTATION_FROM_EXIF):
        assert _call(info, coefs, orientation=o)[0] == INVALID_ARGUMENT, o
    assert _call(info, coefs, restart_interval=65536)[0] == INVALID_ARGUMENT
    assert _call(info, coefs, pitches=[info["blocks_w"][0] - 1, info["blocks_w"][1], info["blocks_w"][2]])[0] == INVALID_ARGUMENT
    assert _call(dict(info, blocks_w=[info["blocks_w"][0] + 1] + info["blocks_w"][1:]), coefs, pitches=[64, 64, 64])[0] == INVALID_ARGUMENT
    assert _call(dict(info, blocks_h=info["blocks_h"][:2] + [info["blocks_h"][2] - 1]), coefs)[0] == INVALID_ARGUMENT
    ptrs = [c.ctypes.data for c in coefs]
    assert _call(info, coefs, pointers=[ptrs[0], ptrs[1] + 2, ptrs[2]])[0] == INVALID_ARGUMENT
    assert _call(info, coefs, pointers=[ptrs[0], ptrs[1] + 8, ptrs[2]])[0] == INVALID_ARGUMENT
    assert _call(info, coefs, pointers=[ptrs[0], ptrs[1], None])[0] == INVALID_ARGUMENT
    for w, h in ((0, 48), (64, 0), (65536, 48), (64, 65536)):
        assert _call(dict(info, width=w, height=h), coefs)[0] == INVALID_ARGUMENT
    # UNSUPPORTED: the header rules
    for q in (0, 256):
        bad = [t.copy() for t in info["qtables"]]
        bad[0][17] = q
        assert _call(dict(info, qtables=bad), coefs)[0] == T.UNSUPPORTED, q
    bad = [t.copy() for t in info["qtables"]]
    bad[2][5] += 1
    assert _call(dict(info, qtables=bad), coefs)[0] == T.UNSUPPORTED  # Cb != Cr
    g_info, g_coefs = _read("decode/s64x48_444_base_q90")
    two = dict(g_info, num_components=2, h=g_info["h"][:2], v=g_info["v"][:2], blocks_w=g_info["blocks_w"][:2], blocks_h=g_info["blocks_h"][:2],
               qtables=g_info["qtables"][:2])
    assert _call(two, g_coefs[:2])[0] == T.UNSUPPORTED
    assert _call(dict(info, color_model=2), coefs)[0] == T.UNSUPPORTED  # RGB
    # UNSUPPORTED: the range rule, over the real area only
    last = coefs[0][-1, -1]
    assert _call(info, coefs)[0] == 0
    last[0, 0], last[7, 7] = 1023, -1023
    assert _call(info, coefs)[0] == 0
    last[0, 0] = 1024
    assert _call(info, coefs)[0] == T.UNSUPPORTED
    last[0, 0], last[7, 7] = 1023, -1024
    assert _call(info, coefs)[0] == T.UNSUPPORTED
    last[0, 0], last[7, 7] = 1024, -1024
    assert _call(info, coefs)[0] == T.UNSUPPORTED
    last[0, 0], last[7, 7] = -1024, 1023  # the DC value's own lower limit
    assert _call(info, coefs)[0] == 0
    last[0, 0], last[7, 7] = 0, 0
    want = lowlevel.encode_coefficients_host(info, coefs)
    padded = [np.zeros((c.shape[0], c.shape[1] + 2, 8, 8), dtype=np.int16) for c in coefs]
    for p, c in zip(padded, coefs):
        p[:, : c.shape[1]] = c
        p[:, c.shape[1]:, 7, 7] = -1024  # the same AC value where nobody reads
        p[:, c.shape[1]:, 0, 0] = 1024
    st, n = _call(info, padded)
    assert st == 0 and n == len(want)
    assert lowlevel.encode_coefficients_host(info, padded) == want
    # BUFFER_TOO_SMALL reports the needed size
    assert _call(info, coefs, capacity=len(want) - 1) == (T.BUFFER_TOO_SMALL, len(want))
    assert _call(info, coefs, capacity=0) == (T.BUFFER_TOO_SMALL, len(want))
    assert _call(info, coefs, capacity=len(want)) == (0, len(want))


def test_python_surface_validates_arrays():
    info, coefs = _read("decode/s17x13_420_base_q90")
    with pytest.raises(TypeError):
        lowlevel.encode_coefficients_host(info, [c.astype(np.int32) for c in coefs])
    with pytest.raises(TypeError):
        lowlevel.encode_coefficients_host(info, [c[:, ::-1] for c in coefs])
    with pytest.raises(TypeError):
        lowlevel.encode_coefficients_host(info, coefs[:2])


# ---------------------------------------------------------------- 6. sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_routes_are_clean_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (tests/sanitizers/coefficients_roundtrip.cpp), never through Python"""
    exe = str(tmp_path / "coefficients_roundtrip")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "coefficients_roundtrip.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "entropy_decode.cpp", "entropy_encode.cpp", "transcode_core.cpp", "coefficients_core.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    truncated = tmp_path / "truncated.jpg"
    truncated.write_bytes(_golden("s64x48_420_base_q90")[:700])
    files = [os.path.join(GOLDEN, "decode", n + ".jpg") for n in ("s1x1_gray_base_q90", "s1x1_420_base_q90", "s3x5_420_base_q90", "s3x5_gray_base_q90",
                                                                  "s17x13_420_base_q90", "s17x13_420_prog_q50")]
    files += sorted(glob.glob(os.path.join(GOLDEN, "cmyk", "*.jpg")))[:1] + [os.path.join(GOLDEN, "damaged", "padding_block_damage.jpg"), str(truncated)]
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "9 files, 6 written, 3 refused, 0 wrong results" in run.stdout, run.stdout
