"""The lossless (SOF3) coder without a GPU: hipjpegEncodeLosslessHost (sample by sample, as the library codes) and
hipjpegEncodeLosslessGpuAlgorithmHost (the kernels' groups, windows, segmented scan and chunks, lane by lane) give libjpeg-turbo's file
byte for byte on every golden of tests/golden/make_golden_lossless_encode.py, equal the numpy model on the kernels' seams, and what
they write decodes back to (samples >> Pt) << Pt."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_encode_model as M
from helpers import lossless_encode_seams as S
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel as LL

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_lossless_encode.json")))["lossless_encode"]
CODERS = {"host": LL.encode_lossless_host, "twin": LL.encode_lossless_gpu_algorithm_host}


def test_manifest_covers_what_the_coder_promises():
    P = {e["precision"] for e in MANIFEST}
    assert {2, 8, 9, 12, 16} <= P and {e["predictor"] for e in MANIFEST} == set(range(1, 8)) and {e["components"] for e in MANIFEST} == {1, 2, 3, 4}
    assert any(e["point_transform"] for e in MANIFEST) and any(not e["point_transform"] for e in MANIFEST)
    assert any(e["restart_rows"] == 1 and e["height"] > 8 for e in MANIFEST) and any(e["restart_rows"] and e["height"] % e["restart_rows"] for e in MANIFEST)
    assert {(1, 1)} <= {(e["height"], e["width"]) for e in MANIFEST} and any(e["height"] == 1 < e["width"] for e in MANIFEST)
    assert any(e["width"] == 1 < e["height"] for e in MANIFEST) and {"constant", "ssss16"} <= {e["kind"] for e in MANIFEST}
    assert any(not e["stored"] for e in MANIFEST)


@pytest.mark.parametrize("coder", sorted(CODERS))
def test_goldens_byte_for_byte(coder):
    for e in MANIFEST:
        s = M.case_samples(e)
        data = CODERS[coder](s, e["precision"], e["predictor"], e["point_transform"], e["restart_rows"])
        assert hashlib.sha256(data).hexdigest() == e["sha256"] and len(data) == e["bytes"], e["name"]
        if e["stored"]:
            assert data == open(os.path.join(GOLDEN, "lossless_encode", e["name"] + ".jpg"), "rb").read(), e["name"]
        got = LL.decode_lossless_host(data, dtype=s.dtype)
        assert np.array_equal(got, M.expected(s, e["point_transform"])), e["name"]


def test_planar_input_gives_the_same_file():
    for e in MANIFEST[:12]:
        s = M.case_samples(e)
        planar = np.ascontiguousarray(s.transpose(2, 0, 1))
        for fn in CODERS.values():
            data = fn(planar, e["precision"], e["predictor"], e["point_transform"], e["restart_rows"], planar=True)
            assert hashlib.sha256(data).hexdigest() == e["sha256"], e["name"]


def _seam_cases():
    shape = LL.lossless_encode_shape()
    return S.cases(shape) + S.searched_cases(shape)


def test_seams_equal_the_model_and_decode_back():
    shape = LL.lossless_encode_shape()
    assert shape["group_samples"] >= 2 and shape["window_samples"] % shape["group_samples"] == 0 and shape["chunk_bytes"] >= 16
    cases = _seam_cases()
    assert len(cases) > 50
    for c in cases:
        x, n, keep = M.padded_input(N, c["samples"], c["planar"], c["pad"], c["offset"])
        want = M.model_file(c["samples"], c["precision"], c["predictor"], c["point_transform"], c["restart_rows"])
        for name, fn in (("host", "hipjpegEncodeLosslessHost"), ("twin", "hipjpegEncodeLosslessGpuAlgorithmHost")):
            st, data = M.encode_raw_host(fn, x, n, c["precision"], c["predictor"], c["point_transform"], c["restart_rows"])
            assert st == 0 and data == want, (c["name"], name)
        got = LL.decode_lossless_host(want, dtype=c["samples"].dtype)
        assert np.array_equal(got, M.expected(c["samples"], c["point_transform"])), c["name"]
        del keep


def test_searched_seams_have_their_property():
    shape = LL.lossless_encode_shape()
    chunk = shape["chunk_bytes"]
    by_name = {c["name"]: c for c in S.searched_cases(shape)}
    for name, at in (("ff_last_of_chunk", chunk - 1), ("ff_first_of_chunk", chunk)):
        c = by_name[name]
        data = LL.encode_lossless_gpu_algorithm_host(c["samples"], 16, 1)
        raw = S.unstuffed_scan(data, 1)
        assert chunk < len(raw) <= 2 * chunk and raw[at] == 0xFF, name
    c = by_name["ff_before_rst"]
    data = LL.encode_lossless_gpu_algorithm_host(c["samples"], 16, 1, restart_rows=1)
    assert any(bytes([0xFF, 0, 0xFF, 0xD0 + k]) in data for k in range(8))
    # where the first interval ends, read from the twin's own file: the code lengths of ITS table (DHT) give the interval's bits, and its
    # first RSTn must stand at exactly that many bits (on the byte), or one padding bit behind them (one bit short)
    for name, tail in (("interval_ends_on_byte", 0), ("interval_one_bit_short", 7)):
        c = by_name[name]
        data = LL.encode_lossless_gpu_algorithm_host(c["samples"], 12, 1, restart_rows=2)
        dht = data.index(b"\xff\xc4")
        bits = [0] + list(data[dht + 5:dht + 21])
        lut = S.LF._codes(bits, list(data[dht + 21:dht + 21 + sum(bits)]))
        ssss, _ = S.LF.categories(M.differences(c["samples"], 12, 1, 0, 2)[:2])
        nbits = int(sum(lut[int(k)][1] + (0 if k == 16 else int(k)) for k in ssss.ravel()))
        assert nbits % 8 == tail, name
        scan = data[M.parse(data)["scan_at"]:]
        first = scan.replace(b"\xff\x00", b"\xff\x01").index(b"\xff\xd0")  # (a stuffed FF 00 cannot be taken for the marker)
        stuffed = scan[:first].count(b"\xff\x00")
        assert first - stuffed == (nbits + 7) // 8 and (nbits + 7) // 8 * 8 - nbits == (8 - tail) % 8, name
        if tail == 7:
            assert scan[first - 1] & 1 == 1  # the one padding bit


def _status(fn, x, p):
    need = ctypes.c_size_t(0)
    return getattr(N.load(), fn)(ctypes.byref(x), ctypes.byref(p), None, 0, ctypes.byref(need))


@pytest.mark.parametrize("fn", ["hipjpegEncodeLosslessHost", "hipjpegEncodeLosslessGpuAlgorithmHost"])
def test_invalid_arguments(fn):
    s = np.zeros((4, 6, 3), dtype=np.uint16)
    x, n = LL.lossless_encode_input(s.ctypes.data, s.shape, s.strides, 2, False)
    good = dict(precision=12, predictor=1, point_transform=0, restart_rows=0, num_components=3)
    assert _status(fn, x, N.LosslessEncodeParams(**good)) == 9  # BUFFER_TOO_SMALL: everything else is fine
    for bad in (dict(precision=1), dict(precision=17), dict(predictor=0), dict(predictor=8), dict(point_transform=12), dict(point_transform=-1),
                dict(num_components=0), dict(num_components=5), dict(restart_rows=-1)):
        assert _status(fn, x, N.LosslessEncodeParams(**dict(good, **bad))) == 1, bad
    s8 = np.zeros((4, 6, 3), dtype=np.uint8)
    x8, _ = LL.lossless_encode_input(s8.ctypes.data, s8.shape, s8.strides, 1, False)
    assert _status(fn, x8, N.LosslessEncodeParams(**dict(good, precision=9))) == 1
    assert _status(fn, x8, N.LosslessEncodeParams(**dict(good, precision=8))) == 9
    short, _ = LL.lossless_encode_input(s.ctypes.data, s.shape, s.strides, 2, False)
    short.pitch[0] = 6 * 3 * 2 - 1
    assert _status(fn, short, N.LosslessEncodeParams(**good)) == 1
    planar = np.zeros((3, 4, 6), dtype=np.uint16)
    xp, _ = LL.lossless_encode_input(planar.ctypes.data, planar.shape, planar.strides, 2, True)
    assert _status(fn, xp, N.LosslessEncodeParams(**good)) == 9
    xp.pitch[2] = 11
    assert _status(fn, xp, N.LosslessEncodeParams(**good)) == 1
    xp.pitch[2] = 12
    xp.plane[1] = None
    assert _status(fn, xp, N.LosslessEncodeParams(**good)) == 1
    for field, value in (("sample_bytes", 3), ("width", 0), ("height", 0), ("width", 65536)):
        y, _ = LL.lossless_encode_input(s.ctypes.data, s.shape, s.strides, 2, False)
        setattr(y, field, value)
        assert _status(fn, y, N.LosslessEncodeParams(**good)) == 1, field
    assert getattr(N.load(), fn)(None, None, None, 0, None) == 1
    # DRI is 16 bits: restart_rows * width may be 65535 and no more (the library would clamp it to a value that is no whole rows)
    wide = np.zeros((3, 21845, 1), dtype=np.uint8)
    xw, _ = LL.lossless_encode_input(wide.ctypes.data, wide.shape, wide.strides, 1, False)
    assert _status(fn, xw, N.LosslessEncodeParams(8, 1, 0, 3, 1)) == 9
    wider = np.zeros((3, 21846, 1), dtype=np.uint8)
    xw, _ = LL.lossless_encode_input(wider.ctypes.data, wider.shape, wider.strides, 1, False)
    assert _status(fn, xw, N.LosslessEncodeParams(8, 1, 0, 3, 1)) == 1 and _status(fn, xw, N.LosslessEncodeParams(8, 1, 0, 0, 1)) == 9


def test_buffer_too_small_names_the_length():
    s = np.arange(35, dtype=np.uint8).reshape(5, 7, 1)
    data = LL.encode_lossless_host(s, 8)
    x, _ = LL.lossless_encode_input(s.ctypes.data, s.shape, s.strides, 1, False)
    p = N.LosslessEncodeParams(8, 1, 0, 0, 1)
    out = np.full(len(data), 0xEE, dtype=np.uint8)
    need = ctypes.c_size_t(0)
    assert N.load().hipjpegEncodeLosslessHost(ctypes.byref(x), ctypes.byref(p), out.ctypes.data, len(data) - 1, ctypes.byref(need)) == 9
    assert need.value == len(data) and (out == 0xEE).all()
    assert N.load().hipjpegEncodeLosslessHost(ctypes.byref(x), ctypes.byref(p), out.ctypes.data, len(data), ctypes.byref(need)) == 0
    assert out.tobytes() == data


def test_bit_offset_predicate_at_its_edge():
    """31 bits per sample and 24 per interval must fit a uint32"""
    fits = LL.lossless_encode_fits_gpu
    top = 0xFFFFFFFF
    n = top // 31
    assert fits(n, 0) and not fits(n + 1, 0)
    k = (top - 31 * (n - 10)) // 24
    assert fits(n - 10, k) and not fits(n - 10, k + 1)
    assert fits(1, 1) and not fits(1 << 40, 1) and not fits(1, 1 << 62)
    # the twin turns away what the kernels would: 12000 x 12000 x 1 is beyond the bound, and nothing is coded (no buffer is touched)
    x = N.LosslessEncodeInput()
    dummy = np.zeros(16, dtype=np.uint8)
    x.plane[0], x.pitch[0], x.sample_bytes, x.planar, x.width, x.height = dummy.ctypes.data, 24000, 2, 0, 12000, 12000
    assert not fits(12000 * 12000, 1)
    assert _status("hipjpegEncodeLosslessGpuAlgorithmHost", x, N.LosslessEncodeParams(16, 1, 0, 0, 1)) == 3
