"""Lossless transcode on the host (no GPU): hipjpegTranscodeHost = host entropy decoder -> relayout -> host coder.  The file it
writes holds every coefficient and the tables of the source, in the coding the caller asks for -- where libjpeg-turbo's own
files exist for the same coefficients (tests/golden/encode_prog, the oracle's baseline encoder) it IS that file, byte for byte."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import transcode_cases as T
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

with open(os.path.join(GOLDEN, "manifest_encode_prog.json")) as _f:
    _MP = json.load(_f)["encode_progressive"]

_DECODE = T.golden_files("decode")
_GAMUT = T.golden_files("gamut")


def _status(data, **kw):
    try:
        return T.SUCCESS, lowlevel.transcode_host(data, **kw)
    except N.HipJpegError as e:
        return e.status, None


@pytest.mark.parametrize("entry", _MP, ids=lambda e: e["name"])
def test_transcodes_between_libjpeg_turbo_files_of_one_picture(entry):
    """Baseline <-> progressive <-> optimized of the same coefficients: each transcode lands on the file the library itself writes."""
    rgb = np.fromfile(os.path.join(GOLDEN, entry["input"]), dtype=np.uint8).reshape(entry["height"], entry["width"], 3)
    with open(os.path.join(GOLDEN, "encode_prog", entry["name"] + ".jpg"), "rb") as f:
        prog = f.read()
    base = oracle.encode(rgb, entry["sub"], entry["quality"])
    assert lowlevel.transcode_host(base, progressive=True, restart_interval=entry["restart"]) == prog
    assert lowlevel.transcode_host(prog) == base
    coefs, _ = oracle.forward(rgb, entry["sub"], entry["quality"])
    opt = lowlevel.encode_from_coefficients_host(entry["width"], entry["height"], coefs, entry["sub"], entry["quality"], optimized_huffman=True)
    assert lowlevel.transcode_host(base, optimized_huffman=True) == opt
    assert lowlevel.transcode_host(prog, optimized_huffman=True) == opt


def test_the_goldens_are_what_the_issue_counted():
    """127 decode goldens, all header-eligible; 32 of the 43 gamut files pass the header rules (7 have 16-bit tables, 4 unequal chroma tables)."""
    assert len(_DECODE) == 127 and all(T.header_eligible(d) for _, d in _DECODE)
    assert len(_GAMUT) == 43 and sum(T.header_eligible(d) for _, d in _GAMUT) == 32
    infos = [lowlevel.get_image_info(d) for _, d in _DECODE]
    assert sum(i["sof_marker"] == 0xC2 for i in infos) == 45 and sum(i["restart_interval"] != 0 for i in infos) == 8
    assert {(i["h"][0], i["v"][0]) for i in infos if i["num_components"] == 3} == T.LUMA_FACTORS
    assert any(i["num_components"] == 1 for i in infos)


@pytest.mark.parametrize("name,data", _DECODE + [(n, d) for n, d in _GAMUT if T.header_eligible(d)], ids=lambda v: v if isinstance(v, str) else "")
def test_every_header_eligible_golden_each_target(name, data):
    """SUCCESS exactly for the files the rules admit (computed here from the header and the oracle's coefficients, never from the call
    under test), UNSUPPORTED exactly for the others; a file that comes out holds the source's coefficients, tables and pixels."""
    header_ok, eligible = T.expected_eligible(data)
    assert header_ok
    if name in {n for n, _ in _DECODE}:
        assert eligible, "every decode golden transcodes"
    want_pixels = oracle.decode(data) if eligible else None
    for target, kw in T.TARGETS.items():
        st, out = _status(data, **kw)
        assert st == (T.SUCCESS if eligible else T.UNSUPPORTED), (name, target, N.STATUS_NAMES.get(st, st))
        if not eligible:
            continue
        info = lowlevel.get_image_info(out)
        assert info["sof_marker"] == (0xC2 if kw.get("progressive") else 0xC0) and info["restart_interval"] == kw.get("restart_interval", 0)
        T.same_picture(data, out)
        assert np.array_equal(oracle.decode(out), want_pixels), (name, target)
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(out))), np.asarray(Image.open(io.BytesIO(data)))), (name, target)


def test_refusals():
    cmyk = T.golden_files("cmyk")[0][1]
    assert _status(cmyk)[0] == T.UNSUPPORTED
    tables = [(d, oracle.decode_coefficients(d)[1]) for _, d in _GAMUT]
    assert all(T.frame_eligible(d) for d, _ in tables)
    wide = [d for d, q in tables if max(int(t.max()) for t in q) > 255]
    uneq = [d for d, q in tables if len(q) == 3 and not np.array_equal(q[1], q[2]) and d not in wide]
    assert len(wide) == 7 and len(uneq) == 4
    for data in (wide[0], uneq[0]):
        for kw in T.TARGETS.values():
            assert _status(data, **kw)[0] == T.UNSUPPORTED
    whole = _DECODE[0][1]
    assert _status(whole[: len(whole) * 2 // 3])[0] == T.TRUNCATED
    # a buffer that is too small: the needed length comes back, nothing is written
    a = np.frombuffer(whole, dtype=np.uint8)
    want = lowlevel.transcode_host(whole)
    p = N.TranscodeParams(0, 0, 0, 0)
    n = ctypes.c_size_t()
    out = np.full(len(want), 0xA5, dtype=np.uint8)
    assert N.load().hipjpegTranscodeHost(a.ctypes.data, a.size, ctypes.byref(p), out.ctypes.data, len(want) - 1, ctypes.byref(n)) == T.BUFFER_TOO_SMALL
    assert n.value == len(want) and bool((out == 0xA5).all())
    assert N.load().hipjpegTranscodeHost(a.ctypes.data, a.size, ctypes.byref(p), out.ctypes.data, len(want), ctypes.byref(n)) == T.SUCCESS
    assert out.tobytes() == want
    # parameters outside their range
    for bad in (N.TranscodeParams(0, 0, -1, 0), N.TranscodeParams(0, 0, 65536, 0), N.TranscodeParams(0, 0, 0, 1)):
        assert N.load().hipjpegTranscodeHost(a.ctypes.data, a.size, ctypes.byref(bad), out.ctypes.data, len(want), ctypes.byref(n)) == 1
