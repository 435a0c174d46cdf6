"""Sequential frames whose components are coded in several scans, or in one scan in another component order
(helpers/sequential_scans.py re-codes the goldens so), through the GPU entropy decoder's algorithm emulated on the host: every scan is a
stream of its own.  The coefficients must equal the host entropy decoder's and the oracle's over the whole buffer, padding blocks
included; damaged scans must get the host decoder's verdict.  tests/test_gpu_multiscan_sequential.py decodes the same files on the GPU."""
import functools
import hashlib
import io
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import sampling_goldens as G
from helpers import sequential_scans as S
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

SCRIPTS3 = [[[0], [1], [2]], [[0], [1, 2]], [[1, 2], [0]], [[2], [1], [0]], [[2, 0, 1]]]
SCRIPTS4 = [[[0, 1], [2, 3]], [[3], [1], [0, 2]]]


def _load(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def sequential_goldens():
    """(name, jpeg bytes, expected sha256 of the RGB / CMYK output, output kind) of every sequential golden with 3 or 4 components"""
    out = []
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        for e in json.load(f)["decode"]:
            if not e["progressive"] and e["sub"] != "gray":
                out.append((e["name"], _load(os.path.join("decode", e["name"] + ".jpg")), e["rgb_sha256"] if e["pixels"] else None, "rgb"))
    for e in G.ENTRIES:
        case = next(c for c in G.CASES if c["name"] == e["name"])
        if not case["progressive"] and len(case["sampling"]) > 1:
            out.append((e["name"], G.jpeg(e), e["sha256"], "cmyk" if len(case["sampling"]) == 4 else "rgb"))
    with open(os.path.join(GOLDEN, "manifest_cmyk.json")) as f:
        for e in json.load(f)["cmyk"]:
            if not e["progressive"]:
                out.append((e["name"], _load(os.path.join("cmyk", e["name"] + ".jpg")), e["cmyk_sha256"], "cmyk"))
    return out


def scripts_for(jpeg):
    return SCRIPTS4 if oracle.read_info(jpeg)["ncomp"] == 4 else SCRIPTS3


@functools.lru_cache(maxsize=None)
def recoded_goldens():
    """-> ([(name, script, re-coded bytes, sha, kind)], number of (file, script) pairs skipped: a DC difference out of category 11)"""
    out, skipped = [], 0
    for name, jpeg, sha, kind in sequential_goldens():
        for script in scripts_for(jpeg):
            try:
                out.append((name, script, S.recode(jpeg, script), sha, kind))
            except S.DcOutOfRange:
                skipped += 1
    return out, skipped


def _same_coefficients(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_emulation(data):
    host, _ = lowlevel.entropy_decode_host(data)
    emu, _ = lowlevel.entropy_decode_gpu_algorithm_host(data)
    orc, _ = oracle.decode_coefficients(data)
    assert _same_coefficients(emu, host)
    assert _same_coefficients(emu, orc)
    return emu


def test_writer_keeps_the_coefficients():
    items, skipped = recoded_goldens()
    assert items
    print("re-coded %d (file, script) pairs; skipped %d (a DC difference out of category 11)" % (len(items), skipped))
    assert skipped <= len(items) // 10
    originals = {name: jpeg for name, jpeg, _, _ in sequential_goldens()}
    for name, script, data, _, _ in items:
        ref, ref_q = oracle.decode_coefficients(originals[name])
        got, got_q = oracle.decode_coefficients(data)
        info = oracle.read_info(originals[name])
        assert all(np.array_equal(a, b) for a, b in zip(ref_q, got_q))
        for c, (a, b) in enumerate(zip(ref, got)):
            # the real blocks: a one-component scan codes no others (the padding of the grid decodes as zero)
            rw, rh = info["dw"][c], info["dh"][c]
            assert np.array_equal(a[:-(-rh // 8), :-(-rw // 8)], b[:-(-rh // 8), :-(-rw // 8)]), (name, script, c)


def test_writer_pixels_through_pillow():
    """libjpeg-turbo's decode of a re-coded file gives the golden pixels.  (It refuses a scan whose components are not in frame order
    -- T.81 B.2.3 asks for that order, this decoder does not -- so those scripts are left out here.)"""
    PIL = pytest.importorskip("PIL.Image")
    n = 0
    for name, script, data, sha, kind in recoded_goldens()[0]:
        if kind != "rgb" or sha is None or any(sorted(scan) != scan for scan in script):
            continue
        img = PIL.open(io.BytesIO(data))
        if img.mode != "RGB":
            continue
        assert hashlib.sha256(np.asarray(img).tobytes()).hexdigest() == sha, (name, script)
        n += 1
    assert n > 0


def test_emulation_across_the_goldens():
    """On a tree without per-scan streams the emulation refuses these files with UNSUPPORTED (status 3)."""
    for name, script, data, _, _ in recoded_goldens()[0]:
        try:
            _check_emulation(data)
        except AssertionError as e:
            raise AssertionError("%s %s" % (name, script)) from e


@pytest.mark.parametrize("w,h,sub", [(17, 13, "420"), (1283, 721, "411"), (320, 240, "422")])
@pytest.mark.parametrize("restarts", [[1, 7, 0], [0, 0, 0], [7, 1, 3]])
def test_restart_intervals_and_odd_sizes(w, h, sub, restarts):
    jpeg = oracle.encode(synth_image(w, h, seed=w + h), sub, 85)
    for script in ([[0], [1], [2]], [[1, 2], [0]]):
        data = S.recode(jpeg, script, restarts[:len(script)])
        emu = _check_emulation(data)
        info = oracle.read_info(data)
        # luma padding blocks, coded by no scan: zero
        assert not emu[0][-(-info["dh"][0] // 8):].any() and not emu[0][:, -(-info["dw"][0] // 8):].any()


def test_restart_interval_of_the_original_is_replaced():
    jpeg = oracle.encode(synth_image(96, 64, seed=3), "420", 90, restart_interval=2)
    _check_emulation(S.recode(jpeg, [[0], [1], [2]], [0, 5, 0]))
    _check_emulation(S.recode(jpeg, [[0], [1, 2]]))


def _status(fn, data):
    try:
        fn(data)
        return 0
    except N.HipJpegError as e:
        return e.status


def _scan_ranges(data):
    """(begin, end) of the entropy-coded bytes of every scan"""
    out, pos = [], 2
    while pos < len(data) - 1:
        m = data[pos + 1]
        if m == 0xDA:
            begin = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
            end = begin
            while not (data[end] == 0xFF and data[end + 1] not in (0x00,) and not 0xD0 <= data[end + 1] <= 0xD7):
                end += 1
            out.append((begin, end))
            pos = end
        else:
            pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return out


def test_damage_in_later_scans_gets_the_host_verdict():
    jpeg = oracle.encode(synth_image(160, 96, seed=11), "420", 90)
    data = S.recode(jpeg, [[0], [1], [2]], [0, 3, 0])
    ranges = _scan_ranges(data)
    assert len(ranges) == 3
    rng = np.random.default_rng(5)
    cases = []
    for s in (1, 2):
        b, e = ranges[s]
        for _ in range(6):
            k = int(rng.integers(b, e))
            if data[k] == 0xFF or data[k - 1] == 0xFF:
                continue
            flipped = bytearray(data)
            flipped[k] ^= 1 << int(rng.integers(0, 8))
            if flipped[k] == 0xFF:
                continue
            cases.append(bytes(flipped))
        cases.append(data[:(b + e) // 2] + b"\xff\xd9")
    # the kernels' verdict: a scan they cannot vouch for hands the picture to the host decoder, whose verdict is final; a scan they
    # decode must give what the host decoder gives
    flagged = 0
    for d in cases:
        host = _status(lowlevel.entropy_decode_host, d)
        emu = _status(lowlevel.entropy_decode_gpu_algorithm_host, d)
        if emu == 3:  # a cut scan with restart intervals lacks markers: the picture is not eligible, the host stage takes it
            continue
        flagged += emu != 0
        if emu == 0:
            assert host == 0
            assert _same_coefficients(lowlevel.entropy_decode_host(d)[0], lowlevel.entropy_decode_gpu_algorithm_host(d)[0])
    assert flagged > 0


def test_missing_or_twice_coded_component_stays_unsupported():
    jpeg = oracle.encode(synth_image(64, 48, seed=2), "420", 90)
    for script in ([[0], [1]], [[0], [1], [2], [1]], [[0, 1, 2], [2]]):
        data = S.recode(jpeg, script)
        assert _status(lowlevel.entropy_decode_gpu_algorithm_host, data) == 3, script
