"""The GPU entropy coder's progressive algorithm with restart intervals (csrc/progressive_encode_core.h, template <bool RST>) executed
on the host with the kernels' own code (hipjpegEncodeProgressiveGpuAlgorithmHost, no GPU): the predictor reset, the flush of the
EOB run and its buffered correction bits at every interval end, the segmented scan of the bit offsets, padding with one-bits, RSTn
markers in the bit buffer and the byte stuffing that spares them must give the host coder's SOF2 file byte for byte -- and with it
libjpeg-turbo's, to which the host coder is pinned (jcphuff.c emit_restart)."""
import json
import os
import re

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image
from test_restart_encode_algorithm import QUALITIES, SIZES, SUBS, _MCU, intervals, mcu_grid

_UNSUPPORTED = 3  # HIPJPEG_STATUS_UNSUPPORTED

with open(os.path.join(GOLDEN, "manifest_encode_prog.json")) as _f:
    _RST_GOLDENS = [e for e in json.load(_f)["encode_progressive"] if e["restart"]]


def _both(w, h, coefs, sub, q, r):
    want = lowlevel.encode_from_coefficients_host(w, h, coefs, sub, q, restart_interval=r, progressive=True)
    got = lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(w, h, coefs, sub, q, restart_interval=r)
    return got, want


def _markers(f):
    """The RSTn numbers of every scan of a file, scan by scan (stuffed data cannot look like a marker)."""
    scans = f.split(b"\xff\xda")[1:]
    return [[m[1] - 0xD0 for m in re.findall(rb"\xff[\xd0-\xd7]", s)] for s in scans]


def test_there_are_three_goldens_with_a_restart_interval():
    assert len(_RST_GOLDENS) == 3


@pytest.mark.parametrize("entry", _RST_GOLDENS, ids=lambda e: e["name"])
def test_golden_files(entry):
    rgb = np.fromfile(os.path.join(GOLDEN, entry["input"]), dtype=np.uint8).reshape(entry["height"], entry["width"], 3)
    coefs, _ = oracle.forward(rgb, entry["sub"], entry["quality"])
    with open(os.path.join(GOLDEN, "encode_prog", entry["name"] + ".jpg"), "rb") as f:
        golden = f.read()
    got, want = _both(entry["width"], entry["height"], coefs, entry["sub"], entry["quality"], entry["restart"])
    assert got == want == golden


@pytest.mark.parametrize("sub", SUBS)
def test_every_sampling_size_quality_and_interval(sub):
    for (w, h) in SIZES:
        rgb = synth_image(w, h, seed=w * 7 + h)
        for q in QUALITIES:
            coefs, _ = oracle.forward(rgb, sub, q)
            for r in intervals(w, h, sub):
                got, want = _both(w, h, coefs, sub, q, r)
                assert got == want, (sub, w, h, q, r)


@pytest.mark.parametrize("sub", ["420", "gray"])
def test_interval_0_is_the_existing_entry_point(sub):
    for (w, h) in SIZES:
        coefs, _ = oracle.forward(synth_image(w, h, seed=w + h), sub, 90)
        assert lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(w, h, coefs, sub, 90) == \
            lowlevel.encode_from_coefficients_gpu_algorithm_host(w, h, coefs, sub, 90), (sub, w, h)


def test_dri_segment_and_marker_sequence():
    """One DRI, between the first scan's DHT and its SOS; in every scan the markers count 0..7 and wrap, and nothing follows the last
    interval even when the MCU count is a multiple of the interval.  An MCU is bpm blocks in the interleaved DC scans and one block in
    the AC scans: 4:2:0 at 64 x 48 has 12 MCUs, 48 luma blocks and 12 blocks per chroma component."""
    w, h, sub = 64, 48, "420"
    coefs, _ = oracle.forward(synth_image(w, h, seed=3), sub, 75)
    units = [12, 48, 12, 12, 48, 48, 12, 12, 12, 48]  # jpeg_simple_progression: DC, Y 1-5, Cr, Cb, Y 6-63, Y refine, DC refine, Cr, Cb, Y
    for r in (1, 4, 12, 48):
        f = lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(w, h, coefs, sub, 75, restart_interval=r)
        assert f.count(b"\xff\xdd\x00\x04") == 1
        sos = f.index(b"\xff\xda")
        assert f[sos - 6:sos] == b"\xff\xdd\x00\x04" + bytes([r >> 8, r & 255])
        assert _markers(f) == [[i % 8 for i in range((n + r - 1) // r - 1)] for n in units]
        assert lowlevel.get_image_info(f)["restart_interval"] == r


def test_all_zero_blocks_flush_a_run_at_every_interval_end():
    """184 x 184 all-zero blocks: every block of every AC scan only lengthens the run, so each interval end flushes a run of the
    interval's length (EOB0 for r = 1, EOB1 + 1 bit for r = 3, ...); r = 33000: the run is cut at 0x7FFF before the interval ends and
    the interval end flushes the other 233."""
    coefs = [np.zeros((184, 184, 64), np.int16)]
    for r in (1, 3, 100, 184, 33000):
        got, want = _both(184 * 8, 184 * 8, coefs, "gray", 100, r)
        assert got == want, r


def test_interval_end_flushes_carry_buffered_correction_bits():
    """8 x 64 blocks whose AC values are all 2 or 3: in the refinement scans a block has no symbol of its own and only buffers its 63
    correction bits, so the interval-end flushes carry the bits of the interval's blocks; r = 20: 63 x 15 = 945 > 937 cuts the run
    inside an interval and the interval end flushes the other five blocks' bits; r = 64: one grid row per interval."""
    rng = np.random.default_rng(7)
    c = np.zeros((8, 64, 64), np.int16)
    c[:, :, 1:] = rng.integers(2, 4, size=(8, 64, 63))
    for r in (1, 5, 20, 64):
        got, want = _both(512, 64, [c], "gray", 100, r)
        assert got == want, r


def test_dummy_block_dc_values_at_interval_starts():
    """The sparse 4:2:0 grid of test_progressive_encode_algorithm.py::test_long_runs_and_extreme_coefficients, 40 x 40 = 3 x 3 MCUs
    over 5 x 5 real luma blocks: the MCUs of the last column and row open intervals with dummy blocks next to them."""
    sparse = [np.zeros((6, 6, 64), np.int16), np.zeros((3, 3, 64), np.int16), np.zeros((3, 3, 64), np.int16)]
    sparse[0][::2, ::3, 40] = 1
    sparse[0][1, 1, 63] = -1
    sparse[1][2, 2, 17] = -5
    sparse[2][0, 0, 0] = 3
    for r in (1, 2):
        got, want = _both(40, 40, sparse, "420", 100, r)
        assert got == want, r
    # and with DC values that differ from block to block, so that a wrong predictor shows
    rng = np.random.default_rng(3)
    for c in sparse:
        c[:, :, 0] = rng.integers(-300, 300, size=c.shape[:2])
    for r in (1, 2):
        got, want = _both(40, 40, sparse, "420", 100, r)
        assert got == want, r


def test_baseline_output_is_not_taken():
    coefs, _ = oracle.forward(synth_image(16, 16, seed=1), "444", 75)
    for r in (0, 2):
        with pytest.raises(N.HipJpegError) as e:
            lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(16, 16, coefs, "444", 75, restart_interval=r, progressive=False)
        assert e.value.status == _UNSUPPORTED


def test_the_existing_entry_point_still_refuses_an_interval():
    coefs, _ = oracle.forward(synth_image(16, 16, seed=1), "444", 75)
    with pytest.raises(N.HipJpegError) as e:
        lowlevel.encode_from_coefficients_gpu_algorithm_host(16, 16, coefs, "444", 75, restart_interval=2)
    assert e.value.status == _UNSUPPORTED


def test_interval_out_of_range_is_refused():
    coefs, _ = oracle.forward(synth_image(16, 16, seed=1), "444", 75)
    for r in (-1, 65536):
        with pytest.raises(N.HipJpegError) as got:
            lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(16, 16, coefs, "444", 75, restart_interval=r)
        with pytest.raises(N.HipJpegError) as base:
            lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(16, 16, coefs, "444", 75, restart_interval=r)
        assert got.value.status == base.value.status


def _real_blocks(w, h, sub, c):
    mw, mh = _MCU[sub]
    sw, sh = (1, 1) if (c == 0 or sub == "gray") else (mw // 8, mh // 8)
    cw, ch = (w + sw - 1) // sw, (h + sh - 1) // sh
    return (cw + 7) // 8, (ch + 7) // 8


@pytest.mark.parametrize("sub,w,h,r", [("420", 257, 66, 3), ("gray", 33, 65, 2)])
def test_round_trip_through_the_interval_decoder(sub, w, h, r):
    """r is smaller than every scan's block count (the chroma scans of 257 x 66 4:2:0 have 17 x 5 blocks): every scan has markers.  The
    file decodes back to the coefficients that went in, through the host form of the interval decoder and the host entropy decoder."""
    coefs, _ = oracle.forward(synth_image(w, h, seed=w * 7 + h), sub, 90)
    f = lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(w, h, coefs, sub, 90, restart_interval=r)
    assert all(len(m) > 0 for m in _markers(f))
    for back in (lowlevel.entropy_decode_gpu_interval_algorithm_host(f), lowlevel.entropy_decode_host(f)[0]):
        assert len(back) == len(coefs)
        for c in range(len(coefs)):
            rw, rh = _real_blocks(w, h, sub, c)
            assert np.array_equal(back[c][:rh, :rw], coefs[c][:rh, :rw]), (sub, c)
