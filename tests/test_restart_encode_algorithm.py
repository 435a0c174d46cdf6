"""The GPU entropy coder's baseline algorithm with restart intervals (csrc/huffman_encode_core.h) executed on the host with the
kernels' own code (hipjpegEncodeBaselineGpuAlgorithmHost, no GPU): predictor reset per interval, the segmented scan of the bit
offsets, padding with one-bits, RSTn markers in the bit buffer and the byte stuffing that spares them must give the host coder's file
byte for byte -- and with it libjpeg-turbo's, to which the host coder is pinned."""
import re

import numpy as np
import pytest

import oracle
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

_UNSUPPORTED = 3  # HIPJPEG_STATUS_UNSUPPORTED
SUBS = ["444", "422", "420", "440", "411", "410", "gray"]
SIZES = ((1, 1), (7, 9), (17, 13), (33, 65), (257, 66))
QUALITIES = (1, 50, 90, 100)
_MCU = {"444": (8, 8), "422": (16, 8), "420": (16, 16), "440": (8, 16), "411": (32, 8), "410": (32, 16), "gray": (8, 8)}


def mcu_grid(w, h, sub):
    mw, mh = _MCU[sub]
    return (w + mw - 1) // mw, (h + mh - 1) // mh


def intervals(w, h, sub):
    """0, 1, 2, 3, 7, one MCU row, exactly the MCU count, more than the MCU count, 65535."""
    mx, my = mcu_grid(w, h, sub)
    return [0, 1, 2, 3, 7, mx, mx * my, mx * my + 1, 65535]


def _both(w, h, coefs, sub, q, r, opt):
    want = lowlevel.encode_from_coefficients_host(w, h, coefs, sub, q, restart_interval=r, optimized_huffman=opt)
    got = lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(w, h, coefs, sub, q, restart_interval=r, optimized_huffman=opt)
    return got, want


@pytest.mark.parametrize("sub", SUBS)
def test_every_sampling_size_quality_interval_and_table(sub):
    for (w, h) in SIZES:
        rgb = synth_image(w, h, seed=w * 7 + h)
        for q in QUALITIES:
            coefs, _ = oracle.forward(rgb, sub, q)
            for r in intervals(w, h, sub):
                for opt in (False, True):
                    got, want = _both(w, h, coefs, sub, q, r, opt)
                    assert got == want, (sub, w, h, q, r, opt)
                # Annex-K tables: libjpeg-turbo's own file for the same picture
                assert lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(w, h, coefs, sub, q, restart_interval=r) == \
                    oracle.encode(rgb, sub, q, restart_interval=r), (sub, w, h, q, r)


def test_dri_segment_and_marker_sequence():
    """DRI sits between DHT and SOS; the markers count 0..7 and wrap; nothing follows the last interval even when the MCU count is
    a multiple of the interval."""
    w, h, sub = 64, 48, "444"  # 8 x 6 = 48 MCUs
    coefs, _ = oracle.forward(synth_image(w, h, seed=3), sub, 75)
    for r in (1, 4, 48):
        f = lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(w, h, coefs, sub, 75, restart_interval=r)
        sos = f.index(b"\xff\xda")
        assert f[sos - 6:sos] == b"\xff\xdd\x00\x04" + bytes([r >> 8, r & 255])
        scan = f[sos:]
        found = [m[1] - 0xD0 for m in re.findall(rb"\xff[\xd0-\xd7]", scan)]
        assert found == [i % 8 for i in range((48 + r - 1) // r - 1)]
        assert scan[-2:] == b"\xff\xd9" and scan[-4:-2] not in [bytes([0xFF, 0xD0 + i]) for i in range(8)]
        assert lowlevel.get_image_info(f)["restart_interval"] == r and oracle.read_info(f)["restart_interval"] == r


def _ends_in_ones_grids():
    """Coefficient grids whose intervals end in one-bits.  A block whose coefficient at zigzag position 63 is not zero emits no EOB,
    and 1023 there ends the block in ten one-bits: whatever the alignment, the interval's last byte is 0xFF -- either data alone or
    data and padding -- and it is the last byte before the marker.  Random sparse coefficients in front vary the alignment."""
    rng = np.random.default_rng(11)
    zz63 = 63  # natural index 63 is zigzag position 63
    g = np.zeros((8, 8, 64), np.int16)
    g[:, :, 0] = rng.integers(-200, 200, size=(8, 8))
    for _ in range(3):
        g[rng.integers(0, 8, 40), rng.integers(0, 8, 40), rng.integers(1, 63, 40)] = rng.integers(-30, 31, 40)
    g[:, :, zz63] = 1023
    yield 64, 64, "gray", [g], 1
    yield 64, 64, "gray", [g], 3
    # 4:2:0: the MCU's last block is Cr; the luma grid is MCU-padded (60 x 40 -> 4 x 3 MCUs with dummy blocks at both edges)
    y = np.zeros((6, 8, 64), np.int16)
    y[:, :, 0] = rng.integers(-100, 100, size=(6, 8))
    y[rng.integers(0, 5, 30), rng.integers(0, 8, 30), rng.integers(1, 64, 30)] = rng.integers(-9, 10, 30)
    cb = np.zeros((3, 4, 64), np.int16)
    cb[:, :, 5] = rng.integers(-3, 4, size=(3, 4))
    cr = np.zeros((3, 4, 64), np.int16)
    cr[:, :, 0] = rng.integers(-50, 50, size=(3, 4))
    cr[:, :, zz63] = 1023
    yield 60, 40, "420", [y, cb, cr], 1
    yield 60, 40, "420", [y, cb, cr], 4


def test_stuffed_byte_in_front_of_a_marker():
    for (w, h, sub, coefs, r) in _ends_in_ones_grids():
        for opt in (False, True):
            got, want = _both(w, h, coefs, sub, 100, r, opt)
            scan = want[want.index(b"\xff\xda"):]
            assert re.search(rb"\xff\x00\xff[\xd0-\xd7]", scan), "the host coder's file has no stuffed 0xFF in front of a marker"
            assert got == want, (w, h, sub, r, opt)


def test_padded_byte_of_ones_is_stuffed():
    """An interval whose data ends byte-aligned minus a few bits, all of them ones, so that the padding completes a 0xFF byte."""
    hits = 0
    for v in range(1, 40):  # DC differences of growing length shift the end of the block through every alignment
        g = np.zeros((1, 16, 64), np.int16)
        g[0, :, 0] = np.arange(16) * v
        g[0, :, 63] = 1
        got, want = _both(128, 8, [g], "gray", 100, 1, False)
        assert got == want, v
        hits += len(re.findall(rb"\xff\x00\xff[\xd0-\xd7]", want[want.index(b"\xff\xda"):]))
    assert hits > 0


def test_progressive_output_is_not_taken():
    coefs, _ = oracle.forward(synth_image(16, 16, seed=1), "444", 75)
    for r in (0, 2):
        with pytest.raises(N.HipJpegError) as e:
            lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(16, 16, coefs, "444", 75, restart_interval=r, progressive=True)
        assert e.value.status == _UNSUPPORTED


def test_interval_out_of_range_is_refused():
    coefs, _ = oracle.forward(synth_image(16, 16, seed=1), "444", 75)
    for r in (-1, 65536):
        with pytest.raises(N.HipJpegError):
            lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(16, 16, coefs, "444", 75, restart_interval=r)


def test_large_picture_many_intervals():
    """More intervals than lanes in the scan's workgroup, so that lanes' ranges hold several boundaries and the spans compose."""
    rgb = synth_image(640, 480, seed=5)
    for sub in ("420", "gray"):
        coefs, _ = oracle.forward(rgb, sub, 85)
        for r in (1, 5, mcu_grid(640, 480, sub)[0]):
            for opt in (False, True):
                got, want = _both(640, 480, coefs, sub, 85, r, opt)
                assert got == want, (sub, r, opt)
