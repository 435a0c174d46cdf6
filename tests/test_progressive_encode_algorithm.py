"""The GPU entropy coder's progressive algorithm (csrc/progressive_encode_core.h) executed on the host with the kernels' per-block
code (hipjpegEncodeFromCoefficientsGpuAlgorithmHost, no GPU): block summaries, EOB-run resolution, lengths and bit emission must
give the host coder's SOF2 file byte for byte -- and with it libjpeg-turbo's, to which the host coder is pinned."""
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

_UNSUPPORTED = 3  # HIPJPEG_STATUS_UNSUPPORTED

with open(os.path.join(GOLDEN, "manifest_encode_prog.json")) as _f:
    _MP = json.load(_f)["encode_progressive"]


def _both(w, h, coefs, sub, q):
    want = lowlevel.encode_from_coefficients_host(w, h, coefs, sub, q, progressive=True)
    got = lowlevel.encode_from_coefficients_gpu_algorithm_host(w, h, coefs, sub, q)
    return got, want


@pytest.mark.parametrize("entry", _MP, ids=lambda e: e["name"])
def test_golden_files(entry):
    rgb = np.fromfile(os.path.join(GOLDEN, entry["input"]), dtype=np.uint8).reshape(entry["height"], entry["width"], 3)
    coefs, _ = oracle.forward(rgb, entry["sub"], entry["quality"])
    args = (entry["width"], entry["height"], coefs, entry["sub"], entry["quality"])
    if entry["restart"]:
        with pytest.raises(N.HipJpegError) as e:
            lowlevel.encode_from_coefficients_gpu_algorithm_host(*args, restart_interval=entry["restart"])
        assert e.value.status == _UNSUPPORTED
        return
    with open(os.path.join(GOLDEN, "encode_prog", entry["name"] + ".jpg"), "rb") as f:
        golden = f.read()
    got, want = _both(*args)
    assert got == want == golden


def test_baseline_output_is_not_taken():
    coefs, _ = oracle.forward(synth_image(16, 16, seed=1), "444", 75)
    with pytest.raises(N.HipJpegError) as e:
        lowlevel.encode_from_coefficients_gpu_algorithm_host(16, 16, coefs, "444", 75, progressive=False)
    assert e.value.status == _UNSUPPORTED


def test_long_runs_and_extreme_coefficients():
    """The grids of test_host_entropy_encode.py::test_progressive_coder_long_runs_and_extreme_coefficients: an all-zero picture of
    33,856 blocks (runs cut at 0x7FFF), refinement scans whose buffered correction bits pass 937, a quantizer of 1's extremes,
    sparse 4:2:0."""
    rng = np.random.default_rng(7)
    cases = [(184 * 8, 184 * 8, "gray", [np.zeros((184, 184, 64), np.int16)])]
    c = np.zeros((8, 64, 64), np.int16)
    c[:, :, 1:] = rng.integers(2, 4, size=(8, 64, 63))
    cases.append((512, 64, "gray", [c]))
    big = rng.integers(-1023, 1024, size=(4, 4, 64)).astype(np.int16)
    big[:, :, 0] = rng.integers(-1024, 1017, size=(4, 4))
    cases.append((32, 32, "gray", [big]))
    sparse = [np.zeros((6, 6, 64), np.int16), np.zeros((3, 3, 64), np.int16), np.zeros((3, 3, 64), np.int16)]
    sparse[0][::2, ::3, 40] = 1
    sparse[0][1, 1, 63] = -1
    sparse[1][2, 2, 17] = -5
    sparse[2][0, 0, 0] = 3
    cases.append((40, 40, "420", sparse))
    for (w, h, sub, coefs) in cases:
        got, want = _both(w, h, coefs, sub, 100)
        assert got == want, (w, h, sub)


@pytest.mark.parametrize("sub", ["444", "422", "420", "440", "411", "410", "gray"])
def test_every_sampling_size_and_quality(sub):
    for (w, h) in ((1, 1), (7, 9), (17, 13), (33, 65), (257, 66)):
        rgb = synth_image(w, h, seed=w * 7 + h)
        for q in (1, 50, 90, 100):
            coefs, _ = oracle.forward(rgb, sub, q)
            got, want = _both(w, h, coefs, sub, q)
            assert got == want, (sub, w, h, q)


def test_runs_cut_by_the_buffer_then_by_0x7fff():
    """Seeded random gray grids: a stretch of blocks whose refinement scans buffer many correction bits (the run is cut by the
    937-bit limit), then more than 0x7FFF empty blocks in the same run (cut by the length limit), then sparse new coefficients."""
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        bw, bh = 200, 180  # 36,000 blocks
        g = np.zeros((bh, bw, 64), np.int16)
        flat = g.reshape(-1, 64)
        k = int(rng.integers(40, 120))
        flat[:k, 1:] = rng.choice([-3, -2, 2, 3], size=(k, 63))  # already non-zero in the last scans: correction bits only
        tail = flat[k + 33000:]
        idx = rng.integers(0, tail.shape[0], size=50)
        tail[idx, rng.integers(1, 64, size=50)] = rng.choice([-1, 1, 5, -7], size=50)
        flat[:, 0] = rng.integers(-60, 60, size=flat.shape[0])
        got, want = _both(bw * 8, bh * 8, [g], "gray", 100)
        assert got == want, seed
