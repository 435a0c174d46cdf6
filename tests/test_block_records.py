"""Block-start records of the synchronisation decodes (csrc/huffman_gpu_core.h), checked WITHOUT a GPU.

hipjpegEntropyDecodeGpuAlgorithmHost records through the same hook as the kernels.  Wherever a record is usable it must name
exactly the blocks, and the bit positions, that the position walk finds; otherwise the call returns
HIPJPEG_STATUS_INTERNAL_ERROR.  So every call below that succeeds, or fails with the host decoder's verdict, has passed that
check."""
import io
import json
import os
import random

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

INTERNAL_ERROR = 10
REC_SLOTS = 30  # blocks one record holds (kRecSlots)

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _M = json.load(_f)


def _same_as_oracle(jpeg):
    coefs, _ = lowlevel.entropy_decode_gpu_algorithm_host(jpeg)
    ref, _ = oracle.decode_coefficients(jpeg)
    assert all(np.array_equal(a, b) for a, b in zip(coefs, ref))


def _scan_bits_per_block(jpeg, blocks):
    sos = jpeg.rfind(b"\xff\xda")
    return (len(jpeg) - sos) * 8 / blocks


@pytest.mark.parametrize("entry", [e for e in _M["decode"] if not e["progressive"]], ids=lambda e: e["name"])
def test_records_match_the_position_walk_on_every_baseline_golden(entry):
    jpeg, _ = load_decode_case(entry)
    try:
        _same_as_oracle(jpeg)
    except N.HipJpegError as e:
        assert e.status == 3  # UNSUPPORTED: not a stream of the GPU entropy stage


def test_restart_interval_streams():
    """No records are taken across restart boundaries: these streams keep the full position walk and its damage check."""
    for (w, h, sub, q, ri) in ((640, 360, "420", 90, 1), (400, 300, "420", 85, 7), (333, 222, "444", 75, 64), (256, 200, "gray", 95, 5)):
        _same_as_oracle(oracle.encode(synth_image(w, h, seed=w + ri), sub, q, restart_interval=ri))


def test_flat_and_striped_pictures_overflow_the_records():
    """A constant picture codes a block in a few bits: far more than REC_SLOTS blocks start in one 1024-bit subsequence, the
    record overflows and the position walk takes the subsequence.  Stripes are periodic and overflow too."""
    flat = np.full((1080, 1920, 3), 90, np.uint8)
    stripes = np.full((1080, 1920, 3), 137, np.uint8)
    stripes[:, ::32] = 30  # (every 16th column: 48 bits per block, no overflow)
    for img, sub in ((flat, "420"), (flat, "444"), (flat[:, :, 0], "gray"), (stripes, "420")):
        jpeg = oracle.encode(img, sub, 90)
        blocks = 1920 * 1080 // 64 * (1 if sub == "gray" else 3 if sub == "444" else 1.5)
        assert _scan_bits_per_block(jpeg, blocks) < 1024 / (REC_SLOTS + 1), "the picture must overflow a record"
        _same_as_oracle(jpeg)


def test_photographs_at_several_qualities():
    for (w, h, sub, q) in ((1920, 1080, "420", 90), (1280, 720, "422", 98), (800, 600, "444", 50), (640, 480, "420", 10)):
        _same_as_oracle(oracle.encode(synth_image(w, h, seed=q), sub, q))


def test_damaged_streams_never_break_the_records():
    """Bit flips, overwrites and cuts: whatever the emulation concludes, it is never a record mismatch."""
    rng = random.Random(31337)
    bases = [oracle.encode(synth_image(w, h, seed=s), sub, q) for (w, h, sub, q, s) in
             ((640, 360, "420", 90, 1), (321, 243, "422", 75, 2), (200, 200, "444", 95, 3))]
    for n in range(40):
        b = bytearray(rng.choice(bases))
        sos = bytes(b).rfind(b"\xff\xda") + 14
        if n % 3 == 0:
            for _ in range(rng.randrange(1, 6)):
                i = rng.randrange(sos, len(b) - 2)
                b[i] ^= 1 << rng.randrange(8)
        elif n % 3 == 1:
            i = rng.randrange(sos, len(b) - 40)
            for k in range(rng.randrange(1, 32)):
                b[i + k] = rng.randrange(256)
        else:
            i = rng.randrange(sos, len(b) - 200)
            del b[i:i + rng.randrange(1, 150)]
        try:
            lowlevel.entropy_decode_gpu_algorithm_host(bytes(b))
        except N.HipJpegError as e:
            assert e.status != INTERNAL_ERROR, n


def test_pillow_streams():
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow makes the inputs")
    for seed in (1234, 1237):
        b = io.BytesIO()
        Image.fromarray(synth_image(1920, 1080, seed=seed)).save(b, "JPEG", quality=90, subsampling=2)
        _same_as_oracle(b.getvalue())
