"""The crafted progressive files of tests/helpers/progressive_seams.py through the kernels (csrc/progressive_gpu.hip).  Every file is known to
sit on the seam it names (tests/test_progressive_seams.py asserts the predicates over the writer's log, get() here does again); what only the
device has -- the word feed with its 64-word step and its long seek, the window that needs word 0 of the next load, windows skipped by a run,
the LDS rings between the stages and their two waits, the DC walker's four table slots, the largest launch -- is reached by construction.
Pixels must be the oracle's, coefficient tensors the numbers the files were written from, and the kernels must have vouched for every image:
a walk that wrongly gives up hands the image to the host decoder, which the pixels alone would never show."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case
from helpers import progressive_seams as S

pytestmark = pytest.mark.gpu

# the pixel stage declines this sampling layout in interleaved RGB (libjpeg would filter Cb with its h1v2 upsampler, tests/test_sampling_layouts.py):
# these files are decoded to planes
PLANES_ONLY = [n for n in S.CASES if "mcu_of_10" in n]
SEAMS = [n for n in sorted(S.CASES) if n not in S.RING_CASES and n not in PLANES_ONLY]


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def _baseline():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        entries = [e for e in json.load(f)["decode"] if not e["progressive"]][:2]
    return tuple(load_decode_case(e)[0] for e in entries)


def _decode_and_check(dec, names):
    import torch
    cases = [S.get(n) for n in names]
    jpegs = [c.jpeg for c in cases]
    jpegs[len(jpegs) // 2:len(jpegs) // 2] = _baseline()  # two baseline files in the middle of the batch
    outs, st = dec.decode(jpegs, fmt="rgb", gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st), (names, list(st))
    assert dec.stats()["gpu_entropy_images"] == sum(c.in_limit for c in cases) + len(_baseline())
    assert dec.host_fallbacks() == 0
    for i, (j, o) in enumerate(zip(jpegs, outs)):
        assert np.array_equal(o.cpu().numpy(), oracle.decode(j)), i


def test_seam_files_in_three_batches(dec):
    """window and chunk seams, run skips, stream ends, group seams, closing runs of sixteen, DC scans, the limits (a file on either side: the
    four over the limit decode through the host entropy stage and are not counted)"""
    assert sum(not S.get(n).in_limit for n in SEAMS) == 4
    for part in (SEAMS[0::3], SEAMS[1::3], SEAMS[2::3]):
        _decode_and_check(dec, part)


def test_rings_between_stages_of_very_different_speed(dec):
    """640 blocks, six stages: a dense first scan in front of five scans that are one run each, and five such scans in front of a dense last one --
    ten groups through rings of four, so both waits of the hand-over happen; alone and as the luma of a 4:2:0 picture"""
    _decode_and_check(dec, S.RING_CASES)


def test_ten_block_mcus_to_planes(dec):
    import torch
    cases = [S.get(n) for n in PLANES_ONLY]
    assert len(cases) == 2
    outs, st = dec.decode([c.jpeg for c in cases], fmt="yuv_planar", gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    assert list(st) == [0, 0] and dec.stats()["gpu_entropy_images"] == 2 and dec.host_fallbacks() == 0
    for c, o in zip(cases, outs):
        for a, b in zip(o, oracle.decode_planes(c.jpeg)):
            assert np.array_equal(a.cpu().numpy(), b), c.name


def test_coefficient_tensors_are_the_numbers_the_files_were_written_from():
    """The reference is no decoder at all."""
    import torch
    from nvimagecodec_amd import lowlevel
    names = sorted(S.CASES)
    cases = [S.get(n) for n in names]
    bc = lowlevel.BatchCoefficients(device=0, num_threads=4, gpu_huffman=True)
    statuses, images = bc.decode([c.jpeg for c in cases])
    torch.cuda.synchronize()
    assert list(statuses) == [0] * len(cases)
    assert bc.stats()["gpu_decoded_images"] == sum(c.in_limit for c in cases)
    for c, im in zip(cases, images):
        assert len(im.coefs) == len(c.coefs)
        for k, t in enumerate(im.coefs):
            rows, cols = S.real_blocks(c, k)
            got = t.cpu().numpy()
            assert got.shape[0] >= rows and got.shape[1] >= cols and got.shape[2:] == (8, 8)
            want = np.asarray(c.coefs[k])[:rows, :cols].astype(np.int16).reshape(rows, cols, 8, 8)
            assert np.array_equal(got[:rows, :cols], want), (c.name, k)
    bc.close()


def test_some_images_demoted_for_lds_and_some_kept():
    """HIPJPEG_PROG_LDS_LIMIT=65536: of four images the planner hands one to the host entropy stage, all decode to the oracle's pixels"""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "decode_partial_demotion.py")
    env = dict(os.environ)
    env["HIPJPEG_PROG_LDS_LIMIT"] = "65536"
    r = subprocess.run([sys.executable, helper], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("partial demotion ok"))
    taken = int(line.split()[-3])
    assert 0 < taken < 4 and taken == 3, line
