"""The crafted restart-interval files of tests/helpers/progressive_interval_seams.py through the interval kernels
(csrc/progressive_intervals.hip) and the destuff kernels in front of them.  Every file is known to sit on the seam it names
(tests/test_progressive_interval_seams.py asserts the predicates over the writer's log, get() here does again); what only the device has -- the
unit word (component << 28) | first interval, workgroups of 256 lanes with the last one partly filled, the table slots in LDS clipped at the
pool's end, stream words behind the end read as ones, the destuff chunks -- is reached by construction.  Pixels must be the oracle's,
coefficient tensors the numbers the files were written from, and the counters must say who decoded what: a lane that wrongly gives up hands
the image to the host decoder, which the pixels alone would never show, and a lane that wrongly vouches for a refusal file would not be counted
as a takeover."""
import functools
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case
from helpers import progressive_interval_seams as I

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _names(kind):
    """(the files are written when a test first asks, not when the module is collected)"""
    return I.names(kind)


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def _neighbours():
    """two baseline goldens and two progressive goldens without restart intervals (the walk): they stand in the middle of every batch"""
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        entries = json.load(f)["decode"]
    pick = [e for e in entries if not e["progressive"]][:2] + [e for e in entries if e["progressive"] and "_rst" not in e["name"]][:2]
    assert len(pick) == 4
    return tuple(load_decode_case(e)[0] for e in pick)


@functools.lru_cache(maxsize=None)
def _reference(jpeg):
    return oracle.decode(jpeg)


def _batches():
    """three batches of good and over-limit files; the three table cases share the first (the largest slot, the pool that ends inside a
    slot, six slots with six tables)"""
    rest = [n for n in sorted(_names("good") + _names("over_limit")) if n not in I.TABLE_CASES]
    return [rest[0::3] + I.TABLE_CASES, rest[1::3], rest[2::3]]


def _decode_and_check(dec, names):
    import torch
    cases = [I.get(n) for n in names]
    jpegs = [c.jpeg for c in cases]
    jpegs[len(jpegs) // 2:len(jpegs) // 2] = _neighbours()
    outs, st = dec.decode(jpegs, fmt="rgb", gpu_huffman=True, gpu_progressive_intervals=True, check=False)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st), (names, list(st))
    stats = dec.stats()
    good, refused = sum(c.kind == "good" for c in cases), sum(c.kind == "refusal" for c in cases)
    # (a refusal is an image the interval kernels were given: it counts among theirs and among the takeovers)
    assert stats["interval_images"] == good + refused, stats
    assert stats["interval_takeovers"] == refused, stats
    assert dec.host_fallbacks() == 0
    if not refused:
        assert stats["gpu_entropy_images"] == good + len(_neighbours()), stats
    for i, (j, o) in enumerate(zip(jpegs, outs)):
        assert np.array_equal(o.cpu().numpy(), _reference(j)), i


@pytest.mark.parametrize("part", [0, 1, 2])
def test_seam_files_in_three_batches(dec, part):
    """reader, stuffing, division of work, tables and stages, the limits (a file on either side: the four over a limit decode through the
    host entropy stage and are not counted)"""
    assert sum(len(b) for b in _batches()) == len(_names("good")) + 4 and len(_names("over_limit")) == 4
    _decode_and_check(dec, _batches()[part])


def test_refusals_between_good_neighbours(dec):
    """the lanes refuse seven images by their own checks -- a run still open at an interval's end, a whole byte of ones behind the padding --,
    the host decoder takes exactly those, and the images around them are not disturbed"""
    good = ["starts_at_every_byte_of_a_word", "count_257_gray", "interleaved_dc_420", "last_interval_of_one_block"]
    refusals = _names("refusal")
    assert len(refusals) == 7
    _decode_and_check(dec, good[:2] + refusals[:4] + good[2:3] + refusals[4:] + good[3:])


def test_coefficient_tensors_are_the_numbers_the_files_were_written_from():
    """The reference is no decoder at all."""
    import torch
    from nvimagecodec_amd import lowlevel
    for names in (sorted(_names("good") + _names("over_limit")), _names("refusal")):
        cases = [I.get(n) for n in names]
        bc = lowlevel.BatchCoefficients(device=0, num_threads=4, gpu_huffman=True, gpu_progressive_intervals=True)
        statuses, images = bc.decode([c.jpeg for c in cases])
        torch.cuda.synchronize()
        assert list(statuses) == [0] * len(cases)
        if names is _names("refusal"):
            assert bc.stats()["interval_takeovers"] == len(cases), bc.stats()
        else:
            assert bc.stats()["gpu_decoded_images"] == len(_names("good")) and bc.stats()["interval_takeovers"] == 0, bc.stats()
        for c, im in zip(cases, images):
            assert len(im.coefs) == len(c.coefs)
            for k, t in enumerate(im.coefs):
                rows, cols = I.real_blocks(c, k)
                got = t.cpu().numpy()
                assert got.shape[0] >= rows and got.shape[1] >= cols and got.shape[2:] == (8, 8)
                want = np.asarray(c.coefs[k])[:rows, :cols].astype(np.int16).reshape(rows, cols, 8, 8)
                assert np.array_equal(got[:rows, :cols], want), (c.name, k)
        bc.close()
