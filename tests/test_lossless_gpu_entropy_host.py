"""The GPU entropy stage of the lossless decoder, run on the CPU (no GPU needed): hipjpegLosslessEntropyAlgorithmHost takes a file
through the kernels' own schedule -- destuffing, pass 0, correction rounds, ripple launches, checks, sums, stores -- lane by lane.  Its
difference planes must be those of the host stage on every golden, and must decode as the numpy model says on files that put samples
on every seam of the schedule; it must say so when a walk cannot converge, and leave damaged files to the host stage's verdict."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_entropy_cases as EC
from helpers import lossless_files as LF
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

CASES = json.load(open(os.path.join(GOLDEN, "manifest_lossless.json")))["lossless"]


@pytest.fixture(scope="module")
def shape():
    return lowlevel.lossless_entropy_shape()


def reconstruct(planes, rr):
    """difference planes N x H x W -> what a decoder returns for them under predictor 1 at 16 bits"""
    return LF.model_decode(np.moveaxis(planes.astype(np.int64), 0, 2), 16, 1, 0, rr)


def test_the_shape_is_what_the_cases_are_built_for(shape):
    assert shape["subsequence_bits"] % 32 == 0 and shape["subsequence_bits"] >= 64  # a sample of 31 bits fits in the overshoot
    assert shape["subsequences_per_workgroup"] == 256
    assert shape["max_rounds"] >= 1 and shape["max_ripple_launches"] >= 1


def test_every_golden_gives_the_host_stages_differences_and_converges():
    assert len(CASES) == 172
    for c in CASES:
        f = open(os.path.join(GOLDEN, "lossless", c["name"] + ".jpg"), "rb").read()
        st, got, converged = lowlevel.lossless_entropy_algorithm_host(f)
        st_host, want = lowlevel.lossless_entropy_host(f)
        assert st == 0 and st_host == 0, c["name"]
        assert converged, c["name"]  # the cap on fallbacks: no natural file goes back to the host stage
        assert np.array_equal(got, want), c["name"]


def test_every_seam_decodes_as_the_model_says(shape):
    cases = EC.seam_cases(shape)
    assert len(cases) == 1 + 6 + 8 + 2 + 2 + 9 + 1 + 2 + 1 + 1
    for name, f, d, rr in cases:
        st, planes, converged = lowlevel.lossless_entropy_algorithm_host(f)
        assert st == 0 and converged, name
        assert np.array_equal(np.moveaxis(planes, 0, 2), (d & 0xFFFF).astype(np.uint16)), name
        assert np.array_equal(reconstruct(planes, rr), LF.model_decode(d, 16, 1, 0, rr)), name
        # and the twin did the work itself: the host stage's planes are the same, not the source of these
        assert np.array_equal(planes, lowlevel.lossless_entropy_host(f)[1]), name


def test_the_stuffed_cases_do_hold_a_stuffed_byte(shape):
    stuffed = [f for name, f, d, rr in EC.seam_cases(shape) if name.startswith("stuffed")]
    assert len(stuffed) == 2 and all(LF.has_stuffed_byte(f) for f in stuffed)


def test_a_stream_that_cannot_synchronise_is_reported(shape):
    f, d = EC.unsynchronisable(shape)
    st, planes, converged = lowlevel.lossless_entropy_algorithm_host(f)
    assert st == 0 and not converged
    assert not planes.any()  # the host stage's differences, as the batch call would upload them
    # one table for all three components (its code for a zero is two bits long, and a subsequence begins at an even bit): the phase
    # stays out of the compared state, and the same picture converges
    same = LF.write_differences(d, 8, 1, table=LF.LONG)
    st, planes, converged = lowlevel.lossless_entropy_algorithm_host(same)
    assert st == 0 and converged and not planes.any()


def host_status(f):
    try:
        lowlevel.decode_lossless_host(f)
        return 0
    except N.HipJpegError as e:
        return e.status


def test_bad_files_get_the_host_decoders_status():
    cases = EC.bad_cases()
    assert len(cases) == 8
    seen = set()
    for name, f in cases:
        want = host_status(f)
        st, planes, converged = lowlevel.lossless_entropy_algorithm_host(f)
        assert st == want, (name, N.STATUS_NAMES[st], N.STATUS_NAMES[want])
        seen.add(N.STATUS_NAMES[want])
    assert {"TRUNCATED", "CORRUPT"} <= seen
