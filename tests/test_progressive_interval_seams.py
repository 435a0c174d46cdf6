"""Crafted progressive scans WITH restart intervals on the seams of the interval kernels (csrc/progressive_intervals.hip, lane code in
csrc/progressive_interval_core.h), without a GPU: each file of tests/helpers/progressive_interval_seams.py is first shown to BE where it
claims to be -- its condition is a predicate over the writer's own log of interval starts, padding and bit positions, asserted here --, then
pinned: the oracle and the host entropy decoder give back the coefficients the file was written from, and the host twin of the kernels
(hipjpegEntropyDecodeGpuIntervalAlgorithmHost: prog_interval_ac / prog_interval_dc and the replay, the very code the lanes run) gives the
oracle's arrays.  Files over a limit of the GPU path are UNSUPPORTED there; the refusal files -- legal for a sequential decoder, which forgets
an open run at a marker and skips what is left in front of it -- are rejected by the twin's own checks and never answered with coefficients.
tests/test_gpu_progressive_interval_seams.py runs the same files through the kernels.  Nothing here needs Pillow."""
import numpy as np
import pytest

import oracle
from helpers import progressive_interval_seams as I
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

OVER_THE_LIMIT = ["limit_10_second_level_tables", "limit_16_ac_scans", "limit_25_scans", "limit_7_stages"]
UNSUPPORTED, CORRUPT = 3, 5


def test_the_list_of_cases():
    assert I.names("over_limit") == OVER_THE_LIMIT
    assert len(I.names("refusal")) == 7 and all(n.startswith("refuse_") for n in I.names("refusal"))
    assert len(I.CASES) == 60 and all(I.CASES[n]()[0].name == n for n in I.CASES)
    for n in I.TABLE_CASES:
        assert I.CASES[n]()[0].kind == "good"


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_the_file_sits_on_its_seam(name):
    """The case's condition holds, and the log it is read from accounts for every bit of every scan: in every interval the events lie end
    to end from the interval's start, the bits left up to the next start are the padding the log states and are ones, starts are whole
    bytes, and in the file RSTn, counted modulo 8, stands in front of every interval but the first."""
    assert I.holds(name)
    c = I.get(name)
    assert max(a.shape[0] * a.shape[1] for a in c.coefs) <= 640
    bits = int.from_bytes(b"".join(s.data for s in c.log) or b"\0", "big")
    total, at = sum(len(s.data) for s in c.log) * 8, 0
    for s in c.log:
        bounds = list(s.starts) + [len(s.data) * 8]
        assert len(s.pads) == len(s.starts) == len(s.raw_starts) and s.starts[0] == 0 and all(p % 8 == 0 for p in bounds)
        assert all(a < b for a, b in zip(bounds, bounds[1:])), s.entry
        evs = sorted((ev for ev in s.events if ev.kind != "block"), key=lambda ev: ev.pos)
        k = 0
        for i, pad in enumerate(s.pads):
            pos = bounds[i]
            while k < len(evs) and evs[k].pos < bounds[i + 1]:
                assert evs[k].pos == pos and evs[k].nbits > 0, (s.entry, i, evs[k])
                pos += evs[k].nbits
                k += 1
            assert pos + pad == bounds[i + 1] and 0 <= pad < 16, (s.entry, i)
            assert (c.kind == "refusal") or pad < 8
            ones = (bits >> (total - at - bounds[i + 1])) & ((1 << pad) - 1)
            assert ones == (1 << pad) - 1, (s.entry, i)
            if i:
                assert c.jpeg[s.raw_starts[i] - 2: s.raw_starts[i]] == bytes([0xFF, 0xD0 + (i - 1) % 8]), (s.entry, i)
        assert k == len(evs) and s.bits == bounds[-1] - s.pads[-1]
        assert all(0 <= ev.pos <= s.bits for ev in s.events if ev.kind == "block")
        at += len(s.data) * 8
    assert c.jpeg.count(b"\xff\xda") == len(c.log)
    assert lowlevel.get_image_info(c.jpeg)["sof_marker"] == 0xC2


def _coefficients_are_the_chosen_ones(c, got, who):
    assert len(got) == len(c.coefs)
    for k in range(len(c.coefs)):
        rows, cols = I.real_blocks(c, k)
        want = np.asarray(c.coefs[k])[:rows, :cols].astype(np.int16)
        assert np.array_equal(np.asarray(got[k])[:rows, :cols], want), (who, k)


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_every_decoder_gives_back_the_chosen_coefficients(name):
    """The oracle and the host entropy decoder pin the writer (a refusal file too: both decode it like any sequential decoder, and they
    must agree before the case is used); then the twin of the kernels."""
    c = I.get(name)
    got, _ = oracle.decode_coefficients(c.jpeg)
    host, _ = lowlevel.entropy_decode_host(c.jpeg)
    _coefficients_are_the_chosen_ones(c, got, "oracle")
    _coefficients_are_the_chosen_ones(c, host, "host decoder")
    for a, b in zip(got, host):
        assert np.array_equal(a, b)
    with pytest.raises(N.HipJpegError) as err:  # the walk's entry point refuses every file with restart intervals
        lowlevel.entropy_decode_gpu_algorithm_host(c.jpeg)
    assert err.value.status == UNSUPPORTED
    if c.kind == "good":
        emu = lowlevel.entropy_decode_gpu_interval_algorithm_host(c.jpeg)
        _coefficients_are_the_chosen_ones(c, emu, "interval algorithm on the host")
        assert len(emu) == len(got)
        for k in range(len(got)):
            assert np.array_equal(emu[k], got[k]), ("blocks of the MCU padding", k)
    else:
        with pytest.raises(N.HipJpegError) as err:
            lowlevel.entropy_decode_gpu_interval_algorithm_host(c.jpeg)
        assert err.value.status == (UNSUPPORTED if c.kind == "over_limit" else CORRUPT), c.kind


def test_the_refusals_are_the_constructs_and_nothing_else():
    """Each refusal file without its construct -- the run written with its own length, no byte of ones behind the padding -- is a file the
    twin decodes: the lane refused for that construct alone."""
    for name in I.names("refusal"):
        c = I.get(name)
        script = [tuple(s.entry) + ({"interval": s.interval},) for s in c.log]
        jpeg, log = I.write_seams(c.width, c.height, c.sampling, c.coefs, I.S._qt(1), script)
        assert jpeg != c.jpeg and all(p < 8 for s in log for p in s.pads)
        emu = lowlevel.entropy_decode_gpu_interval_algorithm_host(jpeg)
        _coefficients_are_the_chosen_ones(c, emu, name)


def test_the_writer_agrees_with_the_helper_it_builds_on():
    """With nothing but intervals write_seams() is write_progressive_restart(), bit for bit, but for DRI segments that repeat the interval
    in force (the helper writes one in front of every scan)."""
    from helpers import progressive_restart_files as P
    for name in ("bands_cut_anywhere", "three_bit_planes", "dc_recut_per_component"):
        samp, w, h, script, intervals, max_run, dense = P.HELPER_CASES[name]
        theirs, coefs = P.helper_file(name)
        qt = [np.full(64, 3 + c, dtype=np.int32) for c in range(len(samp))]
        ours, log = I.write_seams(w, h, samp, coefs, qt, I.iv(script, intervals), max_run)
        prev, expected, at = 0, bytearray(), 0
        for n in intervals:  # drop the helper's DRI segments that change nothing
            j = theirs.index(b"\xff\xdd\x00\x04", at)
            expected += theirs[at:j] + (theirs[j:j + 6] if n != prev else b"")
            at, prev = j + 6, n
        expected += theirs[at:]
        assert ours == bytes(expected), name
        assert any(len(s.starts) > 1 for s in log)
