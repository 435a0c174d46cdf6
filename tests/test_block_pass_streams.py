"""The block pass's decode loop (csrc/huffman_gpu_core.h decode_block) on crafted baseline streams, through the host emulation of the
GPU entropy stage.  The files use a small AC Huffman table of their own with short ZRL and EOB codes and one 16-bit code, so that
ZRL runs, blocks that end without EOB, long codes behind short ones and the end of the stream can be put exactly where wanted.
Good streams are compared with the oracle; damaged ones must get the status the host entropy decoder gives them (include/hipjpeg.h:
CORRUPT for a coefficient index past 63, TRUNCATED for data that ends early).  No GPU needed."""
import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as jc
from helpers.steered_streams import EOB, ZRL, c, gray_file, scan_bits
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

TRUNCATED, CORRUPT = 4, 5  # hipjpegStatus_t


def expected(blocks):
    """Coefficients [1, n, 64] in natural order of a legal token list."""
    out = np.zeros((1, len(blocks), 64), np.int16)
    pred = 0
    for b, (diff, tokens) in enumerate(blocks):
        pred += diff
        out[0, b, 0] = pred
        z = 1
        for tok in tokens:
            if tok == EOB:
                break
            if tok == ZRL:
                z += 16
                continue
            z += tok[1]
            out[0, b, jc.ZIGZAG[z]] = tok[2]
            z += 1
    return out


def check_good(blocks):
    jpeg = gray_file(blocks)
    coefs, _ = lowlevel.entropy_decode_gpu_algorithm_host(jpeg)
    ref, _ = oracle.decode_coefficients(jpeg)
    assert oracle.decode(jpeg, oracle.FMT_GRAY).shape == (8, 8 * len(blocks))
    want = expected(blocks)
    assert np.array_equal(ref[0], want), "the test's own idea of the stream"
    assert np.array_equal(coefs[0], want)


def verdicts(jpeg):
    def run(fn):
        try:
            return 0, fn(jpeg)[0]
        except N.HipJpegError as e:
            return e.status, None
    return run(lowlevel.entropy_decode_gpu_algorithm_host), run(lowlevel.entropy_decode_host)


NEXT = (-3, [c(0, 2), c(0, -1), EOB])  # a block behind the one under test: its DC code must not be taken for an AC symbol


def test_eob_behind_short_symbols():
    check_good([(5, [c(0, 1), EOB]), NEXT])
    check_good([(0, [c(0, -1), c(0, 1), c(0, -2), EOB]), NEXT])
    check_good([(0, [EOB]), (1, [EOB]), NEXT])


def test_zrl_runs():
    check_good([(2, [ZRL, c(0, 1), EOB]), NEXT])
    check_good([(2, [c(0, -1), ZRL, c(0, 3), EOB]), NEXT])
    check_good([(2, [ZRL, ZRL, c(0, 1), ZRL, c(1, -1), EOB]), NEXT])
    check_good([(2, [ZRL, ZRL, ZRL, c(0, 1), c(2, 1), EOB]), NEXT])    # three ZRL: position 49, then 52
    check_good([(2, [ZRL, ZRL, ZRL, c(1, 1), c(0, 1)] + [c(0, -1)] * 12), NEXT])  # ... and on to position 63 without EOB


@pytest.mark.parametrize("lead", [[], [c(1, 1)], [c(0, 7)], [c(2, -1), c(0, 1)]], ids=["even", "run1", "3bits", "run2"])
def test_all_coefficients_present_no_eob(lead):
    """The block ends with the coefficient at position 63, no EOB: the next block's DC code is not taken for an AC symbol."""
    used = sum(t[1] + 1 for t in lead)
    body = [c(0, 1 if i % 3 else -1) for i in range(63 - used)]
    check_good([(1, lead + body), NEXT, (7, lead + body), NEXT])


@pytest.mark.parametrize("lead", [[], [c(1, 1)]], ids=["plain", "run1"])
def test_coefficient_past_position_63_is_reported(lead):
    """Positions 1..62 filled, then a (1,1) symbol: its coefficient would land at 64 -- CORRUPT, from the GPU algorithm and from
    the host decoder."""
    used = sum(t[1] + 1 for t in lead)
    tokens = lead + [c(0, 1)] * (62 - used) + [c(1, 1)]
    (sg, _), (sh, _) = verdicts(gray_file([(1, tokens), NEXT]))
    assert (sg, sh) == (CORRUPT, CORRUPT)


def test_sixteen_bit_code_behind_a_short_one():
    check_good([(1, [c(0, 1), c(0, 9), c(0, -1), c(0, -15), EOB]), NEXT])
    check_good([(1, [ZRL, c(0, 8), c(0, 1), EOB]), NEXT])


def test_last_symbols_at_the_end_of_the_stream():
    """The last block's last symbols end within a few bits of the end of the data (total_bits): every alignment of the end."""
    for n in range(1, 12):
        check_good([(0, [c(0, 1)] * n + [EOB])])
        check_good([(0, [c(0, 1)] * n + [c(0, 2), EOB])])
    check_good([(0, [c(0, 1)] * 63)])


TRUNCATION_BLOCKS = [(3, [c(0, 1), c(0, -1), c(0, 2), ZRL, c(0, 1), c(0, 1), EOB]), (1, [c(0, 1)] * 63), (-2, [c(0, 3), c(0, 1), EOB]),
                     (0, [c(0, 1), c(0, 1), c(0, 1), c(0, 1), EOB])]


def test_truncated_streams_get_the_host_verdict():
    """Cut the scan after every byte: a stream that ends inside a block, or before the last block, is TRUNCATED for the GPU
    algorithm and for the host entropy decoder; only the whole scan decodes, and to equal coefficients."""
    blocks = TRUNCATION_BLOCKS
    scan = scan_bits(blocks)
    rejected = 0
    for keep in range(1, len(scan) + 1):
        jpeg = gray_file(blocks, scan[:keep])
        (sg, cg), (sh, ch) = verdicts(jpeg)
        want = 0 if keep == len(scan) else TRUNCATED
        assert (sg, sh) == (want, want), (keep, sg, sh)
        if sg == 0:
            assert np.array_equal(cg[0], ch[0][: cg[0].shape[0]]) and np.array_equal(cg[0], expected(blocks))
        rejected += sg != 0
    assert rejected == len(scan) - 1
