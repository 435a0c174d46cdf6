"""Table selection of the GPU entropy walks, WITHOUT a GPU.  huff_sync_kernel selects the (DC, AC) table pair of an MCU position from
registers: at most four distinct pairs and a two-bit class per position (TableClasses, csrc/huffman_gpu_core.h), with a short form for
at most two classes.  hipjpegEntropyDecodeGpuAlgorithmHost builds the same classes with the same routine, checks that they reproduce
the per-position array, and runs every walk in the sync kernel's select form and in the tail kernels' branch form (a disagreement is
INTERNAL_ERROR).  The files (helpers/walk_files.py) have one, two, three and four distinct pairs over 1, 3, 4, 6 and 10 positions.

Coefficients must equal the host decoder's and the oracle's.  Pixels: the emulation has no pixel stage, so its coefficients are
written out again as a file with the Annex K tables and that file's planes, decoded by the oracle, must equal the oracle's planes of
the file under test."""
import numpy as np
import pytest

import oracle
from helpers import walk_files as W
from nvimagecodec_amd import lowlevel

FILES = W.class_files()


def test_the_files_are_what_the_issue_asks_for():
    names = {name for name, _, _, _ in FILES}
    assert {"gray_one_pair", "420_two_pairs", "444_pair_changes_every_block", "luma42_ten_positions", "three_pairs", "four_pairs",
            "three_pairs_two_scans"} <= names
    for name, jpeg, _, samp in FILES:
        info = lowlevel.get_image_info(jpeg)
        assert 16 <= info["width"] <= 64 and 16 <= info["height"] <= 64, name
        assert all(bits > 2 * 1024 for bits in W.scan_bits(jpeg)), (name, W.scan_bits(jpeg))   # at least 3 subsequences per stream
    by_name = {name: (jpeg, samp) for name, jpeg, _, samp in FILES}
    assert sum(h * v for h, v in by_name["luma42_ten_positions"][1]) == 10 and sum(h * v for h, v in by_name["420_two_pairs"][1]) == 6
    assert lowlevel.get_image_info(by_name["three_pairs_two_scans"][0])["num_scans"] == 2


@pytest.mark.parametrize("case", FILES, ids=[f[0] for f in FILES])
def test_emulation_equals_host_decoder_and_oracle(case):
    name, jpeg, meant, samp = case
    got, passes = lowlevel.entropy_decode_gpu_algorithm_host(jpeg)   # raises on any status, INTERNAL_ERROR included
    host, _ = lowlevel.entropy_decode_host(jpeg)
    ref, _ = oracle.decode_coefficients(jpeg)
    assert passes >= 1
    for c, (a, b, r) in enumerate(zip(got, host, ref)):
        assert np.array_equal(a, b), (name, "component", c, "differs from the host decoder")
        assert np.array_equal(a, r), (name, "component", c, "differs from the oracle")
    if len(samp) > 1:   # (a one-component file codes its real blocks only: the padding of the grid is not in the file)
        for c, (a, m) in enumerate(zip(got, meant)):
            assert np.array_equal(a, m), (name, "component", c, "differs from what the writer meant")
    # pixels, through the oracle's own IDCT
    info = lowlevel.get_image_info(jpeg)
    again = W.write_scans(info["width"], info["height"], samp, got, [W.LUMA] + [W.CHROMA] * (len(samp) - 1))
    for c, (a, b) in enumerate(zip(oracle.decode_planes(again), oracle.decode_planes(jpeg))):
        assert np.array_equal(a, b), (name, "plane", c)
