"""Long codes in the GPU entropy walks, WITHOUT a GPU.  A code longer than the ten bits of the first-level lookup is, in
huff_sync_kernel's walk, a step of its own: the step that meets it consumes nothing and points the next step's ordinary lookup at
the second-level table and the six bits behind the first ten (select_walk, csrc/huffman_gpu_core.h).  The streams
(helpers/walk_files.py: one component, EOB, ZRL, four coefficient symbols and one DC category with codes of 11 to 16 bits) put such
a code where the two halves can come apart: across a subsequence seam and the sync workgroup's seam, first behind a block end, as
the EOB that ends a block exactly on a seam, as the stream's last symbol, twice in a row -- each without and with a restart
interval -- and one damaged stream whose second-level lookup hits an entry no code owns.

hipjpegEntropyDecodeGpuAlgorithmHost runs every walk in the sync kernel's form and in the tail kernels' form and returns
INTERNAL_ERROR where end states or block-start records differ, or where a record disagrees with the position walk.  sync_passes pins
the trajectories from wrong start states: the table below was taken with the build of commit b0fffd0, before the walks had forms."""
import numpy as np
import pytest

from helpers import walk_files as W
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

FILES = W.long_code_files()
INTERNAL_ERROR = 10

# sync_passes of hipjpegEntropyDecodeGpuAlgorithmHost at commit b0fffd0 ("Entropy tail: enter groups with the state in front, not
# pass 0's guess"), the parent of the change that gave the walks their forms
PASSES_AT_B0FFFD0 = {
    "seam_j1_d1": 2, "seam_j1_d9": 2, "seam_j1_d10": 1, "seam_j1_d11": 1, "seam_j1_d15": 1,
    "seam_j255_d1": 2, "seam_j255_d9": 2, "seam_j255_d10": 2, "seam_j255_d11": 2, "seam_j255_d15": 2,
    "behind_block_end": 1, "eob_at_subsequence_end": 1, "long_dc": 2, "long_zrl": 2, "two_in_a_row": 1,
    "last_symbol_on_a_byte": 2, "last_symbol_seven_padding_bits": 1,
    "seam_j1_d1_rst": 1, "seam_j1_d9_rst": 1, "seam_j1_d10_rst": 1, "seam_j1_d11_rst": 2, "seam_j1_d15_rst": 1,
    "seam_j255_d1_rst": 2, "seam_j255_d9_rst": 2, "seam_j255_d10_rst": 2, "seam_j255_d11_rst": 2, "seam_j255_d15_rst": 2,
    "behind_block_end_rst": 1, "eob_at_subsequence_end_rst": 1, "long_dc_rst": 2, "long_zrl_rst": 2, "two_in_a_row_rst": 1,
    "last_symbol_on_a_byte_rst": 2, "last_symbol_seven_padding_bits_rst": 2,
}


def _code_bits(symbol):
    code, length = W.L_AC[symbol]
    return [(code >> (length - 1 - i)) & 1 for i in range(length)]


def test_the_placements_are_where_they_should_be():
    by_name = {name: w for name, w, _ in FILES}
    assert {n for n, _, ok in FILES if ok} == set(PASSES_AT_B0FFFD0)
    for tag in ("", "_rst"):
        for j in (1, W.WG_SEAM):
            for d in W.SEAM_D:
                w = by_name["seam_j%d_d%d%s" % (j, d, tag)]
                assert w.at == 1024 * j - d and w.bits[w.at:w.at + 16] == _code_bits(0x04) and len(_code_bits(0x04)) == 16
        assert by_name["seam_j255_d1" + tag].total_bits > 257 * 1024 - 1024                 # 257 subsequences, two sync workgroups
        assert by_name["last_symbol_on_a_byte" + tag].total_bits % 8 == 0
        assert by_name["last_symbol_seven_padding_bits" + tag].total_bits % 8 == 1
        for name in ("last_symbol_on_a_byte", "last_symbol_seven_padding_bits"):
            w = by_name[name + tag]
            assert w.bits[w.total_bits - 11:w.total_bits] == _code_bits(0x00) and len(_code_bits(0x00)) == 11   # the long EOB
    assert all(len(w.markers) > 0 for name, w, _ in FILES if name.endswith("_rst"))


@pytest.mark.parametrize("case", [f for f in FILES if f[2]], ids=[f[0] for f in FILES if f[2]])
def test_emulation_equals_host_decoder(case):
    name, w, _ = case
    try:
        got, passes = lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)
    except N.HipJpegError as e:
        assert e.status != INTERNAL_ERROR, "the forms of the walk, or a record and the position walk, disagree"
        raise
    host, _ = lowlevel.entropy_decode_host(w.jpeg)
    assert np.array_equal(got[0], host[0])
    assert np.array_equal(got[0], w.coefficients())
    assert passes == PASSES_AT_B0FFFD0[name]


@pytest.mark.parametrize("case", [f for f in FILES if not f[2]], ids=[f[0] for f in FILES if not f[2]])
def test_no_such_code_in_the_second_level_gets_the_host_verdict(case):
    name, w, _ = case
    with pytest.raises(N.HipJpegError) as host:
        lowlevel.entropy_decode_host(w.jpeg)
    with pytest.raises(N.HipJpegError) as emulated:
        lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)
    assert emulated.value.status == host.value.status and host.value.status != INTERNAL_ERROR
