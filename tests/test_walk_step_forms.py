"""The select step of the synchronisation walk (csrc/huffman_gpu_core.h select_walk), WITHOUT a GPU: the MCU position kept as a
countdown, the pair entry in the single entry's layout behind the test z + z1 < 64, a long code that zeroes the chosen entry.
hipjpegEntropyDecodeGpuAlgorithmHost runs every walk in that form and in the tail kernels' branch form, which counts the MCU
position upwards, and returns INTERNAL_ERROR where end states (the position recovered from the countdown among them) or block-start
records differ.  The files (helpers/walk_step_files.py) put the step on its edges: every wrap of the countdown (1, 3, 4, 6 and 10
blocks per MCU; two, three and four table classes), first symbols that take z + z1 to 62, 63 and 64, EOB and ZRL as the second
symbol, windows of 5 + 5 and 2 + 8 bits, a pair whose second symbol starts one bit in front of, on and behind a subsequence's end
and a pair that ends the stream, and long codes behind a pair, as a subsequence's and the stream's last symbol, on bits 31 and 0 of a
word, twice in a row and closing a block.

The last test reads the pair table itself through hipjpegTestPairSteps: for every 10-bit window and every zigzag position the step
taken from the table must be the one or two symbols a canonical decoder reads there."""
import ctypes

import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as jc
from helpers import steered_streams as ss
from helpers import walk_files as W
from helpers import walk_step_files as F
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

INTERNAL_ERROR = 10
SAMPLING = F.sampling_files(3 * 1024)
STREAMS = F.small() + F.combined()


def _emulate(jpeg):
    try:
        return lowlevel.entropy_decode_gpu_algorithm_host(jpeg)
    except N.HipJpegError as e:
        assert e.status != INTERNAL_ERROR, "the forms of the walk, or a record and the position walk, disagree"
        raise


def test_the_files_are_what_the_issue_asks_for():
    per_mcu = {name: sum(h * v for h, v in samp) for name, _, _, samp in SAMPLING}
    assert {per_mcu[n] for n in ("gray_1", "444_3", "422_4", "420_6", "h4v2_10")} == {1, 3, 4, 6, 10}
    classes = {name: len({repr(t) for t in F.SAMPLINGS[name][1]}) for name in F.SAMPLINGS}
    assert {classes["420_6"], classes["444_three_classes"], classes["420_three_classes"], classes["four_classes"]} == {2, 3, 4}
    assert all(W.scan_bits(jpeg)[0] > 3 * 1024 for _, jpeg, _, _ in SAMPLING)
    names = {n for n, _ in STREAMS}
    for d in ("-1", "+0", "+1"):
        assert "steered_s_pair_across_" + d in names
    assert {"pair_p_sum_62", "pair_p_sum_63", "pair_p_sum_64", "pair_p_two_and_eight", "pair_p_five_and_five", "long_l_behind_a_pair",
            "long_l_word_phases", "long_l_closes_a_block", "steered_s_pair_ends_stream_ends_stream",
            "long_l_long_code_ends_stream_ends_stream"} <= names
    for name, w in F.combined():   # three sync workgroups and a halo
        assert (w.dbits if isinstance(w, ss.Steered) else w.total_bits) > 3 * F.WG_BITS + 1024, name


@pytest.mark.parametrize("case", SAMPLING, ids=[f[0] for f in SAMPLING])
def test_every_wrap_of_the_countdown(case):
    name, jpeg, meant, samp = case
    got, passes = _emulate(jpeg)
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


@pytest.mark.parametrize("case", STREAMS, ids=[f[0] for f in STREAMS])
def test_placed_symbols(case):
    name, w = case
    got, passes = _emulate(w.jpeg)
    host, _ = lowlevel.entropy_decode_host(w.jpeg)
    ref, _ = oracle.decode_coefficients(w.jpeg)
    assert passes >= 1
    assert np.array_equal(got[0], host[0]), "differs from the host decoder"
    assert np.array_equal(got[0], ref[0]), "differs from the oracle"
    assert np.array_equal(got[0], w.coefficients()), "differs from what the writer meant"


# ---------------------------------------------------------------------------------------------------------------- the pair table
TABLES = {"annex_k_luma": jc.AC_LUMA, "annex_k_chroma": jc.AC_CHROMA, "annex_k_luma_reversed": W.LUMA_REVERSED[1],
          "annex_k_chroma_reversed": W.CHROMA_REVERSED[1], "eleven_bits_and_more": W.LONG_AC, "two_bit_zrl": F.PAIR_AC,
          "steered": (ss.S_BITS, ss.S_VALS)}


def _symbol_at(codes, window, bits):
    """the symbol a canonical decoder reads from the top of `bits` bits of window: (total bits, zigzag advance), or None where the
    code (of at most ten bits), or the code with its value bits, does not lie inside them"""
    for sym, (code, length) in codes.items():
        if length <= min(bits, 10) and (window >> (bits - length)) == code:
            size, run = sym & 15, sym >> 4
            total = length + size
            if total > bits:
                return None
            return total, (run + 1 if size else 16 if run == 15 else 64)
    return None


@pytest.mark.parametrize("name", list(TABLES))
def test_a_step_from_the_pair_table_is_one_or_two_single_steps(name):
    bits, vals = TABLES[name]
    codes = jc._codes(bits, vals)
    steps = (ctypes.c_uint32 * (1024 * 64))()
    vals_a = (ctypes.c_uint8 * len(vals))(*vals)
    bits_a = (ctypes.c_uint8 * 16)(*bits)
    assert N.load().hipjpegTestPairSteps(ctypes.addressof(bits_a), ctypes.addressof(vals_a), len(vals), ctypes.addressof(steps)) == 0
    steps = np.frombuffer(steps, np.uint32).reshape(1024, 64)
    pairs_seen = 0
    for w in range(1024):
        first = _symbol_at(codes, w, 10)
        second = None
        if first and first[1] != 64:
            second = _symbol_at(codes, (w << first[0]) & 1023 if first[0] < 10 else 0, 10) if first[0] < 10 else None
            if second and first[0] + second[0] > 10:
                second = None
        # a code of up to ten bits whose value bits reach past the window is a first-level entry all the same: read it from 31 bits
        wide = _symbol_at(codes, w << 21, 31)
        for z in range(64):
            step = int(steps[w, z])
            total, zadv, two, lng = step & 31, (step >> 8) & 127, (step >> 16) & 1, (step >> 17) & 1
            if wide is None:   # no code of up to ten bits opens this window: a long code, or no code at all
                assert not two and (lng and total == 0 and zadv == 0 or (total, zadv) == (1, 1)), (name, w, z)
                continue
            assert not lng, (name, w, z)
            if two:
                pairs_seen += 1
                assert first and second, (name, w, z, "a pair where the window does not hold two whole symbols")
                assert z >= 1 and z + first[1] < 64, (name, w, z, "the first symbol of a pair must leave the block open")
                assert total == first[0] + second[0], (name, w, z)
                # the state after the pair is the state after the two symbols: the same position, or a completed block either way
                single = z + first[1] + second[1]
                assert (z + zadv >= 64) == (single >= 64) and (single >= 64 or z + zadv == single), (name, w, z)
            else:
                assert (total, zadv) == wide, (name, w, z)
                # and where the table could have paired, it has: every AC position from which the first symbol leaves the block open
                if first and second and z >= 1 and z + first[1] < 64 and first[0] + 2 <= 10:
                    pytest.fail("%s: window %d at z = %d holds two symbols and the step took one" % (name, w, z))
    assert pairs_seen > 0 or name in ("annex_k_luma_reversed", "annex_k_chroma_reversed")
