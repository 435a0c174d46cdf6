"""Test helper: progressive (SOF2) files whose scans all have restart intervals, written by write_seams() of progressive_seams.py (option
"interval") from CHOSEN coefficients, each on a seam of the interval kernels (csrc/progressive_intervals.hip, lane code in
csrc/progressive_interval_core.h: a lane per restart interval, ProgIntervalBits / ProgBits per lane, 256 intervals per workgroup, table
slots in LDS) or of the destuff kernels in front of them.  As in progressive_seams.py a case states what it is for as a predicate over the
writer's log -- interval starts and event positions in bits of the destuffed stream with the markers dropped and the padding kept, which
is what the planner uploads from ScanHeader::rst_after; padding bits per interval; raw file offsets for the stuffing cases.
Case.kind: "good" (the kernels decode it), "over_limit" (not eligible: host entropy stage, not counted in interval_images) and "refusal"
(eligible, but a lane returns false by its own checks and the host decoder takes the image: interval_takeovers).

Construct                                                          case
reader  interval starts at every byte of a word, four scan kinds   starts_at_every_byte_of_a_word (interval 0 starts at 0 in every file)
        take(popc) of 31 / 32 / 62 / 63 for a block inside a run   take_31_32_62_63_for_blocks_inside_a_run
        end of band in front of 63 correction bits                 take_72_eob9_in_front_of_63_correction_bits (*), refuse_eob14_take_77_run_outlasts_the_interval
        70 and 78 bits behind one refinement symbol                take_70_refine_symbol_and_62_correction_bits, take_78_16bit_code_and_61_correction_bits
        31 / 32 / 62 correction bits between k and the target      take_31_32_62_between_k_and_the_target
        padding of 0 and of 7 bits, last interval included         pad_{0,7}_bits_{dc_first,ac_first,ac_refine}, pad_0_and_7_bits_dc_refine
        last symbol a 10-bit code, stream ends at / behind a word  last_symbol_long_code_stream_ends_{on_a_word_end,one_byte_past_a_word_end}
        a run of sixteen closes a refined block                    zrl_closes_the_last_block_of_an_interval_and_stands_in_front_of_a_run
stuffing FF 00 FF Dn                                               ff00_in_front_of_every_marker
        FF 00 first in an interval                                 ff00_first_in_every_interval
        DC refinement intervals that are FF 00, >= 17 bytes dropped  dc_refinement_intervals_of_ff00_17_bytes_dropped
        starts in the first / last 16 bytes of a 16,384-byte chunk starts_in_the_first_and_last_16_bytes_of_a_destuff_chunk
work    1, 255, 256, 257, 513 intervals, AC chain and DC scans     count_{1,255,256,257,513}_gray
        ... of component 2 of 4:4:4, component 3 of four           count_{255,256,257,513}_component_2_of_444, ..._component_3_of_four
        last interval of one block / interval above the count      last_interval_of_one_block, count_1_gray
        interval 65535                                             interval_65535, take_72_...
        AC interval 1 for luma, 65535 for chroma                   ac_interval_1_for_luma_65535_for_chroma
        DC scans cut differently from the AC scans and each other  dc_intervals_differ_from_ac_and_from_each_other
        interleaved DC scans over a padded MCU grid                interleaved_dc_{420,422,440,411} (**)
tables  nine second-level tables / two-symbol tables last in the pool / six stages with six tables
                                                                   table_of_nine_second_level_tables, two_symbol_tables_last_in_the_pool,
                                                                   six_ac_stages_each_with_a_table_of_its_own
        four DC tables in one scan                                 dc_four_components_four_tables
        the limits                                                 limit_{6,7}_stages, limit_{15,16}_ac_scans, limit_{24,25}_scans,
                                                                   limit_{9,10}_second_level_tables
refusal a run still open at an interval's end                      refuse_run_open_at_interval_end_{first,refine}, refuse_eob14_...
        a whole byte of ones behind the padding                    refuse_byte_of_ones_behind_the_pad_{ac_first,ac_refine,dc_first,dc_refine}
(*)  An EOB14 the kernels ACCEPT cannot be written: its run covers 16,384 blocks or more, a lane refuses a run that outlasts its interval, and
     a case has at most 640 blocks.  The longest acceptable one here is EOB9 (9 + 63 = 72 bits in one take); the EOB14 itself (14 + 63 = 77)
     is read by the refusal case before the lane finds the run still open.
(**) A padding row needs a vertical factor of 2 (4:2:0, 4:4:0), a padding column a horizontal factor above 1 (4:2:0, 4:2:2, 4:1:1): each
     layout starts an interval in the padding it can have.  The pixel stage takes all of these layouts in interleaved RGB: no case needs planes."""
import collections
import functools

import numpy as np

from helpers import progressive_seams as S
from helpers.jpeg_from_coefficients import random_coefficients
from helpers.progressive_restart_files import AC_PROG
from helpers.progressive_seams import CMYK, GRAY, S420, S444, blank, ends, find, first_filler, second_level_tables, setk, table_from_lengths, write_seams

S422, S440, S411 = [(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(4, 1), (1, 1), (1, 1)]
CHUNK = 16384  # kDestuffChunk: raw bytes of a scan one workgroup of the destuff kernels handles
Case = collections.namedtuple("Case", "name jpeg coefs log sampling width height kind")
CASES = {}  # name -> function() -> (Case, predicate) (cached)


def case(name, kind="good", tries=(None,)):
    """fn() or, with tries, fn(shift) -> (width, height, sampling, coefs, script, check): the first shift whose file meets check(jpeg, log)"""
    def deco(fn):
        @functools.lru_cache(maxsize=None)
        def make():
            for shift in tries:
                width, height, sampling, coefs, script, check = fn() if shift is None else fn(shift)
                jpeg, log = write_seams(width, height, sampling, coefs, S._qt(len(sampling)), script)
                if check(jpeg, log):
                    return Case(name, jpeg, coefs, log, sampling, width, height, kind), check
            raise AssertionError("no filler puts %s on its seam" % name)
        assert name not in CASES
        CASES[name] = make
        return make
    return deco


def iv(script, intervals):
    """the script with a restart interval for every scan (one number for all, or one per scan)"""
    ns = intervals if isinstance(intervals, (list, tuple)) else [intervals] * len(script)
    assert len(ns) == len(script)
    res = []
    for e, n in zip(script, ns):
        opt = dict(e[-1]) if isinstance(e[-1], dict) else {}
        opt["interval"] = n
        res.append(tuple(e[:-1] if isinstance(e[-1], dict) else e) + (opt,))
    return res


FOUR = [("dc", [0], 0, 1), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0), ("dc", [0], 1, 0)]  # the four scan kinds
KINDS = {"dc_first": 0, "ac_first": 1, "ac_refine": 2, "dc_refine": 3}  # -> index into FOUR
REFINE3 = [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0)]


def rand(seed, width, height, sampling=GRAY, dense=6):
    return random_coefficients(np.random.default_rng(seed), width, height, sampling, 5, dense=dense, small=3, dc=60)


def history(a, b, places, bit=None):
    """coefficients of magnitude 2 or 3 (non-zero history for a refinement scan with ah = 1; bit: the correction bit of all of them)"""
    for k in places:
        setk(a, b, k, (2 + ((b + k) % 2 if bit is None else bit)) * (1 if k % 3 else -1))


# ------------------------------------------------------------------------------------------------------------------- the reader
@case("starts_at_every_byte_of_a_word", tries=range(60))
def _starts(seed):
    a = rand(seed, 64, 24)

    def check(jpeg, log):
        return all(len(s.starts) == 12 and {p % 32 for p in s.starts[1:]} == {0, 8, 16, 24} for s in log)
    return 64, 24, GRAY, a, iv(FOUR, 2), check


@case("take_31_32_62_63_for_blocks_inside_a_run")
def _take_in_run():
    """both intervals: a block with a new coefficient opens a run of five; the four blocks inside it have 31, 32, 62 and 63 coefficients
    in their history, a correction bit each"""
    a = blank(80, 8)
    for i in (0, 1):
        setk(a[0], 5 * i, 1 + i, 1)
        for j, n in enumerate((31, 32, 62, 63)):
            history(a[0], 5 * i + 1 + j, range(64 - n, 64) if i else range(1, n + 1))

    def check(jpeg, log):
        s = log[2]
        for i in (0, 1):
            run = find(s, "eob", 5 * i)
            if len(run) != 1 or run[0].arg != 5 or not s.starts[i] <= run[0].pos < (s.starts + (s.bits,))[i + 1]:
                return False
            for j, n in enumerate((31, 32, 62, 63)):
                b = 5 * i + 1 + j
                if [ev.arg for ev in find(s, "block", b)] != [True] or [ev.nbits for ev in find(s, "corr", b)] != [n]:
                    return False
        return len(s.starts) == 2
    return 80, 8, GRAY, a, iv(REFINE3, 5), check


@case("take_72_eob9_in_front_of_63_correction_bits")
def _take_72():
    """one interval (65535) of 520 blocks, one run over all of them: EOB9, its nine extra bits and the first block's 63 correction bits"""
    a = blank(8 * 65, 64)
    history(a[0], 0, range(1, 64))

    def check(jpeg, log):
        s = log[2]
        run = find(s, "eob")
        corr = find(s, "corr", 0)
        return len(run) == 1 and run[0].arg == 520 and run[0].nbits == 7 + 9 and len(corr) == 1 and corr[0].pos == ends(run[0]) and corr[0].nbits == 63 and \
            all(len(x.starts) == 1 for x in log) and jpeg.count(b"\xff\xdd\x00\x04\xff\xff") == 1
    return 8 * 65, 64, GRAY, a, iv(REFINE3, 65535), check


@case("take_31_32_62_between_k_and_the_target")
def _take_between():
    a = blank(48, 8)
    for i in (0, 1):
        for j, n in enumerate((31, 32, 62)):
            history(a[0], 3 * i + j, range(1, n + 1))
            setk(a[0], 3 * i + j, n + 1, -1 if i else 1)

    def check(jpeg, log):
        s = log[2]
        for i in (0, 1):
            for j, n in enumerate((31, 32, 62)):
                new = find(s, "coef", 3 * i + j)
                if len(new) != 1 or new[0].arg != n + 1 or not any(c.pos == ends(new[0]) and c.nbits == n for c in find(s, "corr", 3 * i + j)):
                    return False
        return len(s.starts) == 2
    return 48, 8, GRAY, a, iv(REFINE3, 3), check


def _long_symbol(name, places, new, table, nbits):
    @case(name)
    def fn():
        """interval 1 (blocks 2 and 3): block 2 holds the long symbol"""
        a = blank(32, 8)
        setk(a[0], 0, 2, 1)
        history(a[0], 2, places)
        setk(a[0], 2, new, -1)
        setk(a[0], 3, 2, 1)
        script = iv(REFINE3, 2)
        if table:
            script[2][-1]["ac"] = {0: table}

        def check(jpeg, log):
            s = log[2]
            ev = find(s, "coef", 2)
            corr = [c for c in find(s, "corr", 2) if ev and c.pos == ends(ev[0])]
            return len(ev) == 1 and len(corr) == 1 and ev[0].nbits + corr[0].nbits == nbits and corr[0].nbits == len(places) and ev[0].pos >= s.starts[1] > 0
        return 32, 8, GRAY, a, script, check


_long_symbol("take_70_refine_symbol_and_62_correction_bits", range(1, 63), 63, None, 70)
_long_symbol("take_78_16bit_code_and_61_correction_bits", range(1, 62), 62, S.AC_LONG_NEW, 78)

for _kind in ("dc_first", "ac_first", "ac_refine"):
    for _pad in (0, 7):
        def _pad_case(seed, kind=_kind, pad=_pad):
            a = rand(seed, 64, 24)

            def check(jpeg, log):
                s = log[KINDS[kind]]
                return len(s.pads) == 6 and pad in s.pads[:-1] and s.pads[-1] == pad
            return 64, 24, GRAY, a, iv(FOUR, 4), check
        case("pad_%d_bits_%s" % (_pad, _kind), tries=range(400))(_pad_case)


@case("pad_0_and_7_bits_dc_refine")
def _pad_dc_refine():
    a = rand(3, 64, 24)
    script = iv([("dc", [0], 0, 2), ("ac", 0, 1, 63), ("dc", [0], 2, 1), ("dc", [0], 1, 0)], [8, 8, 8, 1])
    return 64, 24, GRAY, a, script, lambda jpeg, log: log[2].pads == (0, 0, 0) and log[3].pads == (7,) * 24


AC_LATE_EOB = table_from_lengths({0x01: 2, 0x02: 2, 0x03: 3, 0x04: 4, 0x05: 5, 0x11: 6, 0xF0: 7, 0x00: 10, 0x10: 11})
for _name, _rem in (("on_a_word_end", 0), ("one_byte_past_a_word_end", 1)):
    def _late(shift, rem=_rem):
        """the last interval's last block ends with an end of band whose code has 10 bits: the second-level lookup, with the reader's
        look-ahead words behind the stream"""
        a = blank(48, 8)
        setk(a[0], 1, 1, 2)
        first_filler(a[0], 3, shift)
        setk(a[0], 4, 1, -3)
        setk(a[0], 5, 1, 1)

        def check(jpeg, log):
            s = log[1]
            last = max(S.symbols(s), key=lambda ev: ev.pos)
            return last.kind == "eob" and last.block == 5 and last.nbits == 10 and ends(last) == s.bits and len(s.starts) == 2 and \
                len(s.data) % 4 == rem and len(s.data) >= 8 and second_level_tables(AC_LATE_EOB) >= 1
        return 48, 8, GRAY, a, iv([("dc", [0]), ("ac", 0, 1, 63, 0, 0, {"ac": {0: AC_LATE_EOB}})], 3), check
    case("last_symbol_long_code_stream_ends_" + _name, tries=range(65))(_late)


@case("zrl_closes_the_last_block_of_an_interval_and_stands_in_front_of_a_run")
def _zrl():
    """blocks 3 and 4: a new coefficient at place 5, 50 history coefficients behind it, 8 zero-history places left -- a run of sixteen closes
    the block (t > se, s == 0).  Block 3 is the last of interval 0; behind block 4 block 5 opens a run that block 6 lies in"""
    a = blank(64, 8)
    setk(a[0], 0, 9, 1)
    for b in (3, 4):
        setk(a[0], b, 5, 1)
        history(a[0], b, range(6, 56))
    setk(a[0], 5, 2, -1)
    history(a[0], 6, range(1, 40))
    setk(a[0], 7, 63, 1)

    def check(jpeg, log):
        s = log[2]
        z3, z4 = find(s, "zrl", 3), find(s, "zrl", 4)
        if len(z3) != 1 or len(z4) != 1 or z3[0].arg != 8 or z4[0].arg != 8 or len(s.starts) != 2:
            return False
        last0 = max((ev for ev in S.symbols(s) if ev.pos < s.starts[1]), key=lambda ev: ev.pos)
        return last0 == z3[0] and len(find(s, "eob", 5, arg=2)) == 1 and [ev.arg for ev in find(s, "block", 6)] == [True] and \
            [c.nbits for c in find(s, "corr", 6)] == [39] and z4[0].pos > s.starts[1]
    return 64, 8, GRAY, a, iv([REFINE3[0], REFINE3[1], REFINE3[2] + ({"zrl_close": {3, 4}},)], 4), check


# ------------------------------------------------------------------------------------------------------------------- stuffing and markers
def _marker(i):
    return bytes([0xFF, 0xD0 + i % 8])


@case("ff00_in_front_of_every_marker")
def _ff_before():
    """AC refinement, one block per interval: an end of band and 63 correction bits of ones -- the interval's last byte is FF"""
    a = blank(32, 8)
    for b in range(4):
        history(a[0], b, range(1, 64), bit=1)

    def check(jpeg, log):
        s = log[2]
        return len(s.starts) == 4 and all(jpeg[s.raw_starts[i + 1] - 4: s.raw_starts[i + 1]] == b"\xff\x00" + _marker(i) for i in range(3))
    return 32, 8, GRAY, a, iv(REFINE3, 1), check


AC_FF = table_from_lengths({0x00: 1, 0x01: 2, 0x02: 3, 0x03: 4, 0x04: 5, 0x05: 6, 0x11: 7, 0xF0: 8, 0x21: 9})


@case("ff00_first_in_every_interval")
def _ff_first():
    """AC first scan, one block per interval, its first symbol a 9-bit code of eight ones and a zero (second-level lookup at the start)"""
    a = blank(32, 8)
    for b in range(4):
        setk(a[0], b, 3, 1 if b % 2 else -1)
        setk(a[0], b, 4, 2 + b % 2)

    def check(jpeg, log):
        s = log[1]
        return len(s.starts) == 4 and all(jpeg[r: r + 2] == b"\xff\x00" for r in s.raw_starts) and \
            all(jpeg[s.raw_starts[i + 1] - 2: s.raw_starts[i + 1]] == _marker(i) for i in range(3))
    return 32, 8, GRAY, a, iv([("dc", [0]), ("ac", 0, 1, 63, 0, 0, {"ac": {0: AC_FF}})], 1), check


def dropped(s, i):
    """stuffed bytes the destuff kernels have dropped in front of interval i of a scan"""
    return s.raw_starts[i] - s.raw_starts[0] - s.starts[i] // 8 - 2 * i


@case("dc_refinement_intervals_of_ff00_17_bytes_dropped")
def _dc_ones():
    a = blank(128, 128)
    a[0][..., 0] = 1
    setk(a[0], 7, 5, 2)

    def check(jpeg, log):
        s = log[2]
        raw = jpeg[s.raw_starts[0]: s.raw_starts[0] + 4 * 32 - 2]
        return s.data == b"\xff" * 32 and raw == b"".join(b"\xff\x00" + _marker(i) for i in range(32))[:-2] and len(s.starts) == 32 and \
            [dropped(s, i) for i in range(32)] == list(range(32))
    return 128, 128, GRAY, a, iv([("dc", [0], 0, 1), ("ac", 0, 1, 63), ("dc", [0], 1, 0)], [8, 65535, 8]), check


@case("starts_in_the_first_and_last_16_bytes_of_a_destuff_chunk", tries=range(40))
def _chunk_pieces(seed):
    """640 dense blocks, an interval each: the AC scan comes to 37,807 bytes in the file (36,477 destuffed), three chunks of the destuff
    kernels; interval starts lie 16,370 and 32,779 bytes behind the scan's first byte"""
    rng = np.random.default_rng(seed)
    a = S._dense(rng, 80, 8, 40, 30)

    def check(jpeg, log):
        s = log[1]
        offs = [r - s.raw_starts[0] for r in s.raw_starts[1:]]
        return offs[-1] > 2 * CHUNK and any(o >= CHUNK and o % CHUNK < 16 for o in offs) and any(o % CHUNK >= CHUNK - 16 for o in offs) and len(s.starts) == 640
    return 640, 64, GRAY, a, iv(S._FIRST, 1), check


# ------------------------------------------------------------------------------------------------------------------- division of work
for _count, (_bw, _bh, _n) in {1: (5, 5, 26), 255: (15, 17, 1), 256: (16, 16, 1), 257: (257, 1, 1), 513: (27, 19, 1)}.items():
    def _count_gray(count=_count, bw=_bw, bh=_bh, n=_n):
        a = rand(count, 8 * bw, 8 * bh, dense=2)
        return 8 * bw, 8 * bh, GRAY, a, iv(FOUR, n), lambda jpeg, log: all(len(s.starts) == count for s in log) and \
            (jpeg.count(b"\xff\xd0") > 0) == (count > 1)
    case("count_%d_gray" % _count)(_count_gray)

for _what, _samp, _comp in (("component_2_of_444", S444, 2), ("component_3_of_four", CMYK, 3)):
    for _count, (_bw, _bh) in {255: (15, 17), 256: (16, 16), 257: (257, 1), 513: (27, 19)}.items():
        def _count_comp(count=_count, bw=_bw, bh=_bh, samp=_samp, comp=_comp):
            """the component's AC chain and its own DC scans have `count` intervals (the unit word (component << 28) | first with first = 0,
            256, 512), every other scan one"""
            a = rand(count + comp, 8 * bw, 8 * bh, samp, dense=2)
            for c in range(comp):
                a[c][..., 1:] = 0
                setk(a[c], c, 3, 2)
            rest = list(range(comp))
            script = [("dc", rest, 0, 0, {"td": [0] + [1] * (comp - 1)}), ("dc", [comp], 0, 1)] + [("ac", c, 1, 63) for c in rest] + \
                [("ac", comp, 1, 63, 0, 1), ("ac", comp, 1, 63, 1, 0), ("dc", [comp], 1, 0)]
            ns = [65535, 1] + [65535] * comp + [1, 1, 1]

            def check(jpeg, log):
                return [len(s.starts) for s in log] == [1, count] + [1] * comp + [count] * 3 and log[-2].entry[1] == comp
            return 8 * bw, 8 * bh, samp, a, iv(script, ns), check
        case("count_%d_%s" % (_count, _what))(_count_comp)


@case("last_interval_of_one_block")
def _last_one():
    return 40, 40, GRAY, rand(25, 40, 40), iv(FOUR, 4), lambda jpeg, log: 25 % 4 == 1 and all(len(s.starts) == 7 for s in log)


@case("interval_65535")
def _big():
    return 40, 40, GRAY, rand(26, 40, 40), iv(FOUR, 65535), lambda jpeg, log: all(len(s.starts) == 1 for s in log) and b"\xff\xdd\x00\x04\xff\xff" in jpeg


_AC444 = [("ac", c, 1, 63, 0, 1) for c in range(3)] + [("ac", c, 1, 63, 1, 0) for c in range(3)]


@case("ac_interval_1_for_luma_65535_for_chroma")
def _per_component():
    script = iv([("dc", [0, 1, 2])] + _AC444, [5, 1, 65535, 65535, 1, 65535, 65535])
    return 48, 32, S444, rand(31, 48, 32, S444), script, lambda jpeg, log: [len(s.starts) for s in log] == [5, 24, 1, 1, 24, 1, 1]


@case("dc_intervals_differ_from_ac_and_from_each_other")
def _dc_recut():
    script = iv([("dc", [0, 1, 2], 0, 1)] + _AC444 + [("dc", [0], 1, 0), ("dc", [1], 1, 0), ("dc", [2], 1, 0)], [5, 4, 3, 7, 4, 3, 7, 3, 6, 1])
    return 48, 32, S444, rand(32, 48, 32, S444), script, lambda jpeg, log: [len(s.starts) for s in log] == [5, 6, 8, 4, 6, 8, 4, 8, 4, 24]


for _name, _samp, _n in (("420", S420, 2), ("422", S422, 2), ("440", S440, 2), ("411", S411, 3)):
    def _interleaved(samp=_samp, n=_n):
        """40 x 24 samples: five real luma block columns and three rows under an MCU grid that is larger; interleaved DC scans, first and
        refinement, with an interval that starts in the last MCU column and in the last MCU row"""
        a = rand(n + samp[0][0], 40, 24, samp)
        h, v = samp[0]
        mx, my = -(-40 // (8 * h)), -(-24 // (8 * v))
        script = iv([("dc", [0, 1, 2], 0, 1)] + [("ac", c, 1, 63) for c in range(3)] + [("dc", [0, 1, 2], 1, 0)], [n, 3, 2, 2, n])

        def check(jpeg, log):
            first = [(i * n // mx, i * n % mx) for i in range(-(-mx * my // n))]
            pad_col, pad_row = mx * h > 5, my * v > 3
            return all(len(log[s].starts) == len(first) and len(log[s].events) == mx * my * (h * v + 2) for s in (0, 4)) and (pad_col or pad_row) and \
                (not pad_col or any(x == mx - 1 for _, x in first[1:])) and (not pad_row or any(y == my - 1 for y, _ in first[1:]))
        return 40, 24, samp, a, script, check
    case("interleaved_dc_" + _name)(_interleaved)


# ------------------------------------------------------------------------------------------------------------------- tables and stages
TABLE_CASES = ["table_of_nine_second_level_tables", "two_symbol_tables_last_in_the_pool", "six_ac_stages_each_with_a_table_of_its_own"]  # one batch


@case(TABLE_CASES[0])
def _nine():
    """AC_PROG: 2,560 entries, the largest table the kernels take -- it sets the slot size of the batch it is in"""
    return 64, 24, GRAY, rand(9, 64, 24), iv(FOUR, 2), lambda jpeg, log: second_level_tables(AC_PROG) == 9


DC_2, AC_2 = table_from_lengths({0: 1, 1: 2}), table_from_lengths({0x00: 1, 0x01: 2})


@case(TABLE_CASES[1])
def _two_symbols():
    """every table of the file has two symbols and 256 entries; the AC table is the pool's last, so a slot of the batch's size ends behind
    the pool (stage_slot clips at pool_words)"""
    a = blank(32, 16)
    a[0][..., 0] = [[0, 1, 1, 0], [1, 0, 1, 1]]
    for b in range(8):
        for k in range(1, 1 + b % 4):
            setk(a[0], b, k, 1 if (b + k) % 2 else -1)
    script = iv([("dc", [0], 0, 0, {"dc": {0: DC_2}}), ("ac", 0, 1, 63, 0, 0, {"ac": {0: AC_2}, "max_run": 1})], 3)

    def check(jpeg, log):
        return {ev.arg for ev in log[0].events} == {0, 1} and {ev.arg for ev in find(log[1], "eob")} == {1} and len(find(log[1], "coef")) == 12 and \
            second_level_tables(AC_2) == 0 and len(AC_2[1]) == 2 and log[-1].entry[0] == "ac"
    return 32, 16, GRAY, a, script, check


def _rotated(i):
    return AC_PROG[0], AC_PROG[1][i:100] + AC_PROG[1][:i] + AC_PROG[1][100:]


@case(TABLE_CASES[2])
def _six_tables():
    rng = np.random.default_rng(6)
    a = blank(64, 24)
    a[0][...] = rng.integers(-63, 64, size=a[0].shape) * (rng.random(a[0].shape) < 0.3)
    script = [("dc", [0])] + [e + ({"ac": {0: _rotated(7 * i)}},) for i, e in enumerate(S._bit_planes(0, 5))]
    return 64, 24, GRAY, a, iv(script, 5), lambda jpeg, log: len({tuple(e[-1]["ac"][0][1]) for e in script[1:]}) == 6 == S._ac_scans([s.entry for s in log], 0)


@case("dc_four_components_four_tables")
def _dc4():
    rng = np.random.default_rng(7)
    a = blank(72, 40, CMYK)
    for arr in a:
        arr[..., 0] = rng.integers(-900, 900, size=arr.shape[:2])
    script = S._with_ac(rng, a, [("dc", [0, 1, 2, 3], 0, 0, {"dc": {2: S.DC_T2, 3: S.DC_T3}, "td": [0, 1, 2, 3]})])
    return 72, 40, CMYK, a, iv(script, [2, 3, 4, 5, 6]), lambda jpeg, log: len(log[0].events) == 4 * 45 and len(log[0].starts) == 23


def _limit(name, kind, samp, script_of, check):
    @case(name, kind)
    def fn():
        rng = np.random.default_rng(len(name))
        a = blank(40, 24, samp)
        for arr in a:
            arr[...] = rng.integers(-200, 200, size=arr.shape) * (rng.random(arr.shape) < 0.3)
        return 40, 24, samp, a, iv(script_of(), 4), lambda jpeg, log: check([s.entry for s in log]) and all(len(s.starts) == 4 for s in log)


_limit("limit_6_stages", "good", GRAY, lambda: [("dc", [0])] + S._bit_planes(0, 5), lambda es: S._ac_scans(es, 0) == 6)
_limit("limit_7_stages", "over_limit", GRAY, lambda: [("dc", [0])] + S._bit_planes(0, 6), lambda es: S._ac_scans(es, 0) == 7)
_limit("limit_15_ac_scans", "good", CMYK, lambda: [("dc", [0, 1, 2, 3])] + S._bit_planes(0, 3) + S._bit_planes(1, 3) + S._bit_planes(2, 3) + S._bit_planes(3, 2),
       lambda es: S._ac_scans(es) == 15)
_limit("limit_16_ac_scans", "over_limit", CMYK, lambda: [("dc", [0, 1, 2, 3])] + sum((S._bit_planes(c, 3) for c in range(4)), []),
       lambda es: S._ac_scans(es) == 16 and max(S._ac_scans(es, c) for c in range(4)) == 4)
_limit("limit_24_scans", "good", S444, lambda: S._DC3 + sum((S._bit_planes(c, 4) for c in range(3)), []) + S._DC3_REFINED,
       lambda es: len(es) == 24 and S._ac_scans(es) == 15)
_limit("limit_25_scans", "over_limit", S444,
       lambda: [("dc", [0], 0, 3)] + S._DC3[1:] + sum((S._bit_planes(c, 4) for c in range(3)), []) + [("dc", [0], 3, 2)] + S._DC3_REFINED,
       lambda es: len(es) == 25 and S._ac_scans(es) == 15)
_limit("limit_9_second_level_tables", "good", GRAY, lambda: list(REFINE3), lambda es: second_level_tables(AC_PROG) == 9)
_limit("limit_10_second_level_tables", "over_limit", GRAY, lambda: [("dc", [0]), ("ac", 0, 1, 63, 0, 1, {"ac": {0: S.AC_PROG_10}}), ("ac", 0, 1, 63, 1, 0)],
       lambda es: second_level_tables(S.AC_PROG_10) == 10)


# ------------------------------------------------------------------------------------------------------------------- refusals
# Legal for a sequential decoder, which forgets the run at a marker and skips what is left in front of it; a lane of the interval kernels
# vouches only for an interval that ends with no run open and fewer than 8 bits left.
def _run_open(name, refine, declared, table=None):
    @case(name, "refusal")
    def fn():
        """interval 0 (blocks 0..3) ends inside a run: blocks 2 and 3 lie in a run written as `declared` blocks long"""
        a = rand(40 + refine, 64, 8)
        for b in (2, 3):
            a[0][0, b, 1:] = 0
            if refine:
                history(a[0], b, range(1, 64) if b == 2 else range(5, 9))
        a[0][0, 1, S.ZIGZAG[63]] = 1  # block 1 completes its band
        script = iv(REFINE3 if refine else S._FIRST, 4)
        script[-1][-1].update({"declare_last_run": {0: declared}}, **({"ac": {0: table}} if table else {}))

        def check(jpeg, log):
            s = log[-1]
            run = find(s, "eob", 2)
            return len(run) == 1 and run[0].arg == declared > 2 and run[0].pos < s.starts[1] and len(s.starts) == 2 and s.pads[0] < 8 and \
                (not refine or any(c.pos == ends(run[0]) and c.nbits == 63 for c in find(s, "corr", 2)))
        return 64, 8, GRAY, a, script, check


_run_open("refuse_run_open_at_interval_end_first", False, 3)
_run_open("refuse_run_open_at_interval_end_refine", True, 7)
_run_open("refuse_eob14_take_77_run_outlasts_the_interval", True, 16384 + 5)

for _kind in KINDS:
    def _extra(seed, kind=_kind):
        """interval 0 of the scan ends on a whole byte, and a byte of ones follows: exactly 8 bits are left, the fewest a lane refuses"""
        a = rand(seed, 128, 8)
        script = iv(FOUR, 8)
        script[KINDS[kind]][-1]["extra_ones"] = {0}

        def check(jpeg, log):
            s = log[KINDS[kind]]
            return s.pads[0] == 8 and s.pads[1] < 8 and len(s.starts) == 2 and jpeg[s.raw_starts[1] - 4: s.raw_starts[1]] == b"\xff\x00" + _marker(0) and \
                all(p < 8 for k, x in enumerate(log) if k != KINDS[kind] for p in x.pads)
        return 128, 8, GRAY, a, script, check
    case("refuse_byte_of_ones_behind_the_pad_" + _kind, "refusal", tries=range(50, 450))(_extra)


# ------------------------------------------------------------------------------------------------------------------- for the tests
def get(name):
    """-> Case; its predicate is checked here as well, so that no test can use a file that is not where it says"""
    c, check = CASES[name]()
    assert check(c.jpeg, c.log), name
    return c


def holds(name):
    c, check = CASES[name]()
    return bool(check(c.jpeg, c.log))


def names(kind):
    return sorted(n for n in CASES if CASES[n]()[0].kind == kind)


real_blocks = S.real_blocks
