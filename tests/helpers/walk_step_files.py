"""Test helper: files for the forms of the synchronisation walk's select step (csrc/huffman_gpu_core.h select_walk) -- the MCU
position as a countdown, the pair entry in the single entry's layout with its test z + z1 < 64, and long codes as steps of their
own.  Three writers place chosen tokens on chosen bits: steered_streams.Steered (its own AC table: ZRL, EOB and (0,1) in 3 bits,
(0,2) in 5), walk_files.LongCodes (codes of 11 to 16 bits), and PairStream below over PAIR_AC, a table with a 2-bit ZRL and 8-bit
symbols, so that a 10-bit window can hold 2 + 8 bits.  Every case is a function that writes into an open writer; small() makes a
short file of one case, combined() one long stream per writer with every case in each of three sync workgroups' ranges.

PAIR_AC   00 ZRL   01 (0,1)   100 EOB   101 (0,2)   1100 (0,4)   1101 (1,1)   11100 (0,3)   11101 (2,1)
with their value bits: ZRL 2, (0,1) 3, EOB 3, (0,2) 5, (1,1) 5, (2,1) 6, (0,4) 8, (0,3) 8 bits."""
import functools
import random

import numpy as np

from helpers import jpeg_from_coefficients as jc
from helpers import steered_streams as ss
from helpers import walk_files as W

PAIR_AC = ([0, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0xF0, 0x01, 0x00, 0x02, 0x04, 0x11, 0x03, 0x21])
P_AC, P_DC = jc._codes(*PAIR_AC), jc._codes(*jc.DC_LUMA)
assert P_AC[0xF0] == (0, 2) and P_AC[0x01] == (1, 2) and P_AC[0x00] == (4, 3) and P_AC[0x04] == (12, 4) and P_AC[0x03] == (28, 5)
WG_BITS = 255 * 1024      # bits of the subsequences one sync workgroup owns


class PairStream:
    """One scan over (Annex K luma DC, PAIR_AC), token by token; positions are bits of the destuffed stream.  The interface of
    walk_files.LongCodes: open / coef / zrl / eob / fill_to / finish / coefficients, .jpeg, .total_bits, .placed."""

    def __init__(self, cols, seed):
        self.cols = cols
        self.rng = random.Random(seed)
        self.bits, self.blocks, self.pred, self.z, self.placed = [], [], 0, None, []

    @property
    def pos(self):
        return len(self.bits)

    def _put(self, value, length):
        self.bits += [(value >> (length - 1 - i)) & 1 for i in range(length)]

    def open(self, cat=None):
        assert self.z is None
        if cat is None:
            cat = self.rng.randrange(4)
        diff = 0
        if cat:
            mag = self.rng.randrange(1 << (cat - 1), 1 << cat)
            diff = mag if self.pred <= 0 else -mag
        nb, bits = jc._magnitude(diff)
        self._put(*P_DC[nb])
        if nb:
            self._put(bits, nb)
        self.pred += diff
        self.blocks.append([self.pred, {}])
        self.z = 1

    def coef(self, run, size, value=None):
        if value is None:
            mag = self.rng.randrange(1 << (size - 1), 1 << size)
            value = mag if self.rng.random() < 0.5 else -mag
        nb, bits = jc._magnitude(value)
        assert nb == size and self.z + run <= 63
        code, length = P_AC[(run << 4) | size]
        self._put((code << size) | bits, length + size)
        self.z += run
        self.blocks[-1][1][self.z] = value
        self.z += 1

    def zrl(self):
        assert self.z + 15 <= 63
        self._put(*P_AC[0xF0])
        self.z += 16

    def eob(self):
        if self.z < 64:
            self._put(*P_AC[0x00])
        self.z = None

    def fill_to(self, bit, room=2):
        """3-bit and 5-bit coefficients and block breaks (EOB and a DC difference of category 0: 5 bits) up to exactly this bit;
        leaves a block open with room for `room` more coefficients"""
        if self.z is None:
            self.open()
        while True:
            r = bit - self.pos
            assert r >= 0, "the position asked for lies behind"
            if r == 0:
                assert self.z <= 63 - room
                return
            if self.z > 40 - room and ss._reachable(r - 5):
                self.eob()
                self.open(0)
                continue
            fits = [n for n in (3, 5) if ss._reachable(r - n)]
            assert fits and self.z < 63 - room, "no filler fits: ask for a position further on"
            self.coef(0, {3: 1, 5: 2}[self.rng.choice(fits)])

    def finish(self):
        if self.z is not None:
            self.eob()
        while len(self.blocks) % self.cols:
            self.open(0)
            self.eob()
        self.total_bits = self.pos
        self._put((1 << (-self.pos % 8)) - 1, -self.pos % 8)
        data = bytearray()
        for b in np.packbits(np.array(self.bits, np.uint8)).tolist():
            data.append(b)
            if b == 0xFF:
                data.append(0)
        rows = len(self.blocks) // self.cols
        head = bytearray(b"\xff\xd8")
        head += b"\xff\xdb" + (67).to_bytes(2, "big") + b"\x00" + bytes([4] * 64)
        head += b"\xff\xc0" + (11).to_bytes(2, "big") + b"\x08" + (8 * rows).to_bytes(2, "big") + (8 * self.cols).to_bytes(2, "big") + b"\x01\x01\x11\x00"
        head += W._dht(0, 0, jc.DC_LUMA) + W._dht(1, 0, PAIR_AC)
        head += b"\xff\xda" + (8).to_bytes(2, "big") + b"\x01\x01\x00\x00\x3f\x00"
        self.jpeg = bytes(head) + bytes(data) + b"\xff\xd9"
        return self.jpeg

    def coefficients(self):
        out = np.zeros((len(self.blocks), 64), np.int16)
        for b, (dc, ac) in enumerate(self.blocks):
            out[b, 0] = dc
            for z, v in ac.items():
                out[b, jc.ZIGZAG[z]] = v
        return out.reshape(len(self.blocks) // self.cols, self.cols, 64)


def _fresh_block_at(w, z):
    """closes the open block and opens one whose next zigzag position is exactly z, by single (0,1) coefficients"""
    if w.z is not None:
        w.eob()
    w.open()
    while w.z < z:
        w.coef(0, 1)


# ------------------------------------------------------------------------------------------------ the pair test at its edges (PairStream)
def p_sum_62(w):       # z + z1 = 62: the pair (1,1) + (0,1) is taken, then (0,1) completes the block
    _fresh_block_at(w, 60)
    w.coef(1, 1)
    w.coef(0, 1)
    w.coef(0, 1)
    assert w.z == 64
    w.eob()


def p_sum_63(w):       # z + z1 = 63: the pair (2,1) + EOB
    _fresh_block_at(w, 60)
    w.coef(2, 1)
    assert w.z == 63
    w.eob()


def p_sum_64(w):       # z + z1 = 64: no pair -- the bits behind (1,1) are the next block's DC symbol
    _fresh_block_at(w, 62)
    w.coef(1, 1)
    assert w.z == 64
    w.eob()
    w.open(2)
    w.coef(0, 2)


def p_sum_64_by_one(w):   # the same with the shortest symbol, (0,1) from z = 63, and a DC difference of category 0 behind it
    _fresh_block_at(w, 63)
    w.coef(0, 1)
    w.eob()
    w.open(0)
    w.coef(0, 1)


def p_zrl_sums(w):     # ZRL as the first symbol from z = 46 (62) and 47 (63)
    _fresh_block_at(w, 46)
    w.zrl()
    w.coef(0, 1)
    w.eob()
    _fresh_block_at(w, 47)
    w.zrl()
    assert w.z == 63
    w.eob()


def p_eob_second(w):   # EOB as the second symbol from z = 1, 62 (and from 63 there is none: p_sum_64_by_one)
    for z in (1, 62):
        _fresh_block_at(w, z)
        w.coef(0, 1)
        w.eob()


def p_zrl_first_and_second(w):
    _fresh_block_at(w, 3)
    w.zrl()            # 2 + 3 bits
    w.coef(0, 1)
    w.coef(0, 1)       # 3 + 2 bits
    w.zrl()
    w.coef(0, 2)


def p_five_and_five(w):   # a window of two 5-bit symbols
    _fresh_block_at(w, 5)
    w.coef(0, 2)
    w.coef(1, 1)
    w.coef(1, 1)
    w.coef(0, 2)


def p_two_and_eight(w):   # a window of 2 + 8 bits
    _fresh_block_at(w, 2)
    w.zrl()
    w.coef(0, 4)
    w.zrl()
    w.coef(0, 3)


def p_pair_ends_stream(w):   # (0,1) + (0,1) from z = 62: the stream's last two symbols, one step, and no EOB behind them
    _fresh_block_at(w, 62)
    w.coef(0, 1)
    w.coef(0, 1)
    assert w.z == 64


PAIR_CASES = [p_sum_62, p_sum_63, p_sum_64, p_sum_64_by_one, p_zrl_sums, p_eob_second, p_zrl_first_and_second, p_five_and_five,
              p_two_and_eight]


# ------------------------------------------------------------------------------------------------ the loop split (Steered: exact bits)
def s_pair_across(d):
    """the pair (0,1) + (0,2), 3 + 5 bits: its second symbol starts at end + d of a 1,024-bit subsequence"""
    def case(w):
        at = (w.dbits + 200 + 1023) // 1024 * 1024 + d
        w.fill_to_dbit(at - 3, room=3)
        w._coef(1)
        assert w.dbits == at
        w._coef(2)
    case.__name__ = "s_pair_across_%+d" % d
    return case


def s_zrl_pairs(w):    # ZRL (3 bits here) as first and as second symbol
    w.fill_to(w.raw_bit + 40, room=40)
    w._zrl()
    w._coef(1)
    w._coef(1)
    w._zrl()


def s_pair_ends_stream(w):
    """the last two symbols of the stream are the pair, and it completes the last block (z = 62: no EOB behind it)"""
    w.fill_to(w.raw_bit + 100)
    w._close()
    w._open()
    while w.z < 62:
        w._coef(1)
    w._coef(1)
    w._coef(2)
    assert w.z == 64


STEERED_CASES = [s_pair_across(-1), s_pair_across(0), s_pair_across(1), s_zrl_pairs]


# ------------------------------------------------------------------------------------------------ long codes (LongCodes)
def l_behind_a_pair(w):      # (0,1) + (0,2): 3 + 5 bits, then the 16-bit code
    w.fill_to(w.pos + 50, room=10)
    w.coef(0, 1)
    w.coef(0, 2)
    w.coef(0, 4)
    w.coef(0, 1)
    w.coef(0, 2)
    w.coef(2, 1)


def l_last_of_a_subsequence(w):   # (2,1), 14 + 1 bits, ends exactly on a subsequence's last bit
    at = (w.pos + 300 + 1023) // 1024 * 1024 - 15
    w.fill_to(at, room=5)
    w.coef(2, 1)
    assert w.pos % 1024 == 0


def l_word_phases(w):        # the first half starts at bit 31 of a word, and at bit 0
    for phase in (31, 0):
        w.fill_to((w.pos + 100 + 31) // 32 * 32 + phase, room=4)
        assert w.pos % 32 == phase
        w.coef(1, 3)


def l_two_in_a_row(w):
    w.fill_to(w.pos + 60, room=24)
    w.coef(0, 4)
    w.coef(1, 2)
    w.zrl()
    w.coef(2, 1)


def l_closes_a_block(w):     # (1,2) from z = 62: the advance of a long code takes the block to 64
    w.fill_to(w.pos + 40, room=10)
    w.eob()
    w.open()
    while w.z < 62:
        w.coef(0, 1)
    w.coef(1, 2)
    assert w.z == 64
    w.eob()
    w.open(3)                # (an 11-bit DC code behind it)


LONG_CASES = [l_behind_a_pair, l_last_of_a_subsequence, l_word_phases, l_two_in_a_row, l_closes_a_block]


def l_long_code_ends_stream(w):
    l_closes_a_block(w)
    w.fill_to(w.pos + 30, room=10)
    w.eob()
    w.open()
    while w.z < 62:
        w.coef(0, 1)
    w.coef(1, 2)             # the stream's last symbol, and its block's
    assert w.z == 64


# ------------------------------------------------------------------------------------------------ files
def _writer(kind, cols, seed):
    return {"pair": PairStream, "long": W.LongCodes}[kind](cols, seed) if kind != "steered" else ss.Steered(cols, seed)


def _position(w):
    return w.dbits if isinstance(w, ss.Steered) else w.pos


def _fill(w, bit):
    if isinstance(w, ss.Steered):
        w.fill_to_dbit(bit)
    else:
        w.fill_to(bit)


CASES = {"pair": PAIR_CASES, "steered": STEERED_CASES, "long": LONG_CASES}
LAST = {"pair": p_pair_ends_stream, "steered": s_pair_ends_stream, "long": l_long_code_ends_stream}


@functools.lru_cache(maxsize=None)
def small():
    """[(name, finished writer)]: every case alone in a file of a few subsequences, and the cases that end a stream"""
    out = []
    for kind, cases in CASES.items():
        for k, case in enumerate(cases):
            w = _writer(kind, 8, 100 + k)
            _fill(w, 1024 + 37 * k + 300)
            case(w)
            _fill(w, _position(w) + 1500)
            w.finish()
            out.append(("%s_%s" % (kind, case.__name__), w))
        w = _writer(kind, 1, 200)
        _fill(w, 2048 + 300)
        LAST[kind](w)
        w.finish()
        out.append(("%s_%s_ends_stream" % (kind, LAST[kind].__name__), w))
    return out


@functools.lru_cache(maxsize=None)
def combined():
    """[(name, finished writer)]: one stream per writer, three sync workgroups and a halo long, every case of the writer in each
    workgroup's range and the stream-ending case last"""
    out = []
    for kind, cases in CASES.items():
        w = _writer(kind, 64, 300)
        for g in range(3):
            _fill(w, g * WG_BITS + 2000 + 700 * g)
            for case in cases:
                case(w)
                _fill(w, _position(w) + 300)
            _fill(w, (g + 1) * WG_BITS - 3000)
        _fill(w, 3 * WG_BITS + 2048)
        LAST[kind](w)
        w.finish()
        out.append(("combined_" + kind, w))
    return out


# every wrap of the countdown: blocks_per_mcu 1, 3, 4, 6 and 10; one to four table classes
SAMPLINGS = {
    "gray_1": ([(1, 1)], [W.LUMA]),
    "444_3": ([(1, 1)] * 3, [W.LUMA, W.CHROMA, W.CHROMA]),
    "422_4": ([(2, 1), (1, 1), (1, 1)], [W.LUMA, W.CHROMA, W.CHROMA]),
    "420_6": ([(2, 2), (1, 1), (1, 1)], [W.LUMA, W.CHROMA, W.CHROMA]),
    "h4v2_10": ([(4, 2), (1, 1), (1, 1)], [W.LUMA, W.CHROMA, W.CHROMA]),
    "444_three_classes": ([(1, 1)] * 3, [W.LUMA, W.CHROMA, W.LUMA_REVERSED]),
    "420_three_classes": ([(2, 2), (1, 1), (1, 1)], [W.CHROMA_REVERSED, W.LUMA, W.CHROMA]),
    "four_classes": ([(1, 1)] * 4, [W.LUMA, W.CHROMA, (jc.DC_LUMA, jc.AC_CHROMA), (jc.DC_CHROMA, jc.AC_LUMA)]),
}


@functools.lru_cache(maxsize=None)
def sampling_files(min_bits):
    """[(name, file, coefficients, sampling)] of SAMPLINGS, each scan at least min_bits long (destuffed)"""
    out = []
    for k, (name, (samp, tables)) in enumerate(SAMPLINGS.items()):
        side, bits = 32, 0
        while bits < min_bits:   # (a 32 x 32 probe, the size its bits per pixel call for, and 32 more while that falls short)
            side = side + 32 if bits else 32
            coefs = jc.random_coefficients(np.random.default_rng(500 + k), side, side, samp, 40, dense=10, small=5, dc=40)
            jpeg = W.write_scans(side, side, samp, coefs, tables)
            first, bits = bits == 0 and side == 32, W.scan_bits(jpeg)[0]
            if first and bits < min_bits:
                side = max(32, int(32 * (min_bits / bits) ** 0.5) // 32 * 32)
        out.append((name, jpeg, coefs, samp))
    return out
