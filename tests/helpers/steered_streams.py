"""Test helper: one-component baseline JPEG files whose entropy-coded bytes are STEERED -- a stuffed FF 00 or an RSTn marker on a
requested raw byte offset of the scan, blocks of an exact number of bits, blocks longer than a 1,024-bit subsequence, a scan of an
exact raw or destuffed length -- so that tests can put a chosen byte on a chosen seam of the GPU entropy stage (the 16,384-byte
chunks, 64-byte lane slices and 16-byte pieces of the destuff kernels, the 1,024-bit subsequences, the 255 subsequences of a sync
workgroup, the 30 slots of a block-start record, the 128 MCUs of a block-pass group).  Plain Python; everything is generated.

The first part (scan_bits, gray_file and their small AC table) writes token lists exactly as given; tests/test_block_pass_streams.py
was its first user.  The second part (Steered) writes random but legal tokens around the placed bytes and keeps what it meant: the
coefficients of every block and the raw offsets of what it placed."""
import functools
import random

import numpy as np

from helpers import jpeg_from_coefficients as jc

# ---------------------------------------------------------------------------------------------------------------- token lists as given
# AC table: (run << 4 | size) by code length.  00 = (0,1), 01 = ZRL, 100 = EOB, 101 = (0,2), 1100 = (1,1), 1101 = (0,3), 11100 = (2,1),
# 1110100000000000 = (0,4): a 16-bit code.
AC_BITS = [0, 2, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
AC_VALS = [0x01, 0xF0, 0x00, 0x02, 0x11, 0x03, 0x21, 0x04]
AC = jc._codes(AC_BITS, AC_VALS)
DC = jc._codes(*jc.DC_LUMA)
EOB, ZRL = ("eob",), ("zrl",)


def c(run, value):
    return ("c", run, value)


def scan_bits(blocks):
    """blocks: [(dc difference, [tokens])] -> the entropy-coded bytes (stuffed, padded with ones) -- the tokens exactly as given."""
    bw = jc._Bits()
    for diff, tokens in blocks:
        nb, bits = jc._magnitude(diff)
        bw.put(*DC[nb])
        if nb:
            bw.put(bits, nb)
        for tok in tokens:
            if tok == EOB:
                bw.put(*AC[0x00])
            elif tok == ZRL:
                bw.put(*AC[0xF0])
            else:
                nb, bits = jc._magnitude(tok[2])
                bw.put(*AC[(tok[1] << 4) | nb])
                bw.put(bits, nb)
    bw.flush()
    return bytes(bw.out)


def _headers(cols, rows, quant, ac_bits, ac_vals, restart_interval=0):
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xdb" + (67).to_bytes(2, "big") + b"\x00" + bytes(quant)   # (in zigzag order)
    out += b"\xff\xc0" + (11).to_bytes(2, "big") + b"\x08" + (8 * rows).to_bytes(2, "big") + (8 * cols).to_bytes(2, "big") + b"\x01\x01\x11\x00"
    for ident, bits, vals in ((0x00, *jc.DC_LUMA), (0x10, ac_bits, ac_vals)):
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([ident]) + bytes(bits) + bytes(vals)
    if restart_interval:
        out += b"\xff\xdd" + (4).to_bytes(2, "big") + int(restart_interval).to_bytes(2, "big")
    out += b"\xff\xda" + (8).to_bytes(2, "big") + b"\x01\x01\x00\x00\x3f\x00"
    return bytes(out)


def gray_file(blocks, scan=None):
    """A one-component baseline file of len(blocks) 8x8 blocks in a row, quantizers 1."""
    return _headers(len(blocks), 1, [1] * 64, AC_BITS, AC_VALS) + (scan_bits(blocks) if scan is None else scan) + b"\xff\xd9"


# ---------------------------------------------------------------------------------------------------------------------- steered scans
# The writer's AC table.  Every code but the last is a run of ones closed by a zero, so the last, 16-bit one is fifteen ones and a zero:
#   00 (0,1)   01 (0,10)   100 EOB   101 (0,2)   110 ZRL   1110 (0,3)   11110 (0,5)   111110 (0,6)   1111110 (0,7)   11111110 (0,8)
#   111111110 (0,9)   then (1,1) (2,1) (1,2) (3,1) (1,3) (4,1) with 10..15 bits, and 1111111111111110 (0,4).
# (0,1) and (0,2) cost 3 and 5 bits with their values: fillers that reach any bit phase.  EOB ends in a zero, so the ones that pad a
# restart interval or the scan to a whole byte never complete an FF.  A (0,10) coefficient of value 1023 is ten ones, and the 16-bit
# code behind it fifteen more: up to three data bytes FF in a row.
S_BITS = [0, 2, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
S_VALS = [0x01, 0x0A, 0x00, 0x02, 0xF0, 0x03, 0x05, 0x06, 0x07, 0x08, 0x09, 0x11, 0x21, 0x12, 0x31, 0x13, 0x41, 0x04]
S_AC = jc._codes(S_BITS, S_VALS)
assert S_AC[0x04] == (0xFFFE, 16) and S_AC[0x00] == (4, 3) and S_AC[0x0A] == (1, 2)
QUANT = 8            # the quantizers: one step of any coefficient moves pixels, and DC values of +-100 stay inside 0..255 ...
QUANT_TABLE = [8] * 62 + [1, 8]   # ... but 1 at zigzag position 62 (natural order: 62 as well), where ff_at() puts the one value of
#                                  1023 it needs: with 8 there the whole block would saturate and hide whatever else goes wrong in it
assert jc.ZIGZAG[62] == 62
DC_LIMIT = 100       # |DC| of the blocks the writer chooses itself
DC_LEN = [DC[k][1] + k for k in range(12)]   # bits of a DC difference of category k, its code included: 2, 4, 5, 6, 7, 8, 10 ...
TOKEN_SIZE = {3: 1, 5: 2, 7: 3, 10: 5, 12: 6, 14: 7, 16: 8, 18: 9, 20: 4}   # bits of a run-0 coefficient with its code -> its size
TOKEN_LENS = sorted(TOKEN_SIZE)
FF_BLOCKS = ((2, 3), (2, 7), (4, 2), (4, 6))   # (DC category, 5-bit fillers) of the blocks that end in a byte FF: 65 or 73 bits


def _ff_block_bits(cat, fives):
    return DC_LEN[cat] + 3 * 3 + 14 * 3 + 2 * fives + 3


assert all(_ff_block_bits(*b) % 8 == 1 for b in FF_BLOCKS)


_ANY_BREAK, _NEAR, _BULK = (0, 1, 2, 3, 4), (3, 3, 5), (3, 5, 10, 10, 10)


def _reachable(bits):
    """Can 3-bit and 5-bit tokens add up to exactly this many bits?"""
    return bits == 0 or bits in (3, 5, 6) or bits >= 8


@functools.lru_cache(maxsize=None)
def _fits(bits, slots):
    """Can at most `slots` coefficients of the TOKEN_LENS add up to exactly `bits`?"""
    if bits == 0:
        return True
    if bits < 3 or slots == 0 or bits > 20 * slots:
        return False
    if bits >= 100 and bits <= 20 * (slots - 4):
        return True   # twenties, and at most three other tokens for what is left
    lens = (20, 18, 16) if bits >= 100 else TOKEN_LENS
    return any(_fits(bits - n, slots - 1) for n in lens)


class Steered:
    """Writes one scan.  cols: blocks per row of the picture (the rows follow from the number of blocks written; finish() pads the
    last one with empty blocks).  Positions: raw_bit / raw bytes count the scan as it lies in the file, stuffed zeros and markers
    included; dbits counts the destuffed stream (markers gone, the ones that pad an interval included), which is what the
    subsequences of the GPU stage are cut from.  Between calls a block is open in a scan without restart intervals; with
    restart_interval=1 none is."""

    def __init__(self, cols, seed, restart_interval=0):
        self.cols, self.ri = int(cols), int(restart_interval)
        self.rng = random.Random(seed)
        self.out, self.acc, self.n = bytearray(), 0, 0
        self.dbits = 0
        self.blocks = []          # [DC value, {zigzag position: value}]
        self.closed = 0
        self.pred = 0
        self.z = None             # next zigzag position of the open block
        self.limit = 0            # fillers break the open block when z gets here
        self.quiet = False        # fillers: an FF that completes now is a bug of the writer
        self.pending = False      # an interval is complete: its marker goes in front of the next block
        self.dangling = False     # a marker has been written and no block behind it yet
        self.nrst = 0
        self.stuffing_pad = False # the next padding may complete an FF (it is meant to)
        self.placed = []          # ("ff" | "rst", raw byte offset of the FF)
        self.calm = 0             # raw bit position from which fillers may use large values again

    # -- bits
    @property
    def raw_bit(self):
        return 8 * len(self.out) + self.n

    def _put(self, value, length):
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        self.dbits += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                assert not self.quiet, "a filler completed an FF"
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def _pad(self):
        if self.n:
            quiet, self.quiet = self.quiet, not self.stuffing_pad
            self._put((1 << (8 - self.n)) - 1, 8 - self.n)
            self.quiet = quiet
        self.stuffing_pad = False

    def _marker(self):
        assert self.n == 0 and self.pending
        self.out += bytes([0xFF, 0xD0 + (self.nrst & 7)])
        self.nrst += 1
        self.pred = 0
        self.pending, self.dangling = False, True

    # -- tokens
    def _open(self, cat=None):
        """Starts a block with a DC difference of category `cat` (None: a random small one), of random value and of the sign that
        keeps the DC value inside +-DC_LIMIT."""
        assert self.z is None
        if self.pending:
            self._marker()
        self.dangling = False
        if cat is None:
            cat = self.rng.choice((0, 1, 1, 2, 2, 3, 3, 4))
        diff = 0
        if cat:
            mag = self.rng.randrange(1 << (cat - 1), 1 << cat)
            signs = [s for s in (1, -1) if abs(self.pred + s * mag) <= DC_LIMIT]
            diff = self.rng.choice(signs) * mag
        nb, bits = jc._magnitude(diff)
        self._put(*DC[nb])
        if nb:
            self._put(bits, nb)
        self.pred += diff
        self.blocks.append([self.pred, {}])
        self.z = 1
        self.limit = self.rng.randrange(3, 41)

    def _coef(self, size, value=None, run=0):
        """A coefficient of `size` bits behind `run` zeros; value None: a random one of that size, either sign."""
        if value is None:
            p = self.rng.getrandbits(size) if not self.quiet or size < 5 else self.rng.getrandbits(size) & ~(1 << (size // 2))
            value = p if p >> (size - 1) else p - (1 << size) + 1
        nb, bits = jc._magnitude(value)
        assert nb == size and self.z + run <= 63
        code, length = S_AC[(run << 4) | size]
        self._put((code << size) | bits, length + size)
        self.z += run
        self.blocks[-1][1][self.z] = value
        self.z += 1

    def _zrl(self):
        assert self.z + 15 <= 63
        self._put(*S_AC[0xF0])
        self.z += 16

    def _close(self):
        if self.z < 64:
            self._put(*S_AC[0x00])
        self.z = None
        self.closed += 1
        if self.ri and self.closed % self.ri == 0:
            self._pad()
            self.pending = True

    # -- fillers
    def fill_to(self, raw_bit, room=1):
        """Filler coefficients and block breaks up to exactly this raw bit position, none of which stuffs: tokens of 3 and 5 bits
        (values of +-1 .. +-3, which saturate no pixel and so hide no error; 10-bit ones as well where no placed byte is near) and
        breaks (EOB and the next block's DC difference) of 5 to 10 bits, drawn from the seeded generator so that the stream never
        repeats itself.  Leaves a block open with room for `room` more coefficients."""
        assert self.ri == 0
        self.quiet = True
        if self.z is None:
            self._open()
        cap = 63 - room
        while True:
            r = raw_bit - self.raw_bit
            assert r >= 0, "the position asked for lies behind"
            if r == 0 and self.z <= cap:
                break
            if r >= 4096 and self.raw_bit >= self.calm:   # far from every placed byte: longer tokens, for the writer's speed
                breaks, coefs = _ANY_BREAK, (_BULK if self.z > 1 else _NEAR) if self.z < cap else ()
            elif r >= 32:
                breaks, coefs = _ANY_BREAK, _NEAR if self.z < cap else ()
            else:
                breaks = [k for k in range(5) if _reachable(r - 3 - DC_LEN[k])]
                coefs = [n for n in _NEAR if _reachable(r - n)] if self.z < cap else []
            if breaks and (self.z >= self.limit or not coefs or self.rng.random() < 0.04):
                self._close()
                self._open(self.rng.choice(breaks))
            else:
                assert coefs and r, "no filler fits: ask for a position further on"
                n = self.rng.choice(coefs)
                self._coef({3: 1, 5: 2, 10: 5}[n])
        self.quiet = False

    def fill_to_dbit(self, dbit, room=1):
        self.fill_to(self.raw_bit + dbit - self.dbits, room)

    def ff_at(self, raw_byte, run=1, lead=None):
        """A data byte FF at this raw offset of the scan (the file has FF 00 there), or `run` = 2 or 3 of them in a row (FF 00 FF 00
        [FF 00]).  One: the fifteen ones of the 16-bit code, starting `lead` (0..7) bits in front of the byte; its coefficient has 4
        bits, so the block keeps pixels that show an error.  Two: a (0,5) coefficient of value 31 in front of that code, twenty
        ones.  Three: a (0,10) coefficient of value 1023 in front of it, twenty-six with the last bit of its code."""
        ones = {1: 15, 2: 20, 3: 26}[run]   # (the last bit of the (0,10) code is a one as well)
        if lead is None:
            lead = self.rng.choice([k for k in range(8) if 8 * run <= ones - k < 8 * run + 8])
        assert 0 <= lead <= 7 and 8 * run <= ones - lead < 8 * run + 8
        # a zero bit directly in front of the ones, so that the byte in front is no FF: the code of (0,5) ends in one, that of (0,10)
        # is 01; the 16-bit code alone gets a filler of value -1 (000) in front
        if run == 3:
            # 1023 at zigzag position 62, where the quantizer is 1 (see QUANT_TABLE): a block of its own, three ZRL and 13 fillers
            # in front of it
            cat, mix = self.rng.randrange(5), [self.rng.choice((1, 2)) for _ in range(13)]
            self.fill_to(8 * raw_byte - lead - 1 - sum(2 * k + 1 for k in mix) - 9 - DC_LEN[cat] - 3)
            self._close()
            self.quiet = True
            self._open(cat)
            for _ in range(3):
                self._zrl()
            for size in mix:
                self._coef(size)
            self.quiet = False
            assert self.z == 62
            self._coef(10, 1023)
        else:
            self.fill_to(8 * raw_byte - lead - {1: 3, 2: 5}[run], room=3)
            self._coef(*{1: (1, -1), 2: (5, 31)}[run])
        self._coef(4)
        for k in range(run):
            self.placed.append(("ff", raw_byte + 2 * k))
        assert bytes(self.out[raw_byte:raw_byte + 2 * run]) == b"\xff\x00" * run
        self.calm = self.raw_bit + 4096

    # -- restart_interval = 1: every block is an interval of whole bytes
    def _interval(self, nbytes):
        """One block of exactly `nbytes` bytes, none of them FF, never all zero (so that a decoder that loses it shows), and with
        at most five padding bits: a last byte that held only the zeros of EOB could be lost unnoticed, decoders read zeros there."""
        assert self.ri == 1 and self.z is None
        while True:
            cat = self.rng.randrange(1, 7 if nbytes > 1 else 3)
            fits = [a for a in range(8 * nbytes - 5 - DC_LEN[cat] - 3, 8 * nbytes - DC_LEN[cat] - 2) if a >= 0 and _reachable(a)]
            if fits:
                break
        self.quiet = True
        self._open(cat)
        a = self.rng.choice(fits)
        while a:
            n = self.rng.choice([n for n in (3, 5) if _reachable(a - n)])
            self._coef({3: 1, 5: 2}[n])
            a -= n
        self._close()
        self.quiet = False

    def rst_at(self, raw_byte):
        """Intervals of one to three bytes up to this raw offset, and the next marker's FF exactly on it."""
        assert self.ri == 1 and self.z is None
        while True:
            rem = raw_byte - len(self.out) - (2 if self.pending else 0)
            assert rem >= 1, "the position asked for lies behind"
            self._interval(rem if rem <= 3 else self.rng.choice([k for k in (1,) * 10 + (2, 3) if rem - k - 2 >= 1]))
            if len(self.out) == raw_byte:
                break
        self._marker()
        self.placed.append(("rst", raw_byte))

    def _ff_block(self, cat, fives):
        """A whole block that ends without EOB in a 1 bit: DC difference, three ZRL, fourteen fillers (`fives` of them of 5 bits),
        and +1 at position 63.  The FF_BLOCKS are 1 bit longer than whole bytes, so in a byte-aligned interval the seven ones that
        pad it complete an FF: the interval's last data byte."""
        self._open(cat)
        start = self.dbits - DC_LEN[cat]
        for _ in range(3):
            self._zrl()
        mix = [2] * fives + [1] * (14 - fives)
        self.rng.shuffle(mix)
        for size in mix:
            self._coef(size)
        self._coef(1, 1)
        assert self.z == 64 and self.dbits - start == _ff_block_bits(cat, fives)
        self.stuffing_pad = True
        self._close()

    def ff_rst_at(self, raw_byte):
        """FF 00 FF Dn with the marker's FF on this raw offset: an interval whose last data byte is FF."""
        cat, fives = self.rng.choice(FF_BLOCKS)
        self.rst_at(raw_byte - (_ff_block_bits(cat, fives) + 7) // 8 - 3)   # (the block's bytes, its stuffed zero, the marker in front)
        self._ff_block(cat, fives)
        assert len(self.out) == raw_byte and self.out[-2:] == b"\xff\x00"
        self._marker()
        self.placed += [("ff", raw_byte - 2), ("rst", raw_byte)]

    # -- blocks of a given size
    def fixed_blocks(self, count, bits):
        """`count` blocks of exactly `bits` destuffed bits each (DC difference, coefficients, EOB), random in everything else.
        These may stuff."""
        if self.z is not None:
            self._close()
        for _ in range(count):
            cat = self.rng.choice([k for k in range(5) if _fits(bits - 3 - DC_LEN[k], 62)])
            self._open(cat)
            start = self.dbits - DC_LEN[cat]
            a, slots = bits - 3 - DC_LEN[cat], 62
            while a:
                n = self.rng.choice([n for n in TOKEN_LENS if _fits(a - n, slots - 1)])
                self._coef(TOKEN_SIZE[n])
                a, slots = a - n, slots - 1
            assert self.z < 64 and self.dbits + 3 == start + bits
            self._close()

    def long_blocks(self, count):
        """`count` blocks of 63 coefficients behind the 16-bit code each, about 1,260 bits: longer than a subsequence."""
        if self.z is not None:
            self._close()
        for _ in range(count):
            self._open()
            for _ in range(63):
                self._coef(4)
            self._close()

    # -- ends
    def _land(self, raw_bit, extra=0):
        """Closes the open block and as many further ones as complete the picture's last row (with `extra` blocks still to come), so
        that the last of them ends exactly on this raw bit position."""
        assert self.ri == 0
        if self.z is None:
            self._open()
        self.fill_to(max(raw_bit - 5 * self.cols - 200, self.raw_bit))
        m = -(self.closed + 1 + extra) % self.cols
        if m < 4:
            m += self.cols
        a = raw_bit - self.raw_bit - 3 - 5 * m     # bits for coefficients; a break costs what an empty block does
        assert a >= 0 and _reachable(a), "too close to the end: ask for a longer scan or fewer columns"
        self.quiet = True

        def share():   # the open block takes its part of what is left, so that the last one cannot be left with too much
            self.limit = min(62, self.z + -(-a // (3 * (m + 1))) + self.rng.randrange(3))

        share()
        while a:
            coefs = [n for n in (3, 5) if _reachable(a - n)] if self.z <= 62 else []
            if m and (not coefs or self.z >= self.limit):
                self._close()
                self._open(0)
                m -= 1
                share()
                continue
            n = self.rng.choice(coefs)
            self._coef({3: 1, 5: 2}[n])
            a -= n
        self._close()
        for _ in range(m):
            self._open(0)
            self._close()
        self.quiet = False
        assert self.raw_bit == raw_bit and (self.closed + extra) % self.cols == 0

    def finish(self, raw_bytes=None, dbytes=None, padding=0, ends_in_ff=False):
        """Ends the scan and returns the file.  Without arguments: the open block is closed and the last row padded with empty
        blocks.  raw_bytes: the scan is exactly that long in the file; dbytes: exactly that long destuffed, with `padding` (0..7)
        ones behind the last block; ends_in_ff (with raw_bytes): the last data byte is FF, so the scan ends FF 00 in front of EOI."""
        if ends_in_ff:
            cat, fives = self.rng.choice(FF_BLOCKS)
            self._land(8 * (raw_bytes - 2) + 1 - _ff_block_bits(cat, fives), extra=1)
            self._ff_block(cat, fives)
            self.stuffing_pad = True
            self.placed.append(("ff", raw_bytes - 2))
        elif raw_bytes is not None:
            self._land(8 * raw_bytes - self.rng.randrange(7))
        elif dbytes is not None:
            self._land(self.raw_bit + 8 * dbytes - padding - self.dbits)
        elif self.ri == 1:
            while self.closed % self.cols or self.dangling or not self.closed:
                self._interval(self.rng.choice((1, 1, 2)))
        else:
            if self.z is not None:
                self._close()
            while self.closed % self.cols:
                self._open(0)
                self._close()
        self._pad()
        assert self.z is None and self.closed % self.cols == 0 and not self.dangling and self.n == 0
        assert raw_bytes is None or len(self.out) == raw_bytes
        assert dbytes is None or self.dbits == 8 * dbytes
        for kind, at in self.placed:
            assert self.out[at] == 0xFF and (self.out[at + 1] == 0 if kind == "ff" else 0xD0 <= self.out[at + 1] <= 0xD7), (kind, at)
        assert self.ri == 0 or self.nrst == -(-self.closed // self.ri) - 1
        self.scan = bytes(self.out)
        self.header = _headers(self.cols, self.closed // self.cols, QUANT_TABLE, S_BITS, S_VALS, self.ri)
        self.jpeg = self.header + self.scan + b"\xff\xd9"
        return self.jpeg

    def coefficients(self):
        """What the writer meant: int16 [rows, cols, 64] in natural order."""
        out = np.zeros((self.closed, 64), np.int16)
        for b, (dc, ac) in enumerate(self.blocks):
            out[b, 0] = dc
            for z, v in ac.items():
                out[b, jc.ZIGZAG[z]] = v
        return out.reshape(self.closed // self.cols, self.cols, 64)


def mutants(s):
    """For every placed byte of a finished Steered, files that are what a destuffing gone wrong at that byte would have decoded:
    [(name, file, shows)].  A stuffed FF: its 00 kept as data, the FF 00 pair lost, the byte behind it lost.  A marker: the same
    three (a zero byte behind it kept, the marker lost, the byte behind it lost), and also one marker byte kept as data, the byte
    in front lost.  shows: False for the one variant no file can show -- a kept 00 that would be the last byte of its restart
    interval or of the scan, behind the last bit of the last block, where every decoder skips to the marker.  (On the device
    such a byte would still move everything behind it; only its imitation in a file is blind there.)"""
    res = []

    def variant(name, at, cut, insert=b"", shows=True):
        scan = s.scan[:at] + insert + s.scan[at + cut:]
        res.append((name, s.header + scan + b"\xff\xd9", shows))

    for kind, at in s.placed:
        tag = "%s@%d:" % (kind, at)
        last = kind == "ff" and (at + 2 == len(s.scan) or s.scan[at + 2] == 0xFF and s.scan[at + 3] >= 0xD0)
        variant(tag + "zero kept", at + 2, 0, b"\x00", shows=not last)
        variant(tag + "pair lost", at, 2)
        if at + 2 < len(s.scan):
            variant(tag + "byte behind lost", at + 2, 1)
        if kind == "rst":
            variant(tag + "marker byte kept", at + 2, 0, s.scan[at + 1:at + 2])
            variant(tag + "byte in front lost", at - 1, 1)
    return res


# ---------------------------------------------------------------------------------------------------------------------- file families
# What tests/test_steered_streams.py checks on the CPU and tests/test_gpu_steered_streams.py decodes on the device.  Each family is a
# list of finished Steered objects (.jpeg, .scan, .placed, .coefficients()), built once per process.
CHUNK = 16384          # bytes of the raw scan per destuff workgroup
WG_BYTES = 255 * 128   # destuffed bytes of one sync workgroup: kHuffOwn subsequences of 1,024 bits


def _seams():
    """One chunk each: a stuffed FF on, in front of and behind the 16-byte piece, 64-byte lane and 4,096-byte seams; runs of two and
    three across a lane seam.  The scans end at different lengths mod 16."""
    res = []
    for s in (16, 64, 128, 4096 - 64 * 3, 4096):
        for d in (-2, -1, 0, 1):
            w = Steered(16, 1000 + 4 * s + d)
            w.ff_at(s + d)
            res.append((w, s + d + 40 + (s + d) % 7))
    for run, offs in ((2, (-3, -2, -1, 0)), (3, (-5, -4, -3, -2, -1, 0))):
        for d in offs:     # (the run's first FF at 64k + d: its bytes lie on both sides of the seam, or start exactly on it)
            w = Steered(16, 2000 + 10 * run + d)
            w.ff_at(64 * 5 + d, run=run)
            res.append((w, 64 * 5 + 60 + d % 3))
    out = []
    for k, (w, end) in enumerate(res):
        w.finish(raw_bytes=end + (k % 3 == 0) * ((-end) % 16) + (k % 3 == 1) * ((1 - end) % 16) + (k % 3 == 2) * ((15 - end) % 16))
        out.append(w)
    assert {len(w.scan) & 15 for w in out} == {0, 1, 15}
    return out


def _chunks():
    """Three chunks and a bit: a stuffed FF at 16384 + d and at 32768 + d, and 0..3 further ones early in chunk 0, which shift the
    later chunks' destuffed output to every alignment mod 4."""
    out = []
    for d in (-2, -1, 0, 1):
        for early in range(4):
            w = Steered(64, 3000 + 10 * d + early)
            for k in range(early):
                w.ff_at(100 + 50 * k)
            w.ff_at(CHUNK + d)
            w.ff_at(2 * CHUNK + d)
            w.finish(raw_bytes=2 * CHUNK + 700 + 13 * early)
            assert sum(1 for kind, at in w.placed if at < CHUNK - 2) == early
            out.append(w)
    return out


def _last_chunk():
    """Raw scan lengths that leave 1..65 bytes for the last chunk, or nothing; some of them end FF 00."""
    out = []
    for k, n in enumerate((1, 2, 3, 4, 15, 16, 17, 63, 64, 65)):
        w = Steered(32, 4000 + n)
        for early in range(k % 4):   # (the last chunk's output at every alignment mod 4, also where it is 1..4 bytes long)
            w.ff_at(200 + 70 * early)
        w.ff_at(CHUNK - 300 + n)
        out.append(w)
        w.finish(raw_bytes=CHUNK + n, ends_in_ff=n in (2, 17))
    for total in (CHUNK, 2 * CHUNK):
        for ends_in_ff in (False, True):
            w = Steered(32, 4100 + total // CHUNK + ends_in_ff)
            w.ff_at(total - 500)
            w.finish(raw_bytes=total, ends_in_ff=ends_in_ff)
            out.append(w)
    return out


def _restart_placed():
    """restart_interval = 1: a marker's FF on, in front of and two in front of the chunk seam, and on either side of lane seams;
    FF 00 FF Dn across a lane seam and across the chunk seam."""
    out = []
    for k, at in enumerate((CHUNK - 1, CHUNK, CHUNK - 2, 64 * 3 - 1, 64 * 3, 64 * 40 - 1, 64 * 40)):
        w = Steered(32, 5000 + k, restart_interval=1)
        w.rst_at(at)
        if at < CHUNK - 2:
            w.rst_at(at + 64 * 7)   # (a second lane seam further on, same side)
        w.finish()
        out.append(w)
    for k, at in enumerate((64 * 4 + 1, 64 * 4, 64 * 4 - 1, CHUNK + 1, CHUNK, CHUNK - 1)):
        w = Steered(32, 5100 + k, restart_interval=1)   # FF 00 | FF Dn, FF | 00 FF Dn, FF 00 FF | Dn
        w.ff_rst_at(at)
        w.finish()
        out.append(w)
    return out


def _restart_intervals():
    """Intervals of 2, 7 and 128 blocks (and 127 and 129) of 64-bit blocks: 16 blocks a subsequence, so interval boundaries fall on
    subsequence boundaries and on block-pass group boundaries (128 blocks), and one block in front of and behind both."""
    out = []
    for k, ri in enumerate((2, 7, 128, 127, 129)):
        w = Steered(64, 5200 + k, restart_interval=ri)
        w.fixed_blocks(64 * 7, 64)
        w.finish()
        out.append(w)
    return out


def _stream_ends():
    """Destuffed lengths around one subsequence, one sync workgroup (255 subsequences), one more subsequence and two workgroups, each
    with the last block ending on a byte boundary and with seven padding bits."""
    out = []
    for n in (127, 128, 129, WG_BYTES - 1, WG_BYTES, WG_BYTES + 1, WG_BYTES + 128, 2 * WG_BYTES - 1, 2 * WG_BYTES + 1):
        for padding in (0, 7):
            w = Steered(8 if n < 1000 else 64, 6000 + 2 * n + padding)
            if n > 1000:
                w.ff_at(300 + n % 50)
            w.finish(dbytes=n, padding=padding)
            out.append(w)
    return out


def _record_slots():
    """Blocks of 33, 34 and 35 bits: 31/32, 30/31 and 29/30 block starts per subsequence, the edge of a record of 30 slots; blocks
    of exactly 1,024 and 512 bits, each starting on bit 0 of a subsequence.  40 rows of 64 blocks."""
    out = []
    for bits in (33, 34, 35, 1024, 512):
        w = Steered(64, 7000 + bits)
        w.fixed_blocks(64 * 40, bits)
        w.finish()
        out.append(w)
    return out


def _long_blocks():
    """Runs of blocks longer than a subsequence between short ones; in the last file a run lies across the end of the first sync
    workgroup's 32,640 bytes."""
    out = []
    for k, runs in enumerate(((1, 1, 2), (3, 5), (2, 9, 1))):
        w = Steered(16, 8000 + k)
        for r in runs:
            w.fill_to(w.raw_bit + 700 + 37 * r)
            w.long_blocks(r)
            w.fixed_blocks(3, 33)
        w.finish()
        out.append(w)
    w = Steered(64, 8010)
    w.fill_to_dbit(8 * WG_BYTES - 2 * 1260 - 300)
    w.long_blocks(5)
    assert w.dbits > 8 * WG_BYTES + 2 * 1260
    w.fill_to(w.raw_bit + 3000)
    w.long_blocks(2)
    w.finish()
    out.append(w)
    return out


def _strips():
    """One row of 127 .. 257 blocks: one and two block-pass groups of 128, one block short, exact, one block over."""
    out = []
    for n in (127, 128, 129, 255, 256, 257):
        w = Steered(n, 9000 + n)
        w.ff_at(40)
        w.fill_to(w.raw_bit + 40 * n)
        while w.closed + 1 < n:       # (few bits a block so far: whatever is missing, as blocks of 33 bits)
            w.fixed_blocks(min(n - w.closed - (w.z is not None), 8), 33)
        w.finish()
        assert w.closed == n
        out.append(w)
    return out


FAMILIES = {"seams": _seams, "chunks": _chunks, "last_chunk": _last_chunk, "restart_placed": _restart_placed,
            "restart_intervals": _restart_intervals, "stream_ends": _stream_ends, "record_slots": _record_slots,
            "long_blocks": _long_blocks, "strips": _strips}


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


def pixels(w):
    """The oracle's gray pixels of a finished Steered, computed once."""
    import oracle
    if not hasattr(w, "_pixels"):
        w._pixels = oracle.decode(w.jpeg, oracle.FMT_GRAY)
    return w._pixels


def decode_on_device(dec, files, inputs=None):
    """Decodes the files (finished Steered objects) as ONE batch through the GPU entropy stage and compares the pixels with the
    oracle's, bit for bit.  Every one of them must have been decoded by the GPU entropy stage, none handed back to the host decoder.
    inputs: what to pass instead of the files' bytes (the same bitstreams held elsewhere)."""
    import torch
    outs, st = dec.decode([w.jpeg for w in files] if inputs is None else inputs, fmt="y", gpu_huffman=True)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(files)
    assert dec.host_fallbacks() == 0
    for k, (w, o) in enumerate(zip(files, outs)):
        got, want = o.cpu().numpy(), pixels(w)
        assert np.array_equal(got, want), "file %d of the batch (placed: %s): first differing pixel (y, x) = %s" % (
            k, w.placed, tuple(np.argwhere(got != want)[0]))
