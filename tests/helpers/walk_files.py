"""Test helper: sequential JPEG files written from CHOSEN coefficients with a CHOSEN (DC, AC) Huffman table pair per component, chosen
sampling factors and a chosen split into scans -- the files that decide which tables the GPU entropy walks select at every MCU
position (one to four distinct pairs over up to ten positions) -- and one-component streams written token by token over tables
whose codes are LONG (more than the ten bits of the walks' first-level lookup), with a long code placed on a chosen bit of the
destuffed stream.  Plain Python + numpy; everything is generated.

Table specs are (bits[16], vals) as in a DHT segment.  Besides the Annex K tables there are two more complete pairs, the Annex K
code lengths with the symbols in reverse order: every symbol still has a code, the frequent ones now the 16-bit ones, so streams
coded with them are mostly long codes, DC differences included (category 0 gets 9 or 11 bits)."""
import copy
import functools

import numpy as np

from helpers import jpeg_from_coefficients as jc
from helpers import steered_streams as ss

LUMA = (jc.DC_LUMA, jc.AC_LUMA)
CHROMA = (jc.DC_CHROMA, jc.AC_CHROMA)
LUMA_REVERSED = ((jc.DC_LUMA[0], jc.DC_LUMA[1][::-1]), (jc.AC_LUMA[0], jc.AC_LUMA[1][::-1]))
CHROMA_REVERSED = ((jc.DC_CHROMA[0], jc.DC_CHROMA[1][::-1]), (jc.AC_CHROMA[0], jc.AC_CHROMA[1][::-1]))


def _dht(tc, th, spec):
    bits, vals = spec
    return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)


def write_scans(width, height, sampling, coefficients, tables, scans=None, quant=4, restart_interval=0):
    """sampling: [(h, v)] per component; coefficients[c]: int array [blocks_h][blocks_w][64], natural order, over the MCU-padded grid
    (jc.block_grid), DC values absolute; tables[c] = (DC spec, AC spec) of component c -- equal specs share a table slot, distinct
    ones get slots 0, 1, 2, 3 in order of appearance (slots above 1 make the frame an extended-sequential one, SOF1); scans: lists of
    component indices, default one scan of all components.  An interleaved scan walks the frame's MCU grid, a one-component scan
    the component's real blocks in raster order (T.81 A.2).  quant: every quantizer.  Returns the file."""
    ncomp = len(sampling)
    scans = [list(range(ncomp))] if scans is None else scans
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcus_x, mcus_y = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    dc_specs, ac_specs = [], []
    for dc, ac in tables:
        if dc not in dc_specs:
            dc_specs.append(dc)
        if ac not in ac_specs:
            ac_specs.append(ac)
    assert len(dc_specs) <= 4 and len(ac_specs) <= 4
    slot = [(dc_specs.index(dc), ac_specs.index(ac)) for dc, ac in tables]
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xdb" + (67).to_bytes(2, "big") + b"\x00" + bytes([quant] * 64)
    sof = b"\xff\xc0" if max(len(dc_specs), len(ac_specs)) <= 2 else b"\xff\xc1"
    out += sof + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(sampling):
        out += bytes([c + 1, (h << 4) | v, 0])
    for th, spec in enumerate(dc_specs):
        out += _dht(0, th, spec)
    for th, spec in enumerate(ac_specs):
        out += _dht(1, th, spec)
    if restart_interval:
        out += b"\xff\xdd" + (4).to_bytes(2, "big") + int(restart_interval).to_bytes(2, "big")
    dc_codes = [jc._codes(*tables[c][0]) for c in range(ncomp)]
    ac_codes = [jc._codes(*tables[c][1]) for c in range(ncomp)]
    for scan in scans:
        out += b"\xff\xda" + (6 + 2 * len(scan)).to_bytes(2, "big") + bytes([len(scan)])
        for c in scan:
            out += bytes([c + 1, (slot[c][0] << 4) | slot[c][1]])
        out += b"\x00\x3f\x00"
        if len(scan) == 1:
            c = scan[0]
            h, v = sampling[c]
            sw, sh = -(-width * h // hmax), -(-height * v // vmax)
            mcus = [[(c, y, x)] for y in range(-(-sh // 8)) for x in range(-(-sw // 8))]
        else:
            mcus = [[(c, my * sampling[c][1] + by, mx * sampling[c][0] + bx) for c in scan for by in range(sampling[c][1])
                     for bx in range(sampling[c][0])] for my in range(mcus_y) for mx in range(mcus_x)]
        bw = jc._Bits()
        pred = [0] * ncomp
        for m, mcu in enumerate(mcus):
            if restart_interval and m and m % restart_interval == 0:
                bw.flush()
                bw.out += bytes([0xFF, 0xD0 + (m // restart_interval - 1) % 8])
                pred = [0] * ncomp
            for c, y, x in mcu:
                blk = coefficients[c][y][x]
                diff = int(blk[0]) - pred[c]
                pred[c] = int(blk[0])
                nb, bits = jc._magnitude(diff)
                assert nb <= 11
                bw.put(*dc_codes[c][nb])
                if nb:
                    bw.put(bits, nb)
                run = 0
                for k in range(1, 64):
                    val = int(blk[jc.ZIGZAG[k]])
                    if val == 0:
                        run += 1
                        continue
                    while run > 15:
                        bw.put(*ac_codes[c][0xF0])
                        run -= 16
                    nb, bits = jc._magnitude(val)
                    assert nb <= 10
                    bw.put(*ac_codes[c][(run << 4) | nb])
                    bw.put(bits, nb)
                    run = 0
                if run:
                    bw.put(*ac_codes[c][0x00])
        bw.flush()
        out += bw.out
    out += b"\xff\xd9"
    return bytes(out)


def scan_bits(jpeg):
    """Destuffed bits of every scan of the file (restart markers taken out)."""
    res, pos = [], 2
    while pos < len(jpeg):
        assert jpeg[pos] == 0xFF
        m = jpeg[pos + 1]
        if m == 0xD9:
            break
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        pos += 2 + n
        if m != 0xDA:
            continue
        bits = 0
        while True:
            if jpeg[pos] != 0xFF:
                bits, pos = bits + 8, pos + 1
            elif jpeg[pos + 1] == 0:
                bits, pos = bits + 8, pos + 2
            elif 0xD0 <= jpeg[pos + 1] <= 0xD7:
                pos += 2
            else:
                break
        res.append(bits)
    return res


# ------------------------------------------------------------------------------------------------------------- table-class files
def _coefficients(seed, width, height, sampling):
    return jc.random_coefficients(np.random.default_rng(seed), width, height, sampling, 40, dense=10, small=5, dc=40)


@functools.lru_cache(maxsize=None)
def class_files():
    """[(name, file, the coefficients it was written from, sampling)]: one to four distinct table pairs, blocks_per_mcu 1, 3, 4, 6 and 10"""
    g, y420, y444, y42 = [(1, 1)], [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3, [(4, 2), (1, 1), (1, 1)]
    four = [(1, 1)] * 4
    cases = [
        ("gray_one_pair", 64, 64, g, [LUMA], None),
        ("420_two_pairs", 48, 48, y420, [LUMA, CHROMA, CHROMA], None),
        ("444_pair_changes_every_block", 32, 32, y444, [LUMA, CHROMA, LUMA], None),
        ("luma42_ten_positions", 64, 32, y42, [LUMA, CHROMA, CHROMA], None),
        ("three_pairs", 32, 32, y444, [LUMA, CHROMA, LUMA_REVERSED], None),
        ("420_three_pairs", 32, 32, y420, [CHROMA_REVERSED, LUMA, CHROMA], None),
        # (four pairs of their own tables would not fit the 12,288 table entries the kernels accept: two DC and two AC tables, crossed)
        ("four_pairs", 32, 32, four, [LUMA, CHROMA, (jc.DC_LUMA, jc.AC_CHROMA), (jc.DC_CHROMA, jc.AC_LUMA)], None),
        ("three_pairs_two_scans", 48, 48, y444, [LUMA, CHROMA, LUMA_REVERSED], [[0], [1, 2]]),
    ]
    out = []
    for k, (name, w, h, samp, tables, scans) in enumerate(cases):
        coefs = _coefficients(100 + k, w, h, samp)
        out.append((name, write_scans(w, h, samp, coefs, tables, scans), coefs, samp))
    return out


# ---------------------------------------------------------------------------------------------------------------- long-code streams
# One-component streams over tables whose used symbols have codes of 11 to 16 bits.  AC: the steered writer's table (ss.S_BITS /
# ss.S_VALS): (1,1) (2,1) (1,2) (3,1) (1,3) (4,1) have 10 .. 15 bits and (0,4) has 16; short fillers (0,1) = 00 and (0,2) = 101 move
# the position by 3 and 5 bits.  LONG_AC below gives EOB and ZRL long codes as well.  DC: LONG_DC gives category 3 an 11-bit code.
#   LONG_AC   00 (0,1)   01 (0,10)   100 (0,2)   then one code of every length 4 .. 16: (0,3) (0,5) (0,6) (0,7) (0,8) (0,9) (1,1)
#             | 11 bits EOB   12 bits ZRL   13 bits (1,2)   14 bits (2,1)   15 bits (1,3)   16 bits (0,4)
LONG_AC = ([0, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [0x01, 0x0A, 0x02, 0x03, 0x05, 0x06, 0x07, 0x08, 0x09, 0x11, 0x00, 0xF0, 0x12, 0x21, 0x13, 0x04])
#   LONG_DC   00 cat 0   01 cat 1   10 cat 2   110 cat 4   1110 cat 5 ... and category 3 last, with 11 bits
LONG_DC = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 3])
L_AC, L_DC = jc._codes(*LONG_AC), jc._codes(*LONG_DC)
assert L_AC[0x00][1] == 11 and L_AC[0xF0][1] == 12 and L_AC[0x04][1] == 16 and L_DC[3][1] == 11 and L_AC[0x02] == (4, 3)


class LongCodes:
    """Writes one scan over (LONG_DC, LONG_AC), token by token, and keeps the coefficients it meant.  Positions are bits of the
    destuffed stream (finish() stuffs a byte of eight ones and puts the restart markers in).  cols: blocks per row."""

    def __init__(self, cols, seed, restart_interval=0):
        self.cols, self.ri = cols, restart_interval
        self.rng = np.random.default_rng(seed)
        self.bits = []            # the destuffed stream, one int per bit
        self.markers = []         # bit positions (multiples of 8) in front of which a restart marker goes
        self.blocks = []          # [DC value, {zigzag position: value}]
        self.pred = 0
        self.z = None
        self.placed = []          # (as steered_streams.Steered has it: decode_on_device names it in its messages)

    @property
    def pos(self):
        return len(self.bits)

    def _put(self, value, length):
        self.bits += [(value >> (length - 1 - i)) & 1 for i in range(length)]

    # -- tokens
    def open(self, cat=None):
        assert self.z is None
        if self.ri and self.blocks and len(self.blocks) % self.ri == 0:
            self._put((1 << (-self.pos % 8)) - 1, -self.pos % 8)
            self.markers.append(self.pos)
            self.pred = 0
        if cat is None:
            cat = int(self.rng.choice((0, 1, 2)))
        diff = 0
        if cat:
            mag = int(self.rng.integers(1 << (cat - 1), 1 << cat))
            diff = mag if self.pred <= 0 else -mag
        nb, bits = jc._magnitude(diff)
        self._put(*L_DC[nb])
        if nb:
            self._put(bits, nb)
        self.pred += diff
        self.blocks.append([self.pred, {}])
        self.z = 1

    def coef(self, run, size, value=None):
        """a coefficient of `size` bits behind `run` zeros; value None: a random one whose bits are not all ones"""
        if value is None:
            value = -int(self.rng.integers(1 << (size - 1), 1 << size))   # negative: its first bit is a zero
        nb, bits = jc._magnitude(value)
        assert nb == size and self.z + run <= 63
        code, length = L_AC[(run << 4) | size]
        self._put((code << size) | bits, length + size)
        self.z += run
        self.blocks[-1][1][self.z] = value
        self.z += 1

    def zrl(self):
        assert self.z + 15 <= 63
        self._put(*L_AC[0xF0])
        self.z += 16

    def eob(self):
        if self.z < 64:
            self._put(*L_AC[0x00])
        self.z = None

    # -- fillers: (0,1) costs 3 bits, (0,2) 5 bits; a block break costs 11 (EOB) + 2 (DC category 0)
    def fill_to(self, bit, room=2):
        """short coefficients, and block breaks where a block is full, up to exactly this bit; leaves a block open with room for
        `room` more coefficients"""
        if self.z is None:
            self.open()
        while True:
            r = bit - self.pos
            assert r >= 0, "the position asked for lies behind"
            if r == 0:
                assert self.z <= 63 - room
                return
            # a break costs 13 bits, and up to 7 more where the next block opens a restart interval (padding)
            exact = not (self.ri and len(self.blocks) % self.ri == 0)
            if self.z > 50 - room and ((exact and (r == 13 or r >= 21)) or r >= 28):
                self.eob()
                self.open(0)
                continue
            if r >= 64 and self.z < 30 and self.rng.random() < 0.5:   # far from the target: long codes
                run, size = [(1, 1), (1, 2), (2, 1), (1, 3), (0, 4), (15, 0)][int(self.rng.integers(6))]
                if size:
                    self.coef(run, size)
                else:
                    self.zrl()
                continue
            fits = [n for n in (3, 5) if ss._reachable(r - n)]
            assert fits, "no filler fits: ask for a position further on"
            self.coef(0, {3: 1, 5: 2}[int(self.rng.choice(fits))])

    def damage(self, bit):
        """flips one bit of the stream written so far"""
        self.bits[bit] ^= 1

    def finish(self):
        """closes the open block, completes the last row with empty blocks and returns the file"""
        if self.z is not None:
            self.eob()
        while len(self.blocks) % self.cols:
            self.open(0)
            self.eob()
        self.total_bits = self.pos
        self._put((1 << (-self.pos % 8)) - 1, -self.pos % 8)
        data = bytearray()
        marks, nrst = set(self.markers), 0
        for i in range(0, len(self.bits), 8):
            if i in marks:
                data += bytes([0xFF, 0xD0 + (nrst & 7)])
                nrst += 1
            b = int("".join(map(str, self.bits[i:i + 8])), 2)
            data.append(b)
            if b == 0xFF:
                data.append(0)
        self.scan = bytes(data)
        rows = len(self.blocks) // self.cols
        head = bytearray(b"\xff\xd8")
        head += b"\xff\xdb" + (67).to_bytes(2, "big") + b"\x00" + bytes([4] * 64)
        head += b"\xff\xc0" + (11).to_bytes(2, "big") + b"\x08" + (8 * rows).to_bytes(2, "big") + (8 * self.cols).to_bytes(2, "big") + b"\x01\x01\x11\x00"
        head += _dht(0, 0, LONG_DC) + _dht(1, 0, LONG_AC)
        if self.ri:
            head += b"\xff\xdd" + (4).to_bytes(2, "big") + int(self.ri).to_bytes(2, "big")
        head += b"\xff\xda" + (8).to_bytes(2, "big") + b"\x01\x01\x00\x00\x3f\x00"
        self.header = bytes(head)
        self.jpeg = self.header + self.scan + b"\xff\xd9"
        return self.jpeg

    def coefficients(self):
        out = np.zeros((len(self.blocks), 64), np.int16)
        for b, (dc, ac) in enumerate(self.blocks):
            out[b, 0] = dc
            for z, v in ac.items():
                out[b, jc.ZIGZAG[z]] = v
        return out.reshape(len(self.blocks) // self.cols, self.cols, 64)


# Placements.  SEAM_D: a 16-bit code that starts d bits in front of a subsequence seam -- its first bit alone in front of it, its
# ten first-level bits on either side, the seam between its halves, its six second-level bits on either side.
SEAM_D = (1, 9, 10, 11, 15)
WG_SEAM = 255      # subsequences of a sync workgroup: the seam between two of them is bit 1,024 * 255


@functools.lru_cache(maxsize=None)
def _front(j, ri):
    """the first j - 4 subsequences of the seam files of (j, ri): written once, the files part ways behind them"""
    w = LongCodes(64 if j > 1 else 8, 10 * j + 1000 * ri, ri)
    if j > 4:
        w.fill_to(1024 * (j - 4))
    return w


def _seam(j, d, ri):
    w = copy.copy(_front(j, ri))
    w.bits, w.markers, w.blocks = list(w.bits), list(w.markers), [[dc, dict(ac)] for dc, ac in w.blocks]
    w.rng = np.random.default_rng(10 * j + d + 1000 * ri)
    w.fill_to(1024 * j - d, room=3)
    w.at = w.pos
    w.coef(0, 4)
    w.fill_to(w.pos + 2 * 1024 + 100)
    w.finish()
    return w


def _small(build, seed, ri, cols=8):
    w = LongCodes(cols, seed + 1000 * ri, ri)
    build(w)
    w.finish()
    return w


def _behind_block_end(w):
    w.fill_to(1500)
    w.eob()
    w.open(3)          # the next block's DC symbol: 11 bits
    w.coef(0, 4)       # and its first coefficient: 16
    w.fill_to(w.pos + 2200)


def _eob_at_seam(w):
    w.fill_to(2 * 1024 - 11)
    w.eob()            # the long EOB ends the block on bit 2,048
    assert w.pos == 2048
    w.open()
    w.fill_to(w.pos + 1500)


def _long_dc(w):
    for k in range(40):
        w.fill_to(w.pos + 60 + 7 * k)
        w.eob()
        w.open(3)


def _long_zrl(w):
    for k in range(12):
        w.fill_to(w.pos + 200 + 11 * k, room=50)
        w.eob()
        w.open()
        w.zrl()
        w.zrl()
        w.coef(0, 4)


def _two_in_a_row(w):
    for k in range(12):
        w.fill_to(w.pos + 180 + 13 * k, room=6)
        w.coef(0, 4)
        w.coef(1, 3)
        w.coef(2, 1)


def _last_symbol(padding):
    def build(w):
        w.fill_to(3 * 1024 + 64 - 11 - padding)   # the long EOB is the stream's last symbol; then `padding` ones
    return build


def _damaged(w):
    w.fill_to(1300, room=3)
    at = w.pos
    w.coef(0, 4)
    w.damage(at + 15)   # sixteen ones: the second-level entry behind ten ones that no code owns
    w.fill_to(w.pos + 2500)


@functools.lru_cache(maxsize=None)
def long_code_files():
    """[(name, finished LongCodes, intact)], every placement without and with a restart interval"""
    out = []
    for ri in (0, 5):
        tag = "_rst" if ri else ""
        for j in (1, WG_SEAM):
            for d in SEAM_D:
                out.append(("seam_j%d_d%d%s" % (j, d, tag), _seam(j, d, ri), True))
        out.append(("behind_block_end" + tag, _small(_behind_block_end, 1, ri), True))
        out.append(("eob_at_subsequence_end" + tag, _small(_eob_at_seam, 2, ri), True))
        out.append(("long_dc" + tag, _small(_long_dc, 3, ri), True))
        out.append(("long_zrl" + tag, _small(_long_zrl, 4, ri), True))
        out.append(("two_in_a_row" + tag, _small(_two_in_a_row, 5, ri), True))
        out.append(("last_symbol_on_a_byte" + tag, _small(_last_symbol(0), 6, ri, cols=1), True))
        out.append(("last_symbol_seven_padding_bits" + tag, _small(_last_symbol(7), 7, ri, cols=1), True))
        out.append(("damaged_second_level" + tag, _small(_damaged, 8, ri), False))
    return out
