"""Test helper: coefficient pictures steered onto the seams of the GPU entropy coder's kernels (csrc/gpu_huffman_encode.hip,
csrc/progressive_encode.hip), the way steered_streams.py and progressive_seams.py steer files onto the decoder's.  The coder's write
kernel assembles 256 blocks per workgroup in an LDS window and shares the window's end words with its neighbours; its count / layout /
expand kernels cut the unstuffed bytes into 4096-byte chunks, 16-byte pieces and 64-lane waves and copy dwords plus ragged bytes.  None
of that exists in the host executions of the kernels' code, so a case here states WHERE its bytes land as a predicate over the host
coder's file -- parsed back into scans, and for baseline files modelled bit by bit from the file's own DHT segments -- and the tests
assert the predicate before they compare the GPU's file: a case provably sits on the seam it claims.

Every case is rebuilt from its name alone: a builder is a bounded, deterministic search that calls the host coder per candidate and
returns the first candidate whose predicate holds (LookupError when its try cap runs out; never a near miss).  Plain numpy plus the host
entry points of nvimagecodec_amd.lowlevel; no GPU."""
import collections
import functools
import re

import numpy as np

from helpers.jpeg_from_coefficients import ZIGZAG, write_baseline
from nvimagecodec_amd import lowlevel

# The kernels' constants, restated; (file under nvimagecodec_amd/csrc, the text that sets it).  tests/test_coder_seams.py looks the text up.
UNIT_BLOCKS = 256     # blocks per workgroup of the length / write kernels
WINDOW_WORDS = 4096   # words of the write kernel's LDS window
CHUNK = 4096          # unstuffed bytes per workgroup of the count / expand kernels
PIECE = 16            # bytes per lane of a chunk
WAVE = 64             # lanes whose 0xFF counts one shuffle prefix covers: WAVE * PIECE = 1024 bytes
FILE_ALIGN = 16       # files start at multiples of this in the output arena
SOURCE_TEXT = {
    "UNIT_BLOCKS": [("gpu_huffman_encode.hip", "constexpr int kThreads = %d;" % UNIT_BLOCKS),
                    ("encoder_core.cpp", "b < h.total_blocks; b += %d" % UNIT_BLOCKS), ("encoder_core.cpp", "b < sc.nblocks; b += %d" % UNIT_BLOCKS)],
    "WINDOW_WORDS": [("gpu_huffman_encode.hip", "constexpr int kWindowWords = %d;" % WINDOW_WORDS)],
    "CHUNK": [("gpu_huffman_encode.h", "constexpr int kHencChunk = %d;" % CHUNK)],
    "PIECE": [("gpu_huffman_encode.hip", "chunk * kHencChunk + threadIdx.x * %d;" % PIECE), ("gpu_huffman_encode.hip", "a + t * %d + excl" % PIECE)],
    "WAVE": [("gpu_huffman_encode.hip", "for (int d = 1; d < %d; d <<= 1)" % WAVE), ("gpu_huffman_encode.hip", "if ((t & %d) == %d)" % (WAVE - 1, WAVE - 1))],
    "FILE_ALIGN": [("gpu_huffman_encode.hip", "(flen + %d) & ~%du" % (FILE_ALIGN - 1, FILE_ALIGN - 1)),
                   ("encoder_core.cpp", "align_up(file_bytes, %d)" % FILE_ALIGN)],
}

# Try caps of the builders (candidates per case; every candidate is one call of the host coder)
CAP_SEARCH = 4096   # one predicate over one strip
CAP_COVER = 400     # candidates looked at to collect the 16 combinations of E3

SEAMS = ("W1", "W2", "W3", "W4", "W5", "W6", "S1", "E1", "E2", "E3", "E4", "E5", "E6", "E6b", "E6c", "E7", "E8")

Case = collections.namedtuple("Case", "name seams info coefs params predicate")
Segment = collections.namedtuple("Segment", "start header_bytes data markers ff")
Batch = collections.namedtuple("Batch", "name seams cases")

_NAT = np.array(ZIGZAG)
_ESCAPE = re.compile(rb"\xff[\x00\xd0-\xd7]")
_SCAN_END = re.compile(rb"\xff[^\x00\xd0-\xd7]")


# ---------------------------------------------------------------- the routes
def reference(info, coefs, params):
    return lowlevel.encode_coefficients_host(info, coefs, **params)


def grid_coefficients(info, coefs):
    """The MCU-padded grids [blocks_h][blocks_w][64] (natural order) that the kernel-code-on-host entry points and write_baseline take,
    with libjpeg's dummy blocks (jccoefct.c compress_data): zero AC, the DC of the block coded in front of them in their component."""
    nc = info["num_components"]
    hmax, vmax = max(info["h"]), max(info["v"])
    mx, my = -(-info["width"] // (8 * hmax)), -(-info["height"] // (8 * vmax))
    out = []
    for c in range(nc):
        h, v = (info["h"][c], info["v"][c]) if nc > 1 else (1, 1)
        gh, gw = (my * v, mx * h) if nc > 1 else (info["blocks_h"][c], info["blocks_w"][c])
        g = np.zeros((gh, gw, 64), np.int16)
        rh, rw = info["blocks_h"][c], info["blocks_w"][c]
        g[:rh, :rw] = coefs[c].reshape(rh, rw, 64)
        for y in range(gh):
            for x in range(gw):
                if y < rh and x < rw:
                    continue
                if y < rh or y % v == 0:
                    g[y, x, 0] = g[y, x - 1, 0]  # right edge: the block to the left
                else:
                    g[y, x, 0] = g[y - 1, (x // h) * h + h - 1, 0]  # a dummy row of the MCU: the last block of the MCU's row above
        out.append(g)
    return out


def _sub(info):
    if info["num_components"] == 1:
        return "gray"
    return {(1, 1): "444", (2, 1): "422", (2, 2): "420", (1, 2): "440", (4, 1): "411", (4, 2): "410"}[(info["h"][0], info["v"][0])]


def algorithm_host_files(case):
    """{entry point: file} of every kernel-code-on-host entry point that accepts the case (quantizers all one = quality 100)"""
    info, p = case.info, case.params
    assert all((q == 1).all() for q in info["qtables"])
    grids = grid_coefficients(info, case.coefs)
    args = (info["width"], info["height"], grids, _sub(info), 100)
    out = {}
    if not p["progressive"]:
        out["hipjpegEncodeBaselineGpuAlgorithmHost"] = lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(
            *args, restart_interval=p["restart_interval"], optimized_huffman=p["optimized_huffman"])
    else:
        if not p["restart_interval"]:
            out["hipjpegEncodeFromCoefficientsGpuAlgorithmHost"] = lowlevel.encode_from_coefficients_gpu_algorithm_host(*args)
        out["hipjpegEncodeProgressiveGpuAlgorithmHost"] = lowlevel.encode_from_coefficients_progressive_gpu_algorithm_host(
            *args, restart_interval=p["restart_interval"])
    return out


def entropy_bytes(file):
    """SOS header excluded: from the first scan's first entropy-coded byte to the end of the file"""
    sos = file.index(b"\xff\xda")
    return file[sos + 2 + int.from_bytes(file[sos + 2:sos + 4], "big"):]


def anchor_file(case):
    """The independent writer's file for an Annex-K baseline case (shares no code with the product)"""
    info = case.info
    sampling = list(zip(info["h"], info["v"])) if info["num_components"] > 1 else [(1, 1)]
    grids = [g.astype(np.int32) for g in grid_coefficients(info, case.coefs)]
    return write_baseline(info["width"], info["height"], sampling, grids, [np.ones(64, int)] * len(sampling),
                          restart_interval=case.params["restart_interval"])


# ---------------------------------------------------------------- reading a file back
def parse(file):
    """[Segment] per scan: start (file offset of the segment's header: 0, or the end of the scan in front), header_bytes (up to and
    including the SOS header), data (unstuffed: FF 00 -> FF, RSTn kept), markers (positions in data of the FF of every RSTn; the Dn is the
    byte behind it), ff (positions in data of every 0xFF that is data)."""
    assert file[:2] == b"\xff\xd8"
    segs, pos, start = [], 2, 0
    while True:
        assert file[pos] == 0xFF, pos
        m = file[pos + 1]
        if m == 0xD9:
            assert pos + 2 == len(file)
            return segs
        ln = int.from_bytes(file[pos + 2:pos + 4], "big")
        pos += 2 + ln
        if m != 0xDA:
            continue
        end = _SCAN_END.search(file, pos).start()
        stuffed, out, markers, last = file[pos:end], bytearray(), [], 0
        for e in _ESCAPE.finditer(stuffed):
            out += stuffed[last:e.start()]
            if e.group()[1] == 0:
                out.append(0xFF)
            else:
                markers.append(len(out))
                out += e.group()
            last = e.end()
        out += stuffed[last:]
        data = np.frombuffer(bytes(out), np.uint8)
        markers = np.array(markers, np.int64)
        ff = np.setdiff1d(np.flatnonzero(data == 0xFF), markers)
        assert len(data) + len(ff) == len(stuffed)
        segs.append(Segment(start, pos - start, data, markers, ff))
        pos = start = end


def chunks(seg):
    """[(c, a, n_out, chunk_len)] as henc_expand_kernel sees the segment's chunks: a = misalignment of the chunk's first output byte in
    the file (files start at FILE_ALIGN boundaries), n_out = bytes it writes (data + stuffed zeros)"""
    out = []
    for c in range(-(-len(seg.data) // CHUNK)):
        lo, hi = c * CHUNK, min(len(seg.data), (c + 1) * CHUNK)
        ff_before = int(np.searchsorted(seg.ff, lo))
        ffs = int(np.searchsorted(seg.ff, hi)) - ff_before
        out.append((c, (seg.start + seg.header_bytes + lo + ff_before) % 4, hi - lo + ffs, hi - lo))
    return out


def dht_lengths(file):
    """{(class, id): {symbol: code length}} from the file's DHT segments (the last definition of a slot wins)"""
    tables, pos = {}, 2
    while file[pos + 1] != 0xDA:
        ln = int.from_bytes(file[pos + 2:pos + 4], "big")
        if file[pos + 1] == 0xC4:
            p, end = pos + 4, pos + 2 + ln
            while p < end:
                counts, t, p = file[p + 1:p + 17], {}, p + 17
                slot = (file[p - 17] >> 4, file[p - 17] & 15)
                for length, n in enumerate(counts, 1):
                    for _ in range(n):
                        t[file[p]] = length
                        p += 1
                tables[slot] = t
        pos += 2 + ln
    return tables


def coding_order(info):
    """[(component, block row, block column, real)] in the order of the scan; bpm = blocks per MCU"""
    if info["num_components"] == 1:
        return [(0, y, x, True) for y in range(info["blocks_h"][0]) for x in range(info["blocks_w"][0])], 1
    hmax, vmax = max(info["h"]), max(info["v"])
    mx, my = -(-info["width"] // (8 * hmax)), -(-info["height"] // (8 * vmax))
    order = [(c, yy * info["v"][c] + by, xx * info["h"][c] + bx, None) for yy in range(my) for xx in range(mx)
             for c in range(info["num_components"]) for by in range(info["v"][c]) for bx in range(info["h"][c])]
    return [(c, y, x, y < info["blocks_h"][c] and x < info["blocks_w"][c]) for c, y, x, _ in order], sum(h * v for h, v in zip(info["h"], info["v"]))


class BitModel:
    """Bit lengths and offsets of a baseline file's blocks from its own DHT segments: DC category and code, AC run/size codes and value
    bits, ZRL, EOB; dummy blocks (DC difference 0, no AC); predictor reset, byte alignment and 16 marker bits per restart interval."""

    def __init__(self, file, info, coefs, restart_interval):
        lengths = dht_lengths(file)
        order, bpm = coding_order(info)
        n = self.n = len(order)
        self.rst_blocks = rst = restart_interval * bpm
        self.bits, self.off, self.marker_at = np.zeros(n, np.int64), np.zeros(n, np.int64), []
        pred, run, cache = [0] * info["num_components"], 0, {}
        for i, (c, y, x, real) in enumerate(order):
            if rst and i % rst == 0:
                pred = [0] * info["num_components"]
            dc_len, ac_len = lengths[(0, min(c, 1))], lengths[(1, min(c, 1))]
            if real:
                nat = coefs[c][y, x].reshape(64)
                cat = abs(int(nat[0]) - pred[c]).bit_length()
                pred[c] = int(nat[0])
                key = (min(c, 1), nat[1:].tobytes())
                if key not in cache:
                    cache[key] = self._ac_bits(nat[_NAT], ac_len)
                b = dc_len[cat] + cat + cache[key]
            else:
                b = dc_len[0] + ac_len[0]
            self.off[i], self.bits[i] = run, b
            run += b
            if rst and (i + 1) % rst == 0 and i + 1 < n:  # henc_ends_interval: padding up to a byte, then the marker
                run = (run + 7) // 8 * 8
                self.marker_at.append(run // 8)
                run += 16
        self.total = run

    @staticmethod
    def _ac_bits(zz, ac_len):
        bits, run = 0, 0
        for k in range(1, 64):
            v = int(zz[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits += ac_len[0xF0]
                run -= 16
            s = abs(v).bit_length()
            bits += ac_len[(run << 4) | s] + s
            run = 0
        return bits + (ac_len[0] if run else 0)

    def self_check(self, seg):
        assert (self.total + 7) // 8 == len(seg.data), (self.total, len(seg.data))
        assert list(seg.markers) == self.marker_at
        assert [int(seg.data[p + 1]) for p in seg.markers] == [0xD0 + k % 8 for k in range(len(self.marker_at))]

    def ends_interval(self, i):
        return bool(self.rst_blocks) and (i + 1) % self.rst_blocks == 0 and i + 1 < self.n

    @property
    def groups(self):
        return -(-self.n // UNIT_BLOCKS)

    def group(self, g):
        """(first_bit, end_bit, w0, w1) of workgroup g as henc_write_kernel computes them (gpu_huffman_encode.hip, `if (t == 0)`)"""
        last = min(UNIT_BLOCKS * g + UNIT_BLOCKS, self.n) - 1
        first_bit = int(self.off[UNIT_BLOCKS * g])
        end_bit = int(self.off[last] + self.bits[last]) + (7 if last == self.n - 1 else 0)
        if self.ends_interval(last):
            end_bit = (end_bit + 7) // 8 * 8 + 16
        return first_bit, end_bit, first_bit >> 5, (end_bit - 1) >> 5

    def words(self, g):
        _, _, w0, w1 = self.group(g)
        return w1 - w0 + 1


class View:
    """What a predicate looks at: the reference file of (info, coefs, params), parsed; for baseline files the bit model"""

    def __init__(self, info, coefs, params, file=None):
        self.info, self.coefs, self.params = info, coefs, params
        self.file = file if file is not None else reference(info, coefs, params)

    @functools.cached_property
    def segs(self):
        return parse(self.file)

    @functools.cached_property
    def model(self):
        assert not self.params["progressive"]
        m = BitModel(self.file, self.info, self.coefs, self.params["restart_interval"])
        m.self_check(self.segs[0])
        return m


def view(case):
    return View(case.info, case.coefs, case.params)


# ---------------------------------------------------------------- building blocks
def _block(zz):
    b = np.zeros(64, np.int16)
    b[_NAT] = zz
    return b


def _zz(**at):
    z = np.zeros(64, np.int16)
    for k, v in at.items():
        z[int(k[1:])] = v
    return z


FILLER = _block(np.zeros(64))                       # 6 bits with the Annex-K tables
HEAVY = _block(np.r_[0, np.full(63, 1023)])         # 1640 bits = 205 bytes, more than half of them 0xFF
MEDIUM = _block(np.r_[0, np.ones(63)])              # 191 bits
ONES_END = _block(_zz(k63=1023))                    # no EOB: ends in ten one-bits


def lead(i):
    """The tunable first block: i % 64 small coefficients (3 bits each) and a DC difference that grows with i // 64"""
    z = np.zeros(64, np.int16)
    z[1:1 + i % 64] = 1
    z[0] = 5 * (i // 64)
    return _block(z)


def random_block(rng, count, amplitude):
    z = np.zeros(64, np.int16)
    z[0] = rng.integers(-200, 201)
    z[rng.choice(np.arange(1, 64), size=count, replace=False)] = rng.integers(-amplitude, amplitude + 1, size=count)
    return _block(z)


@functools.lru_cache(maxsize=None)
def _gray_info(n, rows=1):
    assert n % rows == 0
    info = lowlevel.encode_coefficient_info(8 * n // rows, 8 * rows, "gray", 100)
    info["qtables"] = [np.ones(64, np.uint16)]  # (what quality 100 gives: stated, because the other routes are called with quality 100)
    return info


def strip(blocks, rows=1):
    """A gray strip 8n x 8 (or 8n/2 x 16) of the given blocks in coding order"""
    n = len(blocks)
    return _gray_info(n, rows), [np.ascontiguousarray(np.stack(blocks).reshape(rows, n // rows, 8, 8))]


def params(optimized_huffman=False, progressive=False, restart_interval=0):
    return dict(optimized_huffman=optimized_huffman, progressive=progressive, restart_interval=restart_interval)


def search(name, seams, candidate, predicate, cap=CAP_SEARCH, **coding):
    p = params(**coding)
    for i in range(cap):
        info, coefs = candidate(i)
        if predicate(View(info, coefs, p)):
            return Case(name, tuple(seams), info, coefs, p, predicate)
    raise LookupError(f"{name}: no candidate among {cap} reaches the seam")


# ---------------------------------------------------------------- predicates: the write kernel (baseline files, bit model)
def shares_word(m, g):
    """workgroups g and g + 1 share a word"""
    return m.group(g + 1)[2] == m.group(g)[3]


def p_boundary(residue):
    """W1: the first bit of workgroup 1 at `residue` inside a word; the word is shared unless residue == 0"""
    def p(v):
        m = v.model
        return m.groups >= 2 and m.group(1)[0] % 32 == residue and shares_word(m, 0) == (residue != 0)
    return p


def p_group_words(nwords, g=1):
    """W2: workgroup g (behind g - 1, sharing its first word with it) spans exactly nwords words"""
    def p(v):
        m = v.model
        return m.groups > g and m.words(g) == nwords and shares_word(m, g - 1)
    return p


def p_window(nwords):
    """W3: the middle workgroup of three spans exactly nwords words and shares a word with the windowed workgroup on either side"""
    def p(v):
        m = v.model
        return (m.groups == 3 and m.words(1) == nwords and shares_word(m, 0) and shares_word(m, 1) and
                m.words(0) <= WINDOW_WORDS and m.words(2) <= WINDOW_WORDS)
    return p


def p_marker_straddles(v):
    """W4: workgroup 0's last block ends an interval and the marker's 16 bits straddle a word boundary (FF in one word, Dn in the next)"""
    m = v.model
    if m.groups < 2 or not m.ends_interval(UNIT_BLOCKS - 1):
        return False
    end = m.group(0)[1]
    return (end - 16) % 32 == 24 and end == m.group(1)[0]


def p_interval_never_on_boundary(v):
    m = v.model
    return m.groups >= 2 and m.rst_blocks and all(not m.ends_interval(UNIT_BLOCKS * g - 1) for g in range(1, m.groups))


# ---------------------------------------------------------------- predicates: count / layout / expand (any file)
def _any_seg(f):
    return lambda v: any(f(s) for s in v.segs)


def _has(positions, modulus, residue):
    return bool(np.any(positions % modulus == residue))


def p_ff_across_chunks(s):
    """E1: a data 0xFF on a chunk's last byte and on the next chunk's first, in one segment"""
    last = s.ff[s.ff % CHUNK == CHUNK - 1]
    return bool(len(np.intersect1d(last + 1, s.ff)))


def p_ff_piece_and_wave(s):
    """E2: a data 0xFF at piece offsets 15 and 0 and on a wave's last byte"""
    return _has(s.ff, PIECE, PIECE - 1) and _has(s.ff, PIECE, 0) and _has(s.ff, WAVE * PIECE, WAVE * PIECE - 1)


def p_last_chunk(nbytes):
    """E4: more than one chunk, the last of nbytes"""
    return lambda s: len(s.data) > CHUNK and (len(s.data) - 1) % CHUNK + 1 == nbytes


def p_segment_bytes(nbytes, a=None):
    """E4: a whole segment of nbytes (whose first output byte is misaligned by a)"""
    return lambda s: len(s.data) == nbytes and (a is None or chunks(s)[0][1] == a)


def p_ends_in_ff(s):
    """E5: the segment's last unstuffed byte is a data 0xFF"""
    return len(s.ff) and s.ff[-1] == len(s.data) - 1


def p_marker_at(kind):
    """E6: a marker's FF on the last byte of a piece / wave / chunk (and of nothing larger), its Dn on the first of the next"""
    def p(s):
        m = s.markers
        piece, wave, chunk = m % PIECE == PIECE - 1, m % (WAVE * PIECE) == WAVE * PIECE - 1, m % CHUNK == CHUNK - 1
        return bool(np.any({"piece": piece & ~wave, "wave": wave & ~chunk, "chunk": chunk}[kind]))
    return p


def p_ff_before_marker(s):
    """E6b"""
    return bool(len(np.intersect1d(s.ff + 1, s.markers)))


def p_false_marker(s):
    """E6c: data FF followed by a byte D0..D7, in a segment that has real markers"""
    nxt = s.ff[s.ff + 1 < len(s.data)] + 1
    return len(s.markers) > 0 and bool(np.any((s.data[nxt] & 0xF8) == 0xD0))


def ff_share(s):
    """the largest share of data 0xFF among the bytes of one full chunk"""
    full = len(s.data) // CHUNK
    return max((np.count_nonzero(s.ff // CHUNK == c) / CHUNK for c in range(full)), default=0.0)


def p_half_ff(s):
    """E7"""
    return ff_share(s) >= 0.5


def alignment_combinations(v):
    """E3: {(a, n_out % 4)} over the chunks c >= 1 of every segment"""
    return {(a, n_out % 4) for s in v.segs for c, a, n_out, _ in chunks(s) if c >= 1}


# ---------------------------------------------------------------- the cases
def _two_leads(n, near, body=FILLER, tail=8):
    """n blocks of `body` with a tunable block at 0 (i // 64) and at `near` (i % 64), then `tail` more blocks.  The block behind `near`
    has a DC difference of category 3, whose code starts with a one-bit: a boundary in front of it at bit 31 of a word leaves a bit in
    the shared word that is seen when lost."""
    def cand(i):
        blocks = [body] * (n + tail)
        blocks[0], blocks[near], blocks[near + 1] = lead(i // 64), lead(i % 64), _block(_zz(k0=7))
        return strip(blocks)
    return cand


def _heavy_strip(n_heavy, tail=()):
    return lambda i: strip([lead(i)] + [HEAVY] * n_heavy + list(tail))


def _sized_strip(n_heavy, n_medium=0):
    """lead(i % 64), n_heavy heavy blocks and n_medium + i // 64 medium ones: the length moves in steps of 3 and of 191 bits"""
    return lambda i: strip([lead(i % 64)] + [HEAVY] * n_heavy + [MEDIUM] * (n_medium + i // 64))


def _sized_refinement_strip(n_heavy):
    """For progressive output: a block whose first i % 64 coefficients are 1023 and n_heavy + i // 64 heavy blocks.  In the refinement
    scans a coefficient that is already non-zero costs one bit: their length moves in steps of 1 and of about 63 bits."""
    def cand(i):
        z = np.zeros(64, np.int16)
        z[1:1 + i % 64] = 1023
        return strip([_block(z)] + [HEAVY] * (n_heavy + i // 64))
    return cand


def _random_strip(n, count, amplitude, seed, rows=1):
    rng = np.random.default_rng(seed)
    blocks = [random_block(rng, count, amplitude) for _ in range(n)]
    return lambda i: strip([lead(i)] + blocks[1:], rows)


def _reseeded_strip(n, count, amplitude):
    return lambda i: _random_strip(n, count, amplitude, 1000 + i)(0)


def _window_strip(i):
    mid = [lead(i % 64)] + [HEAVY] * 79 + [MEDIUM] * (i // 64) + [FILLER] * (176 - i // 64)
    return strip([lead(1)] + [FILLER] * 255 + mid + [FILLER] * 256)


def _picture_420(seed):
    """166 x 54 at 4:2:0: 11 x 4 MCUs = 264 blocks, luma 21 x 7 real blocks of 22 x 8 -- dummy blocks at the right and the bottom edge"""
    info = lowlevel.encode_coefficient_info(166, 54, "420", 100)
    info["qtables"] = [np.ones(64, np.uint16)] * 3
    rng = np.random.default_rng(seed)
    coefs = [np.ascontiguousarray(np.stack([random_block(rng, 5, 60) for _ in range(bh * bw)]).reshape(bh, bw, 8, 8))
             for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
    return info, coefs


def p_420_boundary_inside_mcu(v):
    order, bpm = coding_order(v.info)
    dummy = [(c, y, x) for c, y, x, real in order if not real]
    return (v.model.groups >= 2 and UNIT_BLOCKS % bpm != 0 and any(x >= v.info["blocks_w"][0] for _, _, x in dummy) and
            any(y >= v.info["blocks_h"][0] for _, y, _ in dummy))


def p_scan_batches(v):
    """S1: the scan kernel's per-lane range is >= 9 blocks, no multiple of its batches of 8, and the last lanes run short"""
    per = -(-v.model.n // UNIT_BLOCKS)
    return per >= 9 and per % 8 != 0 and v.model.n % UNIT_BLOCKS != 0


def _cover_alignments(tag, candidate, cap=CAP_COVER, **coding):
    """E3: cases that together reach all 16 combinations of (a, n_out % 4) on chunks c >= 1; a candidate is kept when it adds one"""
    p, seen, cases = params(**coding), set(), []
    for i in range(cap):
        info, coefs = candidate(i)
        new = alignment_combinations(View(info, coefs, p)) - seen
        if new:
            seen |= new
            want = frozenset(new)
            cases.append(Case(f"{tag}_e3_{len(cases)}", ("E3",), info, coefs, p, lambda v, want=want: want <= alignment_combinations(v)))
        if len(seen) == 16:
            return cases
    raise LookupError(f"{tag}: E3 reached only {sorted(seen)} in {cap} candidates")


def _baseline_cases():
    out = []
    add = lambda *a, **k: out.append(search(*a, **k))
    # --- write kernel
    for rst in (0, 3):
        r = f"_rst{rst}" if rst else ""
        for residue in (1, 31, 0):
            add(f"w1_bit{residue}{r}", ["W1"] + (["W4"] if rst else []), _two_leads(256, 255),
                (lambda v, q=p_boundary(residue), rst=rst: q(v) and (not rst or p_interval_never_on_boundary(v))), restart_interval=rst)
    add("w2_one_word", ["W2", "W5"], _two_leads(256, 255, tail=1), lambda v: v.model.n == 257 and p_group_words(1)(v))
    add("w2_two_words", ["W2"], _two_leads(256, 255, tail=1), p_group_words(2))
    add("w3_window_4096", ["W3"], _window_strip, p_window(WINDOW_WORDS))
    add("w3_through_4097", ["W3"], _window_strip, p_window(WINDOW_WORDS + 1))
    add("w4_marker_straddles_rst64", ["W4"], _two_leads(256, 255), p_marker_straddles, restart_interval=64)
    for n in (1, 255, 256, 257):
        add(f"w5_{n}_blocks", ["W5"], _random_strip(n, 6, 40, 50 + n), lambda v, n=n: v.model.n == n)
    add("w5_420_dummy_blocks", ["W5"], lambda i: _picture_420(7 + i), p_420_boundary_inside_mcu)
    add("w5_420_dummy_blocks_rst2", ["W5"], lambda i: _picture_420(7 + i), p_420_boundary_inside_mcu, restart_interval=2)
    # --- scan kernel
    add("s1_2330_blocks", ["S1"], _random_strip(2330, 4, 30, 61, rows=2), p_scan_batches)
    add("s1_2330_blocks_rst3", ["S1"], _random_strip(2330, 4, 30, 61, rows=2), p_scan_batches, restart_interval=3)
    # --- optimized tables on the same seams (and for the mixed launch, W6)
    add("w1_bit31_optimized", ["W1", "W6"], _two_leads(256, 255), p_boundary(31), optimized_huffman=True)
    add("w5_420_optimized_rst2", ["W5", "W6"], lambda i: _picture_420(7 + i), p_420_boundary_inside_mcu, optimized_huffman=True, restart_interval=2)
    return out


def _expand_cases(tag, progressive):
    """The count / layout / expand seams for baseline (tag "base") or progressive (tag "prog") output"""
    out = []
    kw = dict(progressive=progressive)
    add = lambda name, seams, cand, p, **k: out.append(search(f"{tag}_{name}", seams, cand, p, **dict(kw, **k)))
    rich = _heavy_strip(45) if not progressive else _heavy_strip(1100)
    add("e1_ff_across_chunks", ["E1"], rich, _any_seg(p_ff_across_chunks))
    add("e2_ff_piece_wave", ["E2"], rich, _any_seg(p_ff_piece_and_wave))
    add("e7_half_ff", ["E7"], rich, _any_seg(p_half_ff))
    out.extend(_cover_alignments(tag, _sized_strip(40) if not progressive else _sized_refinement_strip(1040), **kw))
    sized = _sized_strip(19, 8) if not progressive else _sized_refinement_strip(502)
    for nbytes in (1, 2, 3, 15, 16, 17):
        add(f"e4_last_chunk_{nbytes}", ["E4"], sized, _any_seg(p_last_chunk(nbytes)))
    for nbytes in (CHUNK, CHUNK + 1):
        add(f"e4_segment_{nbytes}", ["E4"], _sized_refinement_strip(517) if progressive else sized, _any_seg(p_segment_bytes(nbytes)))
    if progressive:  # scans of an all-zero band and DC refinement bits: tiny segments, at every alignment
        def tiny(i):  # the DC refinement scan is one bit per block; the coefficients of the first block move the scans in front of it
            z = np.zeros(64, np.int16)
            z[1:1 + i % 64] = 7
            return strip([_block(z)] + [FILLER] * (i // 64))
        for nbytes in (1, 2, 3):
            for a in range(4):
                add(f"e4_segment_{nbytes}_a{a}", ["E4"], tiny, _any_seg(p_segment_bytes(nbytes, a)))
    else:  # one block; the header's length is fixed with the Annex-K tables, optimized tables move it
        tiny = lambda i: strip([lead(i)])
        for nbytes in (1, 2, 3):
            add(f"e4_segment_{nbytes}", ["E4"], tiny, _any_seg(p_segment_bytes(nbytes)))
            add(f"e4_segment_{nbytes}_optimized", ["E4", "W6"], tiny, _any_seg(p_segment_bytes(nbytes)), optimized_huffman=True)
    add("e5_ends_in_ff", ["E5"], _heavy_strip(3, [ONES_END]), lambda v: p_ends_in_ff(v.segs[-1]))  # the stuffed zero in front of EOI
    if progressive:  # ... and in front of the next segment's header
        add("e5_inner_segment_ends_in_ff", ["E5"], _heavy_strip(3, [ONES_END]), lambda v: any(p_ends_in_ff(s) for s in v.segs[:-1]))
    # --- restart intervals
    for kind in ("piece", "wave", "chunk"):
        add(f"e6_marker_across_{kind}", ["E6"], _reseeded_strip(1500, 12, 200) if progressive else _random_strip(700, 6, 40, 71),
            _any_seg(p_marker_at(kind)), restart_interval=1)
    add("e6b_ff_before_marker", ["E6b"], lambda i: strip([lead(i)] + [ONES_END] * 41), _any_seg(p_ff_before_marker), restart_interval=2)
    add("e6c_false_marker", ["E6c"], _reseeded_strip(60, 63, 1023), _any_seg(p_false_marker), restart_interval=5)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_baseline_cases() + _expand_cases("base", False) + _expand_cases("prog", True))


def one_block_images(n):
    """E8: n one-block gray images, baseline and progressive alternating (files of one and of several segments)"""
    rng = np.random.default_rng(n)
    out = []
    for k in range(n):
        info, coefs = strip([random_block(rng, int(rng.integers(0, 20)), 300)])
        out.append(Case(f"e8_{n}_{k}", ("E8",), info, coefs, params(progressive=bool(k % 2)), lambda v: len(v.segs) >= 1))
    return out


@functools.lru_cache(maxsize=None)
def batches():
    """Launches whose seam is the mix itself"""
    base = [c for c in cases() if not c.params["progressive"]]
    return (Batch("w6_mixed_baseline_launch", ("W6",), tuple(base)),
            Batch("e8_257_one_block_images", ("E8",), tuple(one_block_images(UNIT_BLOCKS + 1))),
            Batch("e8_513_one_block_images", ("E8",), tuple(one_block_images(2 * UNIT_BLOCKS + 1))))


def p_mixed_launch(batch):
    """W6: Annex-K and optimized tables, with and without a restart interval, in one launch"""
    kinds = {(c.params["optimized_huffman"], bool(c.params["restart_interval"])) for c in batch}
    return kinds == {(False, False), (False, True), (True, False), (True, True)}
