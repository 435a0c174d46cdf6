"""Test helper: progressive (SOF2) files without restart intervals (CASES below; with them: the "interval" option of write_seams and the cases
of progressive_interval_seams.py), written from CHOSEN coefficients like progressive_restart_files.py,
by a coder that also says WHERE everything landed: per scan a log of events (block start, coefficient symbol, run of sixteen, end of
band with its run length, correction bits, DC symbol, DC refinement bit), each with the bit position in the destuffed scan where it starts
and its length in bits -- the coder knows them from its own put() calls, byte stuffing does not change them.  A case states what it is
for as a predicate over that log (CASES below), the tests assert it: the file then provably sits on the seam of the GPU walk
(csrc/progressive_gpu.hip: 64-bit windows, 2,048-bit loads of the word feed, groups of 64 blocks) it was made for, whatever any decoder says.
Beyond progressive_restart_files.py: Huffman tables per scan (DHT segments in front of the scan, ids 0..3), a chosen bound on the correction
bits buffered behind one run symbol, blocks closed by a run of sixteen (ZRL) instead of an end of band -- legal, never written by libjpeg's
coder --, runs cut behind chosen blocks, a declared run longer than the scan.  Plain Python + numpy; at most 640 blocks per component."""
import collections
import functools

import numpy as np

from helpers.jpeg_from_coefficients import DC_CHROMA, DC_LUMA, ZIGZAG, _Bits, _codes, _magnitude, block_grid
from helpers.progressive_restart_files import AC_PROG, _AcCoder

W, C = 64, 2048  # bits of a window of the walk / of a load of its word feed (64 words)

# kind: "block" (arg: True inside an end-of-band run), "coef" (code + value bits, resp. code + sign bit; arg: the coefficient's zigzag
# position), "zrl" (arg: -1, or where it closes the block the zeros that were left), "eob" (code + extra bits; arg: the run length written), "corr" (nbits correction
# bits), "dc" (code + value bits; arg: category), "dcbit"
Ev = collections.namedtuple("Ev", "kind block pos nbits arg")
# bits: before the (last) padding; data: the destuffed bytes, the stream the kernels see (restart markers dropped, the padding in front of
# them kept); starts: where each restart interval starts in that stream, in bits (0 first; ScanHeader::rst_after * 8 behind it); pads: the
# 1-bits between each interval's last symbol and its end; raw_starts: the file offset of each interval's first byte; interval: the scan's
# restart interval (0: none)
Scan = collections.namedtuple("Scan", "entry events bits data starts pads raw_starts interval")


class _LogBits(_Bits):
    def __init__(self):
        super().__init__()
        self.pos = 0
        self.raw = bytearray()  # destuffed

    def put(self, value, length):
        self.pos += length
        n0 = len(self.out)
        super().put(value, length)
        self.raw += bytes(b for i, b in enumerate(self.out[n0:]) if not (b == 0 and i and self.out[n0 + i - 1] == 0xFF))

    def flush(self):
        self.bits = self.pos
        super().flush()


def table_from_lengths(lengths):
    """{symbol: code length} -> (bits, vals), codes assigned in the order given within a length.  No code of ones only (T.81 C)."""
    assert sum(2.0 ** -n for n in lengths.values()) < 1.0
    bits = [sum(1 for n in lengths.values() if n == l) for l in range(1, 17)]
    vals = [s for l in range(1, 17) for s, n in lengths.items() if n == l]
    return bits, vals


def second_level_tables(table):
    """How many 8-bit prefixes of the table's codes continue (the kernels take nine: kProgTableMax = 256 * (1 + 9))."""
    return len({code >> (n - 8) for code, n in _codes(*table).values() if n > 8})


class _SeamCoder(_AcCoder):
    """_AcCoder with the log and the constructs libjpeg's coder never writes."""

    def __init__(self, bw, codes, max_run, events, pending=900, zrl_close=False, cuts=(), declare_last_run=None):
        super().__init__(bw, codes, max_run)
        self.events, self.pending_limit, self.zrl_close, self.cuts, self.declare_last_run = events, pending, zrl_close, set(cuts), declare_last_run
        self.in_run = []  # (block, its correction bits) of the open run, the run's first block first
        self.npending = 0

    def ev(self, kind, block, pos, nbits, arg=None):
        self.events.append(Ev(kind, block, pos, nbits, arg))

    def sym(self, kind, block, symbol, value=0, nvalue=0, arg=None):
        pos = self.bw.pos
        self.bw.put(*self.codes[symbol])
        if nvalue:
            self.bw.put(value, nvalue)
        self.ev(kind, block, pos, self.bw.pos - pos, arg)

    def corr(self, block, bits):
        if bits:
            self.ev("corr", block, self.bw.pos, len(bits))
            for b in bits:
                self.bw.put(b, 1)

    def close_band(self, last=False):
        if self.eobrun:
            run = self.declare_last_run if last and self.declare_last_run else self.eobrun
            assert run >= self.eobrun
            nbits = run.bit_length() - 1
            self.sym("eob", self.in_run[0][0], nbits << 4, run & ((1 << nbits) - 1), nbits, run)
            self.eobrun = 0
        for i, (block, bits) in enumerate(self.in_run):
            if i:
                self.ev("block", block, self.bw.pos, 0, True)
            self.corr(block, bits)
        self.in_run, self.npending = [], 0

    def _closes_by_zrl(self, b):
        return self.zrl_close is True or (self.zrl_close and b in self.zrl_close)

    def _begin(self, b, started):
        """in front of the block's first symbol of its own"""
        self.close_band()
        if not started:
            self.ev("block", b, self.bw.pos, 0, False)
        return True

    def _join_run(self, b, bits, started):
        if self.eobrun == 0 and not started:
            self.ev("block", b, self.bw.pos, 0, False)  # the run's first block: the run symbol will stand here
        assert not (self.eobrun and started)
        self.in_run.append((b, bits))
        self.eobrun += 1
        self.npending += len(bits)
        if self.eobrun >= self.max_run or self.npending > self.pending_limit or b in self.cuts:
            self.close_band()

    def first(self, b, blk, ss, se, al):  # encode_mcu_AC_first
        run, started = 0, False
        for k in range(ss, se + 1):
            val = int(blk[ZIGZAG[k]])
            mag = abs(val) >> al
            if mag == 0:
                run += 1
                continue
            started = self._begin(b, started)
            while run > 15:
                self.sym("zrl", b, 0xF0, arg=-1)
                run -= 16
            nb, bits = _magnitude(mag if val > 0 else -mag)
            assert nb <= 10
            self.sym("coef", b, (run << 4) | nb, bits, nb, k)
            run = 0
        if run and run <= 16 and self._closes_by_zrl(b):  # k += 16 leaves the band: the block is complete without an end of band
            started = self._begin(b, started)
            self.sym("zrl", b, 0xF0, arg=run)
        elif run:
            self._join_run(b, [], started)

    def refine(self, b, blk, ss, se, al):  # encode_mcu_AC_refine
        mags = {k: abs(int(blk[ZIGZAG[k]])) >> al for k in range(ss, se + 1)}
        eob = max([k for k in mags if mags[k] == 1], default=0)
        run, mine, started = 0, [], False
        for k in range(ss, se + 1):
            mag = mags[k]
            if mag == 0:
                run += 1
                continue
            while run > 15 and k <= eob:
                started = self._begin(b, started)
                self.sym("zrl", b, 0xF0, arg=-1)
                run -= 16
                self.corr(b, mine)
                mine = []
            if mag > 1:
                mine.append(mag & 1)
                continue
            started = self._begin(b, started)
            self.sym("coef", b, (run << 4) | 1, 0 if int(blk[ZIGZAG[k]]) < 0 else 1, 1, k)
            self.corr(b, mine)
            mine, run = [], 0
        if run > 0 or mine:
            # `run` zero-history coefficients are left.  A run of sixteen closes the block if it has at most 15 of them (the decoder then
            # corrects up to the band's end) or exactly 16 with the sixteenth on the band's last place
            if self._closes_by_zrl(b) and (run <= 15 or (run == 16 and mags[se] == 0)):
                started = self._begin(b, started)
                self.sym("zrl", b, 0xF0, arg=run)
                self.corr(b, mine)
            else:
                self._join_run(b, mine, started)


def write_seams(width, height, sampling, coefficients, qtables, script, max_run=0x7FFF):
    """script: as write_progressive_restart -- ("dc", [component, ...], ah, al) and ("ac", component, ss, se, ah, al) --, each entry optionally
    followed by a dict of options:
      "dc": {id: (bits, vals)}, "ac": {id: (bits, vals)}   Huffman tables defined in front of this scan (they stay defined, as in any JPEG file)
      "td": [id per scan component], "ta": id              the tables the scan uses (default: 0 for component 0, else 1)
      "pending": n        an end-of-band run is closed once more than n correction bits are buffered behind it (default 900, libjpeg's habit)
      "max_run": n        ... or once it covers n blocks
      "cuts": {block}     ... or behind one of these blocks
      "zrl_close": True or {block}   these blocks end with a run of sixteen instead of an end of band where the tail allows it
      "declare_last_run": n          the run still open at the scan's end is written as n blocks long
      "interval": n       the scan's restart interval (MCUs of an interleaved scan, blocks of a one-component scan): a DRI segment in front of
                          the SOS; in front of every marker the open run and its correction bits are written out, the bits are padded with
                          ones, RSTn counts modulo 8, and the DC predictors start over (as write_progressive_restart does)
      with an interval, two ways to end an interval that a sequential decoder accepts and a lane of the interval kernels must refuse:
      "declare_last_run": {interval: n}   the run still open at the end of that interval is written as n blocks long
      "extra_ones": {interval}            a whole data byte of ones (FF 00 in the file) behind the padding of these intervals
    At the start the file defines DC_LUMA / DC_CHROMA as DC tables 0 / 1 and AC_PROG as AC tables 0 / 1.  No DRI segment unless a scan asks
    for an interval; a scan without the option behind one with it gets a DRI of 0.
    Returns (file, log): log[i] = Scan(entry, events, bits, destuffed bytes, starts, pads, raw_starts, interval) of script[i]; event positions are bit
    positions in the destuffed bytes, padding included."""
    ncomp = len(sampling)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcus_x, mcus_y = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = bytearray(b"\xff\xd8")
    for c in range(ncomp):
        q = [int(qtables[c][ZIGZAG[k]]) for k in range(64)]
        assert all(1 <= x <= 255 for x in q)
        out += b"\xff\xdb" + (67).to_bytes(2, "big") + bytes([c]) + bytes(q)
    out += b"\xff\xc2" + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(sampling):
        out += bytes([c + 1, (h << 4) | v, c])

    def dht(ident, table):
        bits, vals = table
        return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([ident]) + bytes(bits) + bytes(vals)

    dc_tab, ac_tab = {0: DC_LUMA, 1: DC_CHROMA}, {0: AC_PROG, 1: AC_PROG}
    out += dht(0x00, DC_LUMA) + dht(0x10, AC_PROG) + (dht(0x01, DC_CHROMA) + dht(0x11, AC_PROG) if ncomp > 1 else b"")

    def real_blocks(c):
        h, v = sampling[c]
        cw, ch = -(-width * h // hmax), -(-height * v // vmax)
        return -(-cw // 8), -(-ch // 8)

    log, dri = [], 0
    for entry in script:
        opt = entry[-1] if isinstance(entry[-1], dict) else {}
        e = entry[:-1] if opt else entry
        for tid, t in sorted(opt.get("dc", {}).items()):
            out += dht(tid, t)
            dc_tab[tid] = t
        for tid, t in sorted(opt.get("ac", {}).items()):
            out += dht(0x10 | tid, t)
            ac_tab[tid] = t
        interval = int(opt.get("interval", 0))
        if interval != dri:  # (a DRI stays in force, as the tables do)
            out += b"\xff\xdd" + (4).to_bytes(2, "big") + interval.to_bytes(2, "big")
            dri = interval
        declare, extra = opt.get("declare_last_run"), set(opt.get("extra_ones", ()))
        bw, events = _LogBits(), []
        starts, pads, raw_starts = [0], [], []

        def close_interval(last=False):
            """pads the interval that ends here with ones (+ a whole byte of ones where asked for), then the marker"""
            bw.flush()
            if len(pads) in extra:
                bw.put(0xFF, 8)
            pads.append(bw.pos - bw.bits)
            if not last:
                bw.out += bytes([0xFF, 0xD0 + (len(pads) - 1) % 8])
                starts.append(bw.pos)
                raw_starts.append(sos + len(bw.out))

        def declared(i):
            """the run length written for the run open at the end of interval i (None: its own); a plain number is for the scan's end"""
            return declare.get(i) if isinstance(declare, dict) else declare if i is None else None

        if e[0] == "dc":
            comps = list(e[1])
            ah, al = (e[2], e[3]) if len(e) > 2 else (0, 0)
            td = opt.get("td", [0 if c == 0 else 1 for c in comps])
            out += b"\xff\xda" + (6 + 2 * len(comps)).to_bytes(2, "big") + bytes([len(comps)])
            for c, t in zip(comps, td):
                out += bytes([c + 1, t << 4])
            out += bytes([0, 0, (ah << 4) | al])
            sos = len(out)
            raw_starts.append(sos)
            codes = {c: _codes(*dc_tab[t]) for c, t in zip(comps, td)}
            if len(comps) == 1:
                nbx, nby = real_blocks(comps[0])
                units = [[(comps[0], y, x)] for y in range(nby) for x in range(nbx)]
            else:
                units = [[(c, my * sampling[c][1] + by, mx * sampling[c][0] + bx) for c in comps for by in range(sampling[c][1]) for bx in range(sampling[c][0])]
                         for my in range(mcus_y) for mx in range(mcus_x)]
            pred, b = {}, 0
            for m, unit in enumerate(units):
                if interval and m and m % interval == 0:
                    close_interval()
                    pred = {}
                for c, y, x in unit:
                    v = int(coefficients[c][y][x][0])
                    b += 1
                    if ah:
                        events.append(Ev("dcbit", b - 1, bw.pos, 1, (v >> al) & 1))
                        bw.put((v >> al) & 1, 1)
                        continue
                    v >>= al
                    nb, bits = _magnitude(v - pred.get(c, 0))
                    pred[c] = v
                    assert nb <= 11
                    pos = bw.pos
                    bw.put(*codes[c][nb])
                    if nb:
                        bw.put(bits, nb)
                    events.append(Ev("dc", b - 1, pos, bw.pos - pos, nb))
        else:
            c, ss, se = e[1], e[2], e[3]
            ah, al = (e[4], e[5]) if len(e) > 4 else (0, 0)
            assert 1 <= ss <= se <= 63
            ta = opt.get("ta", 0 if c == 0 else 1)
            out += b"\xff\xda" + (8).to_bytes(2, "big") + bytes([1, c + 1, ((ta & 1) << 4) | ta, ss, se, (ah << 4) | al])  # (the DC selector means nothing here)
            sos = len(out)
            raw_starts.append(sos)
            nbx, nby = real_blocks(c)
            coder = _SeamCoder(bw, _codes(*ac_tab[ta]), opt.get("max_run", max_run), events, opt.get("pending", 900), opt.get("zrl_close", False),
                               opt.get("cuts", ()), declared(None))
            for b in range(nbx * nby):
                if interval and b and b % interval == 0:
                    coder.declare_last_run = declared(len(pads))
                    coder.close_band(last=True)
                    close_interval()
                (coder.refine if ah else coder.first)(b, coefficients[c][b // nbx][b % nbx], ss, se, al)
            coder.declare_last_run = declared(len(pads)) if isinstance(declare, dict) else declared(None)
            coder.close_band(last=True)
        close_interval(last=True)
        out += bw.out
        log.append(Scan(e, events, bw.bits, bytes(bw.raw), tuple(starts), tuple(pads), tuple(raw_starts), interval))
    out += b"\xff\xd9"
    return bytes(out), log


# ---------------------------------------------------------------------------------------------------------------- what a predicate asks
def off(ev):
    return ev.pos % W


def ends(ev):
    return ev.pos + ev.nbits


def starts_at_63(ev):
    return off(ev) == 63


def ends_at_64(ev):
    return ends(ev) % W == 0


def straddles(ev):
    return off(ev) + ev.nbits > W


def at_chunk_end(ev, chunk):
    """a code that starts in the second half of the last window of 2,048-bit load `chunk`: its bits need word 0 of the next load"""
    return (chunk + 1) * C - 32 <= ev.pos < (chunk + 1) * C


def symbols(scan):
    return [ev for ev in scan.events if ev.kind in ("coef", "zrl", "eob", "dc")]


def find(scan, kind, block=None, **kw):
    return [ev for ev in scan.events if ev.kind == kind and (block is None or ev.block == block) and all(getattr(ev, k) == v for k, v in kw.items())]


# ---------------------------------------------------------------------------------------------------------------- the cases
GRAY = [(1, 1)]
S420 = [(2, 2), (1, 1), (1, 1)]
S444 = [(1, 1)] * 3
CMYK = [(1, 1)] * 4
Case = collections.namedtuple("Case", "name jpeg coefs log sampling width height in_limit")
CASES = {}  # name -> function() -> Case (cached)
_FIRST = [("dc", [0]), ("ac", 0, 1, 63, 0, 0)]
_REFINE = [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0)]


def blank(width, height, sampling=GRAY):
    return [np.zeros((bh, bwid, 64), dtype=np.int32) for bh, bwid in block_grid(width, height, sampling)]


def setk(a, b, k, v):
    """coefficient at zigzag position k of block b (raster order) of one component's array"""
    a[b // a.shape[1], b % a.shape[1], ZIGZAG[k]] = v


def _qt(n):
    return [np.full(64, 2 + c, dtype=np.int32) for c in range(n)]


def case(name, in_limit=True):
    def deco(fn):
        @functools.lru_cache(maxsize=None)
        def make():
            width, height, sampling, coefs, script, check = fn()
            jpeg, log = write_seams(width, height, sampling, coefs, _qt(len(sampling)), script)
            return Case(name, jpeg, coefs, log, sampling, width, height, in_limit), check
        CASES[name] = make
        return make
    return deco


def steered(name, tries, in_limit=True):
    """fn(shift) -> (width, height, sampling, coefs, script, check): the first shift in `tries` whose file meets check(log) is the case"""
    def deco(fn):
        @functools.lru_cache(maxsize=None)
        def make():
            for shift in tries:
                width, height, sampling, coefs, script, check = fn(shift)
                jpeg, log = write_seams(width, height, sampling, coefs, _qt(len(sampling)), script)
                if check(log):
                    return Case(name, jpeg, coefs, log, sampling, width, height, in_limit), check
            raise AssertionError("no filler puts %s on its seam" % name)
        CASES[name] = make
        return make
    return deco


def first_filler(a, b, extra):
    """block b of a first scan: 16 coefficients of 8 bits each with AC_PROG (7-bit code, size 1), `extra` more bits (<= 64) by larger sizes"""
    for k in range(1, 17):
        s = 1 + min(4, extra)
        extra -= s - 1
        setk(a, b, k, (1 << s) - 1 if k % 2 else -(1 << (s - 1)))
    assert extra == 0


def refine_filler(a, b, shift):
    """block b in front of the event of a refinement scan with ah = 1: shift % 63 non-zero-history coefficients (a correction bit each), and
    for shift >= 63 a new coefficient at place 63 (8 more bits with AC_PROG, and no end of band).  Any offset in a window can be reached."""
    for k in range(1, shift % 63 + 1):
        setk(a, b, k, (2 + (k & 1)) * (1 if k % 3 else -1))
    if shift >= 63:
        setk(a, b, 63, 1)


# -- window seams: every event kind starts at offset 63 of a window / ends exactly at offset 64 / straddles the window's end.
# First scans: block 0 is the filler, block 1 holds the event, block 2 a coefficient (so that runs end where they should).
def _event_blocks(a, kind, refine):
    """-> (kind of the event in the log, its block)"""
    v = 1 if refine else 5
    if kind == "coef":
        setk(a, 1, 3, v)
        return "coef", 1
    if kind == "eob":  # a run of one block
        setk(a, 1, 2, -v)
        setk(a, 2, 1, v)
        return "eob", 1
    if kind == "eobrun":  # blocks 1..3: EOB1 and one extra bit
        setk(a, 1, 2, v)
        setk(a, 4, 1, -v)
        return "eob", 1
    if kind == "zrl":
        setk(a, 1, 20, v)
        setk(a, 2, 1, v)
        return "zrl", 1
    assert kind == "last"  # a coefficient at se: the band is complete, no end of band follows
    setk(a, 1, 63, -v)
    setk(a, 2, 1, v)
    return "coef", 1


for _refine in (False, True):
    for _kind in ("coef", "eob", "eobrun", "zrl", "last"):
        for _cond in (starts_at_63, ends_at_64, straddles):
            def _window_case(shift, refine=_refine, kind=_kind, cond=_cond):
                a = blank(48, 8)
                if refine:
                    refine_filler(a[0], 0, shift)
                else:
                    first_filler(a[0], 0, shift)
                what, blk = _event_blocks(a[0], kind, refine)

                def check(log, what=what, blk=blk):
                    evs = find(log[-1], what, blk)
                    return len(evs) == 1 and cond(evs[0]) and (kind != "eobrun" or evs[0].arg in (2, 3)) and \
                        (kind != "last" or (evs[0].arg == 63 and not find(log[-1], "eob", blk)))
                return 48, 8, GRAY, a, _REFINE if refine else _FIRST, check
            steered("window_%s_%s_%s" % ("refine" if _refine else "first", _kind, _cond.__name__), range(0, 126 if _refine else 65))(_window_case)


# EOB14 with a 16-bit code and extra bits of ones: 30 bits, the run length is read from the 32 bits behind the symbol's start
AC_LONG_EOB14 = table_from_lengths({0x00: 2, 0x01: 3, 0x02: 4, 0x03: 5, 0x04: 6, 0x05: 7, 0x11: 8, 0xF0: 9, 0xE0: 16})


@steered("window_eob14_16bit_code_run_32767", range(0, 65))
def _eob14(shift):
    a = blank(48, 8)
    first_filler(a[0], 0, shift)
    setk(a[0], 1, 1, 3)  # blocks 1..5: the run, declared as 32,767 blocks and cut by the scan's end

    def check(log):
        evs = find(log[1], "eob", 1)
        return len(evs) == 1 and evs[0].arg == 32767 and evs[0].nbits == 30 and off(evs[0]) >= 35
    return 48, 8, GRAY, a, [("dc", [0]), ("ac", 0, 1, 63, 0, 0, {"ac": {0: AC_LONG_EOB14}, "declare_last_run": 32767})], check


# a refinement symbol of 70 bits and more that starts late in a window: the position passes over a whole window in one step
AC_LONG_NEW = table_from_lengths({0x00: 1, 0x11: 2, 0x21: 3, 0xF0: 4, 0x10: 5, 0x20: 6, 0x01: 16})


@steered("window_refine_symbol_of_70_bits_at_60", range(0, 126))
def _long70(shift):
    a = blank(48, 8)
    refine_filler(a[0], 0, shift)
    for k in range(1, 63):
        setk(a[0], 1, k, 2 + (k % 3 == 0))
    setk(a[0], 1, 63, -1)
    setk(a[0], 2, 5, 1)

    def check(log):
        ev = find(log[2], "coef", 1)[0]
        corr = [c for c in find(log[2], "corr", 1) if c.pos == ends(ev)]
        return len(corr) == 1 and ev.nbits + corr[0].nbits >= 70 and off(ev) >= 60 and (ev.pos + ev.nbits + corr[0].nbits) // W >= ev.pos // W + 2
    return 48, 8, GRAY, a, _REFINE, check


@steered("window_refine_16bit_code_78_bits_at_60", range(0, 63))
def _long78(shift):
    a = blank(48, 8)
    refine_filler(a[0], 0, shift)
    for k in range(1, 62):
        setk(a[0], 1, k, -2 - (k % 3 == 0))
    setk(a[0], 1, 62, 1)  # 16-bit code, sign, 61 correction bits; place 63 stays zero: an end of band follows
    setk(a[0], 2, 2, 1)

    def check(log):
        ev = find(log[2], "coef", 1)[0]
        corr = [c for c in find(log[2], "corr", 1) if c.pos == ends(ev)]
        return ev.nbits == 17 and corr[0].nbits == 61 and off(ev) >= 60 and len(find(log[2], "eob", 1)) == 1
    return 48, 8, GRAY, a, [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0, {"ac": {0: AC_LONG_NEW}})], check


# -- chunk seams: a code starts in the second half of the last window of load 0 and of load 1; the scan is longer than three loads
def _dense(rng, nblocks_x, nblocks_y, per_block, small, refine_share=0.0):
    a = blank(8 * nblocks_x, 8 * nblocks_y)
    for b in range(nblocks_x * nblocks_y):
        for k in rng.choice(np.arange(1, 64), size=per_block, replace=False):
            v = 1 if rng.random() < refine_share else int(rng.integers(2, small + 1))
            setk(a[0], b, int(k), v if rng.random() < 0.5 else -v)
    return a


for _refine in (False, True):
    def _chunk_case(seed, refine=_refine):
        rng = np.random.default_rng(seed)
        a = _dense(rng, 10, 6, 24, 30, 0.5 if refine else 0.0)

        def check(log):
            s = log[-1]
            return s.bits > 3 * C and all(any(at_chunk_end(ev, ch) for ev in symbols(s)) for ch in (0, 1))
        return 80, 48, GRAY, a, _REFINE if refine else _FIRST, check
    steered("chunk_end_%s" % ("refine" if _refine else "first"), range(20))(_chunk_case)


# -- run skips: one end-of-band run of a refinement scan, 60 correction bits per block, then a new coefficient off a window's start
def _run_skip(name, nrun, cond):
    def fn(shift):
        n = nrun + 2
        a = blank(8 * n, 8)
        refine_filler(a[0], 0, shift)
        setk(a[0], 0, 63, -1)  # block 0 completes its band: the run starts with block 1
        for b in range(1, nrun + 1):
            for k in range(1, 61):
                setk(a[0], b, k, (2 + ((b + k) % 2)) * (-1 if k % 3 else 1))
        setk(a[0], nrun + 1, 1, 1)

        def check(log):
            s = log[2]
            run, new = find(s, "eob", 1), find(s, "coef", nrun + 1)
            if len(run) != 1 or run[0].arg != nrun or len(new) != 1:
                return False
            return new[0].pos - ends(run[0]) == 60 * nrun and off(new[0]) != 0 and cond(run[0], new[0])
        return 8 * n, 8, GRAY, a, [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0, {"pending": 1 << 20})], check
    steered(name, range(0, 8))(fn)


_run_skip("run_skip_windows_inside_a_chunk", 10, lambda run, new: run.pos // C == new.pos // C and 2 <= new.pos // W - run.pos // W <= 31)
_run_skip("run_skip_across_a_chunk_end", 40, lambda run, new: new.pos // C == run.pos // C + 1 and new.pos // 32 - run.pos // 32 < 128)
_run_skip("run_skip_4096_bits", 70, lambda run, new: 4096 <= new.pos - ends(run) < 8192 and new.pos // 32 >= 128)
_run_skip("run_skip_8192_bits", 140, lambda run, new: new.pos - ends(run) >= 8192)


# -- stream ends
for _rem in range(4):
    def _len_case(shift, rem=_rem):
        a = blank(48, 8)
        first_filler(a[0], 0, shift)
        setk(a[0], 3, 7, -9)
        return 48, 8, GRAY, a, _FIRST, lambda log: len(log[1].data) % 4 == rem and len(log[1].data) >= 8
    steered("stream_length_4k_plus_%d" % _rem, range(0, 65))(_len_case)

for _pad in (0, 7):
    def _pad_case(shift, pad=_pad):
        a = blank(48, 8)
        first_filler(a[0], 0, shift)
        setk(a[0], 5, 63, 77)  # the last block's last symbol completes the band: the scan's last bit is a value bit
        return 48, 8, GRAY, a, _FIRST, lambda log: (-log[1].bits) % 8 == pad and max(ends(e) for e in log[1].events) == log[1].bits
    steered("stream_ends_with_%d_padding_bits" % _pad, range(0, 65))(_pad_case)


@case("stream_of_fewer_than_8_bytes")
def _short():
    a = blank(16, 8)
    setk(a[0], 0, 1, 3)
    setk(a[0], 1, 2, -1)
    return 16, 8, GRAY, a, _REFINE, lambda log: all(0 < len(s.data) < 8 for s in log)


@case("stream_of_ff_bytes")
def _ones():
    """the DC refinement scan is FF bytes only, the AC refinement scan has 300 correction bits of ones behind each other"""
    a = blank(40, 40)
    a[0][..., 0] = 1
    for b in range(5):
        for k in range(1, 61):
            setk(a[0], b, k, 3)
    setk(a[0], 5, 1, 1)

    def check(log):
        return set(log[3].data) == {0xFF} and len(log[3].data) == 4 and b"\xff" * 37 in log[2].data
    return 40, 40, GRAY, a, [("dc", [0], 0, 1), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0, {"pending": 1 << 20}), ("dc", [0], 1, 0)], check


# -- group seams: N x 1 blocks; ONE end-of-band run, every other block completes its band with a coefficient at place 63.
#    N -> (the run's first block, its last)
GROUP_RUNS = {63: (40, 62), 64: (10, 63), 65: (20, 63), 128: (63, 127), 129: (63, 128), 192: (63, 128)}
for _refine in (False, True):
    for _n, (_b0, _b1) in GROUP_RUNS.items():
        def _group_case(n=_n, b0=_b0, b1=_b1, refine=_refine):
            a = blank(8 * n, 8)
            for b in range(n):
                if refine:
                    for k in range(10, 15):  # five correction bits in every block, the ones inside the run included
                        setk(a[0], b, k, (2 + (b + k) % 2) * (1 if (b + k) % 3 else -1))
                if b < b0 or b > b1:
                    setk(a[0], b, 1 + b % 5, -1 if refine else 3 + b % 9)
                    setk(a[0], b, 63, 1 if refine else -2)
            setk(a[0], b0, 3, 1 if refine else 6)  # the run's first block has a coefficient of its own

            def check(log):
                s = log[-1]
                run, inside = find(s, "eob"), [ev for ev in find(s, "block") if ev.arg]
                return len(run) == 1 and run[0].block == b0 and run[0].arg == b1 - b0 + 1 and [ev.block for ev in inside] == list(range(b0 + 1, b1 + 1)) and \
                    (not refine or all(len(find(s, "corr", b, nbits=5)) == 1 for b in range(b0, b1 + 1)))
            return 8 * n, 8, GRAY, a, _REFINE if refine else _FIRST, check
        case("group_%s_%d_blocks_run_%d_to_%d" % ("refine" if _refine else "first", _n, _b0, _b1))(_group_case)


# -- rings: 640 blocks, six AC scans; the stages of the pipeline run at very different speeds over ten groups
_RING_SCRIPT = [("ac", 0, 1, 63, 0, 5, {"pending": 1 << 20})] + [("ac", 0, 1, 63, ah, ah - 1, {"pending": 1 << 20}) for ah in (5, 4, 3, 2, 1)]
RING_CASES = []
for _heavy in ("front", "back"):
    for _colour in (False, True):
        def _ring_case(heavy=_heavy, colour=_colour):
            rng = np.random.default_rng(len(heavy) + colour)
            samp = S420 if colour else GRAY
            a = blank(640, 64, samp)
            mags = rng.integers(32, 64, size=(8, 80, 64)) if heavy == "front" else np.ones((8, 80, 64), dtype=np.int64)
            a[0][...] = mags * rng.choice([-1, 1], size=mags.shape)
            a[0][..., 0] = rng.integers(-30, 30, size=(8, 80))
            script = [("dc", [0, 1, 2] if colour else [0])] + _RING_SCRIPT
            for c in range(1, len(samp)):
                a[c][...] = rng.integers(-3, 4, size=a[c].shape) * (rng.random(a[c].shape) < 0.2)
                script += [("ac", c, 1, 63, 0, 1), ("ac", c, 1, 63, 1, 0)]

            def check(log):
                dense, runs = (log[1], log[2:7]) if heavy == "front" else (log[6], log[1:6])
                if len(find(dense, "coef")) != 640 * 63 or find(dense, "eob"):
                    return False
                for s in runs:  # one run over all ten groups, in the refinement scans of "front" with 63 correction bits per block
                    run = find(s, "eob")
                    if len(run) != 1 or run[0].arg != 640 or find(s, "coef") or sum(ev.nbits for ev in find(s, "corr")) != (640 * 63 if heavy == "front" else 0):
                        return False
                return True
            return 640, 64, samp, a, script, check
        RING_CASES.append("ring_%s_heavy_%s" % (_heavy, "420" if _colour else "gray"))
        case(RING_CASES[-1])(_ring_case)


# -- blocks closed by a run of sixteen
def _random_gray(seed, width, height, dense, small=3):
    from helpers.jpeg_from_coefficients import random_coefficients
    return random_coefficients(np.random.default_rng(seed), width, height, GRAY, 5, dense=dense, small=small, dc=30)


@case("zrl_closes_blocks_of_first_and_refinement_scans")
def _zrl_random():
    a = _random_gray(5, 200, 160, 9)
    z = {"zrl_close": True}

    def check(log):
        first = [ev.arg for ev in find(log[1], "zrl") if ev.arg >= 0]
        refine = [ev.arg for s in log[2:] for ev in find(s, "zrl") if ev.arg >= 0]
        return first.count(16) >= 10 and sum(1 for r in first if r < 16) >= 50 and sum(1 for r in refine if r <= 15) >= 100 and refine.count(0) >= 1
    return 200, 160, GRAY, a, [("dc", [0]), ("ac", 0, 1, 63, 0, 2, z), ("ac", 0, 1, 63, 2, 1, z), ("ac", 0, 1, 63, 1, 0, z)], check


@case("zrl_closes_a_refinement_tail_of_exactly_16")
def _zrl_16():
    """behind the last new coefficient: n non-zero-history coefficients mixed with exactly 16 zero-history ones, the last of them at place 63"""
    a = blank(64, 8)
    for b in range(8):
        new = 63 - 16 - b
        setk(a[0], b, new, 1 if b % 2 else -1)
        hist = list(range(new + 1, 63))[::2][:b] if b % 2 else list(range(new + 1, new + 1 + b))
        for k in hist:
            setk(a[0], b, k, 2 + k % 2)
        if b >= 4:
            setk(a[0], b, 2, -3)

    def check(log):
        z = find(log[2], "zrl")
        return [ev.arg for ev in z if ev.arg >= 0] == [16] * 8 and not find(log[2], "eob") and sum(ev.nbits for ev in find(log[2], "corr")) == sum(range(8)) + 4
    return 64, 8, GRAY, a, [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0, {"zrl_close": True})], check


@case("zrl_bands_of_one_place_and_bands_ending_at_62_and_63")
def _zrl_bands():
    a = _random_gray(11, 96, 80, 14)
    z = {"zrl_close": True}
    script = [("dc", [0]), ("ac", 0, 1, 4, 0, 0, z), ("ac", 0, 5, 5, 0, 1, z), ("ac", 0, 6, 62, 0, 1, z), ("ac", 0, 63, 63, 0, 0, z), ("ac", 0, 5, 5, 1, 0, z),
              ("ac", 0, 6, 62, 1, 0, z)]

    def check(log):
        closing = [sum(1 for ev in find(s, "zrl") if ev.arg >= 0) for s in log[1:]]
        return all(n > 0 for n in closing) and all(find(s, "coef") for s in log[1:])
    return 96, 80, GRAY, a, script, check


@case("zrl_and_runs_over_blocks_with_all_63_places_in_the_history")
def _full_history():
    a = blank(80, 8)
    for b in (1, 4, 6, 8):
        for k in range(1, 64):
            setk(a[0], b, k, (2 + (b + k) % 2) * (1 if k % 3 else -1))
    for b in (0, 2, 5, 7, 9):
        setk(a[0], b, 7 + b, 1)
        setk(a[0], b, 63, -1)  # (these blocks complete their band: no end of band of theirs opens a run)
    setk(a[0], 3, 9, 3)  # block 3 starts the run that block 4 lies in

    def check(log):
        s = log[2]
        alone, inside, by_zrl = find(s, "eob", 1), [ev for ev in find(s, "block", 4) if ev.arg], find(s, "zrl", 6)
        return len(alone) == 1 and alone[0].arg == 1 and len(inside) == 1 and len(find(s, "eob", 3, arg=2)) == 1 and len(by_zrl) == 1 and by_zrl[0].arg == 0 and \
            all(len(find(s, "corr", b, nbits=63)) == 1 for b in (1, 4, 6, 8))
    return 80, 8, GRAY, a, [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0, {"zrl_close": {6}})], check


# -- DC scans
DC_T2 = table_from_lengths({0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 4, 7: 5, 8: 6, 9: 7, 10: 8, 11: 9})
DC_T3 = table_from_lengths({5: 2, 4: 3, 3: 3, 6: 4, 2: 4, 1: 5, 0: 5, 7: 6, 8: 7, 9: 8, 10: 9, 11: 10})
DC_16 = table_from_lengths({0: 2, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 16, 9: 16, 10: 16, 11: 16})


def _with_ac(rng, a, script, share=0.1):
    """a few AC coefficients and one AC scan per component, so that every component has a chain to replay"""
    for c, arr in enumerate(a):
        ac = rng.integers(-4, 5, size=arr.shape) * (rng.random(arr.shape) < share)
        ac[..., 0] = 0
        arr += ac
        script.append(("ac", c, 1, 63, 0, 0))
    return script


for _name, _td in (("four_tables", [0, 1, 2, 3]), ("two_tables_shared_0_2_and_1_3", [0, 1, 0, 1])):
    def _dc4(td=_td):
        rng = np.random.default_rng(7)
        a = blank(72, 40, CMYK)
        for arr in a:
            arr[..., 0] = rng.integers(-900, 900, size=arr.shape[:2])
        script = _with_ac(rng, a, [("dc", [0, 1, 2, 3], 0, 0, {"dc": {2: DC_T2, 3: DC_T3}, "td": td})])

        def check(log):
            return len(log[0].events) == 4 * 45 and log[0].entry[1] == [0, 1, 2, 3]
        return 72, 40, CMYK, a, script, check
    case("dc_four_components_" + _name)(_dc4)


@steered("dc_16bit_codes_category_11_straddles_a_window", range(200))
def _dc16(seed):
    rng = np.random.default_rng(seed)
    a = blank(8 * 70, 8)
    v = rng.integers(-100, 100, size=70)
    v[10:14] = [1023, -1000, 500, -700]  # differences of category 11 with either sign, 10 and 11
    v[40:44] = [-1024, 1020, -900, 1000]
    a[0][0, :, 0] = v
    script = _with_ac(rng, a, [("dc", [0], 0, 0, {"dc": {0: DC_16}})])

    def check(log):
        long = [ev for ev in log[0].events if ev.nbits == 27]
        signs = {int(np.sign(v[ev.block] - v[ev.block - 1])) for ev in long}
        return signs == {-1, 1} and any(straddles(ev) for ev in long) and second_level_tables(DC_16) == 1
    return 8 * 70, 8, GRAY, a, script, check


S_MCU10 = [(2, 2), (2, 1), (2, 2)]
for _name, _samp, _w, _h in (("mcu_of_3_one_wide_70_tall", S444, 8, 560), ("mcu_of_6_one_wide_66_tall", S420, 16, 1056), ("mcu_of_6_66_wide", S420, 1056, 16),
                             ("mcu_of_10", S_MCU10, 80, 48), ("mcu_of_10_66_wide", S_MCU10, 1056, 16)):
    def _dc_mcu(samp=_samp, w=_w, h=_h):
        rng = np.random.default_rng(w + h)
        a = blank(w, h, samp)
        for arr in a:
            arr[..., 0] = rng.integers(-200, 200, size=arr.shape[:2])
        script = _with_ac(rng, a, [("dc", [0, 1, 2], 0, 1), ("dc", [0, 1, 2], 1, 0)], 0.05)
        mcus = (-(-w // (8 * samp[0][0]))) * (-(-h // (8 * samp[0][1])))

        def check(log):
            return len(log[0].events) == mcus * sum(hh * vv for hh, vv in samp) == len(log[1].events)
        return w, h, samp, a, script, check
    case("dc_" + _name)(_dc_mcu)

for _n in (63, 64, 65, 95):
    def _dc_blocks(n=_n):
        """n blocks in the DC first scan and in its two refinement scans (n = 32 k, 32 k + 1, 32 k + 31), al = 1 on negative values, the last
        block's bit set in both"""
        rng = np.random.default_rng(n)
        a = blank(8 * n, 8)
        v = rng.integers(-300, 300, size=n)
        v[::2] = -np.abs(v[::2]) - 1
        v[-1] = -5 if n % 2 else 7  # bits 1 and 0 set (two's complement of -5: ...1011)
        a[0][0, :, 0] = v
        script = _with_ac(rng, a, [("dc", [0], 0, 2), ("dc", [0], 2, 1), ("dc", [0], 1, 0)])

        def check(log):
            return all(len(s.events) == n for s in log[:3]) and log[1].events[-1].arg == 1 and log[2].events[-1].arg == 1 and (v < 0).sum() >= n // 2
        return 8 * n, 8, GRAY, a, script, check
    case("dc_%d_blocks_refined_twice" % _n)(_dc_blocks)


# -- the limits of the GPU path, a file on either side
def _bit_planes(c, top):
    """AC scans of component c: the whole band with al = top, refined down to al = 0 -- top + 1 scans"""
    return [("ac", c, 1, 63, 0, top)] + [("ac", c, 1, 63, ah, ah - 1) for ah in range(top, 0, -1)]


def _limit_case(name, in_limit, samp, script_of, check):
    def fn():
        rng = np.random.default_rng(len(name))
        a = blank(40, 24, samp)
        for arr in a:
            arr[...] = rng.integers(-200, 200, size=arr.shape) * (rng.random(arr.shape) < 0.3)
        script = script_of()
        return 40, 24, samp, a, script, lambda log: check([s.entry for s in log])
    case(name, in_limit)(fn)


def _ac_scans(entries, c=None):
    return sum(1 for e in entries if e[0] == "ac" and (c is None or e[1] == c))


_limit_case("limit_6_stages", True, GRAY, lambda: [("dc", [0])] + _bit_planes(0, 5), lambda es: _ac_scans(es, 0) == 6)
_limit_case("limit_7_stages", False, GRAY, lambda: [("dc", [0])] + _bit_planes(0, 6), lambda es: _ac_scans(es, 0) == 7)
# 15 AC scans is also the largest launch of the walk: 16 waves, 4 + 15 table slots of 2,560 entries (AC_PROG has nine second-level tables), 11 rings
LARGEST = "limit_15_ac_scans_four_component_dc_scan"
_limit_case(LARGEST, True, CMYK, lambda: [("dc", [0, 1, 2, 3])] + _bit_planes(0, 3) + _bit_planes(1, 3) + _bit_planes(2, 3) + _bit_planes(3, 2),
            lambda es: _ac_scans(es) == 15 and es[0][1] == [0, 1, 2, 3] and second_level_tables(AC_PROG) == 9)
_limit_case("limit_16_ac_scans", False, CMYK, lambda: [("dc", [0, 1, 2, 3])] + sum((_bit_planes(c, 3) for c in range(4)), []),
            lambda es: _ac_scans(es) == 16 and max(_ac_scans(es, c) for c in range(4)) == 4)
_DC3 = [("dc", [c], 0, 2) for c in range(3)]
_DC3_REFINED = [("dc", [c], ah, ah - 1) for ah in (2, 1) for c in range(3)]
_limit_case("limit_24_scans", True, S444, lambda: _DC3 + sum((_bit_planes(c, 4) for c in range(3)), []) + _DC3_REFINED,
            lambda es: len(es) == 24 and _ac_scans(es) == 15 and sum(1 for e in es if e[0] == "dc" and e[2]) == 6)
_limit_case("limit_25_scans", False, S444,
            lambda: [("dc", [0], 0, 3)] + _DC3[1:] + sum((_bit_planes(c, 4) for c in range(3)), []) + [("dc", [0], 3, 2)] + _DC3_REFINED,
            lambda es: len(es) == 25 and _ac_scans(es) == 15)
AC_PROG_10 = (AC_PROG[0][:9] + [40] + AC_PROG[0][10:], AC_PROG[1] + [0x0B, 0x1B, 0x2B, 0x3B])
_limit_case("limit_9_second_level_tables", True, GRAY, lambda: [("dc", [0]), ("ac", 0, 1, 63, 0, 1), ("ac", 0, 1, 63, 1, 0)],
            lambda es: second_level_tables(AC_PROG) == 9)
_limit_case("limit_10_second_level_tables", False, GRAY, lambda: [("dc", [0]), ("ac", 0, 1, 63, 0, 1, {"ac": {0: AC_PROG_10}}), ("ac", 0, 1, 63, 1, 0)],
            lambda es: second_level_tables(AC_PROG_10) == 10)


# ---------------------------------------------------------------------------------------------------------------- for the tests
def get(name):
    """-> Case; its predicate is checked here as well, so that no test can use a file that is not where it says"""
    c, check = CASES[name]()
    assert check(c.log), name
    return c


def holds(name):
    c, check = CASES[name]()
    return bool(check(c.log))


def real_blocks(c, comp):
    """(rows, columns) of the real blocks of component comp of a Case"""
    hmax, vmax = max(s[0] for s in c.sampling), max(s[1] for s in c.sampling)
    cw, ch = -(-c.width * c.sampling[comp][0] // hmax), -(-c.height * c.sampling[comp][1] // vmax)
    return -(-ch // 8), -(-cw // 8)
