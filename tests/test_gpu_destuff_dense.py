"""Scans that are dense in stuffed bytes, for the compaction of destuff_compact_kernel (csrc/gpu_huffman.hip): a lane squeezes the
dropped bytes out of its sixteen words and gives the kept ones to LDS as aligned dwords, bytes only at its two ragged ends.  The
photographs and the steered files of the other tests have a stuffed byte in one lane of five; here almost every word of a lane has
one or two.

The files have tables of their own, built as tests/helpers/steered_streams.py builds its files: every Huffman code, DC and AC, is 8 bits
long and every coefficient has 8 value bits, so the scan is a sequence of whole bytes -- code, value -- and a coefficient of +255 is
the three raw bytes `code FF 00`.  A dense run is nothing but such triples: every third raw byte is a stuffed zero.  (A block holds at
most 63 coefficients, and the byte or two between two blocks -- EOB, the next DC code -- carry no FF: over a whole chunk the share
stays a little under a third, 0.328 with this writer's blocks; test_files_are_what_they_claim counts it.)  Values other than +255 give runs without any
FF.  The cases: whole 16,384-byte chunks of dense runs; a chunk without a single stuffed byte; dense runs whose last stuffed zero is a
64-byte lane's last byte, or its first; chunks whose output starts at every misalignment 0..3 of the destination, set by the number
of bytes dropped in front of them."""
import functools
import random

import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as jc

CHUNK, LANE = 16384, 64
RUNS = (0, 1, 3, 7)
AC_BITS = [0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0]
AC_VALS = [0x00] + [(r << 4) | 8 for r in RUNS]      # EOB, then (run, 8): codes 00 .. 04
DC_BITS = [0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = [0, 8]                                     # difference 0: code 00; a difference of 8 bits: code 01
AC = jc._codes(AC_BITS, AC_VALS)
DC = jc._codes(DC_BITS, DC_VALS)
assert all(length == 8 and code < 5 for code, length in list(AC.values()) + list(DC.values()))


def _headers(cols, rows):
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xdb" + (67).to_bytes(2, "big") + b"\x00" + bytes([1] * 64)
    out += b"\xff\xc0" + (11).to_bytes(2, "big") + b"\x08" + (8 * rows).to_bytes(2, "big") + (8 * cols).to_bytes(2, "big") + b"\x01\x01\x11\x00"
    for ident, bits, vals in ((0x00, DC_BITS, DC_VALS), (0x10, AC_BITS, AC_VALS)):
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([ident]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda" + (8).to_bytes(2, "big") + b"\x01\x01\x00\x00\x3f\x00"
    return bytes(out)


def _value_byte(v):
    """The 8 value bits of a coefficient or DC difference of +-128 .. +-255."""
    assert 128 <= abs(v) <= 255
    return v if v > 0 else v + 255


class Dense:
    """Writes one scan of whole bytes.  A block is open between calls."""

    def __init__(self, cols, seed):
        self.cols, self.rng = cols, random.Random(seed)
        self.out = bytearray()
        self.blocks, self.pred, self.z, self.closed = [], 0, None, 0
        self.placed = []     # raw offsets of the stuffed zeros the cases are about

    def _byte(self, b):
        self.out.append(b)
        if b == 0xFF:
            self.out.append(0)

    def _open(self, diff=0):
        self.out.append(DC[8 if diff else 0][0])
        if diff:
            self._byte(_value_byte(diff))
        self.pred += diff
        self.blocks.append([self.pred, {}])
        self.z = 1

    def _open_big(self, dense):
        """A DC difference of 8 bits that keeps the DC value small: +255 (a triple) where a dense run may have it."""
        if dense and self.pred <= 0:
            self._open(255)
        else:
            mag = self.rng.randrange(128, 255)
            self._open(-mag if self.pred > 0 else mag)

    def _tok(self, run, value):
        assert self.z + run <= 63
        self.out.append(AC[(run << 4) | 8][0])
        self._byte(_value_byte(value))
        self.z += run
        self.blocks[-1][1][self.z] = value
        self.z += 1

    def _close(self):
        if self.z < 64:
            self.out.append(AC[0x00][0])
        self.z = None
        self.closed += 1

    def _quiet_value(self):
        mag = self.rng.randrange(128, 255)      # never 255: its value byte would be FF (positive) -- or 00, fine, but keep both off
        return mag if self.rng.random() < 0.5 else -mag

    def quiet_to(self, pos, room=1):
        """Coefficients and block breaks without any FF up to exactly this raw offset; leaves room for `room` more coefficients."""
        if self.z is None:
            self._open()
        while True:
            r = pos - len(self.out)
            assert r >= 0 and r != 1, "the position asked for lies behind, or one byte ahead"
            if r == 0:
                break
            run = self.rng.choice([k for k in RUNS if self.z + k + 1 <= 63 - room] or [None])
            if r % 2:                      # a break of three bytes: EOB, DC code, value
                self._close()
                self._open_big(False)
            elif run is None or self.rng.random() < 0.05:
                self._close()
                self._open()
            else:
                self._tok(run, self._quiet_value())
        assert self.z <= 63 - room

    def dense_run(self, n):
        """n triples `code FF 00` in a row, nothing between them."""
        for _ in range(n):
            self._tok(0, 255)

    def dense_to(self, pos):
        """Triples up to this raw offset or at most two bytes further, the blocks broken as rarely as their 63 coefficients allow
        (with a few shorter ones, so that the stream does not repeat itself)."""
        if self.z is None:
            self._open_big(True)
        while len(self.out) < pos:
            runs = [k for k in (0,) * 12 + (1, 3, 7) if self.z + k <= 63]
            if not runs or self.rng.random() < 0.01:
                self._close()
                self._open_big(True)
            else:
                self._tok(self.rng.choice(runs), 255)

    def finish(self):
        self._close()
        while self.closed % self.cols:
            self._open()
            self._close()
        self.scan = bytes(self.out)
        self.jpeg = _headers(self.cols, self.closed // self.cols) + self.scan + b"\xff\xd9"
        return self

    def coefficients(self):
        out = np.zeros((self.closed, 64), np.int16)
        for b, (dc, ac) in enumerate(self.blocks):
            out[b, 0] = dc
            for z, v in ac.items():
                out[b, jc.ZIGZAG[z]] = v
        return out.reshape(self.closed // self.cols, self.cols, 64)


def _stuffed(scan, lo, hi):
    """Offsets of the stuffed zeros in scan[lo:hi]."""
    return [i for i in range(max(lo, 1), min(hi, len(scan))) if scan[i] == 0 and scan[i - 1] == 0xFF]


@functools.lru_cache(maxsize=None)
def files():
    res = {}
    # three whole chunks of dense runs
    w = Dense(16, 1)
    w.dense_to(3 * CHUNK + 500)
    res["dense"] = w.finish()
    # a chunk without a stuffed byte between two dense ones; the byte in front of it is no FF either
    w = Dense(16, 2)
    w.dense_to(CHUNK - 200)
    w.quiet_to(2 * CHUNK + 2)
    w.dense_to(2 * CHUNK + 3000)
    res["none"] = w.finish()
    # dense runs of 1, 2, 21 and 43 triples whose last stuffed zero is a lane's last byte (offset 64 k + 63) or its first (64 k), early
    # in a chunk and late, with lanes without any drop on either side
    for name, phase in (("lane_last", LANE - 1), ("lane_first", 0)):
        w = Dense(16, 3 + phase)
        for n, k in ((1, 7), (2, 15), (21, 30), (43, 60), (1, 210), (21, 230)):
            zero = LANE * k + phase
            w.quiet_to(zero + 1 - 3 * n, room=n)
            w.dense_run(n)
            assert len(w.out) == zero + 1 and w.out[zero] == 0 and w.out[zero - 1] == 0xFF
            w.placed.append(zero)
            w.quiet_to(zero - phase + 4 * LANE)
        res[name] = w.finish()
    # the destination of chunk 1 at every misalignment: 0 .. 15 triples early in chunk 0, a dense run across the chunk seam
    by_shift = {}
    for extra in range(16):
        w = Dense(16, 100 + extra)
        w.quiet_to(200, room=extra)
        w.dense_run(extra)
        w.quiet_to(CHUNK - 400)
        w.dense_to(2 * CHUNK + 300)
        w.finish()
        by_shift.setdefault((CHUNK - len(_stuffed(w.scan, 0, CHUNK))) % 4, w)
    assert sorted(by_shift) == [0, 1, 2, 3]
    for shift, w in by_shift.items():
        res["shift%d" % shift] = w
    return res


def test_files_are_what_they_claim():
    """On the CPU: the oracle and the host entropy decoder accept every file and find the coefficients the writer meant; the host
    emulation of the GPU stage's algorithm agrees; and the scans have the stuffed bytes where the cases want them."""
    from nvimagecodec_amd import lowlevel
    f = files()
    for name, w in f.items():
        want = w.coefficients()
        got, _ = oracle.decode_coefficients(w.jpeg)
        assert np.array_equal(np.asarray(got[0]).reshape(want.shape), want), name
        host, _ = lowlevel.entropy_decode_host(w.jpeg)
        assert np.array_equal(np.asarray(host[0]).reshape(want.shape), want), name
        emu, _ = lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)
        assert np.array_equal(np.asarray(emu[0]).reshape(want.shape), want), name
    scan = f["dense"].scan
    for c in range(3):   # every third raw byte but the breaks between blocks: 0.3280 .. 0.3284 of the chunks as written
        assert len(_stuffed(scan, c * CHUNK, (c + 1) * CHUNK)) >= 0.3275 * CHUNK, c
    scan = f["none"].scan
    assert 0xFF not in scan[CHUNK - 1:2 * CHUNK + 1]
    assert len(_stuffed(scan, 0, CHUNK)) > 4000 and len(_stuffed(scan, 2 * CHUNK, len(scan))) > 500
    for name, phase in (("lane_last", LANE - 1), ("lane_first", 0)):
        w = f[name]
        assert len(w.placed) == 6 and {z // CHUNK for z in w.placed} == {0} and max(w.placed) > CHUNK - 3000
        for z in w.placed:
            assert z % LANE == phase and w.scan[z - 1:z + 1] == b"\xff\x00"
            lane = z // LANE
            assert 0xFF not in w.scan[z + 1:(lane + 3) * LANE]      # nothing dropped behind the run: two lanes without a drop
    assert [(CHUNK - len(_stuffed(f["shift%d" % k].scan, 0, CHUNK))) % 4 for k in range(4)] == [0, 1, 2, 3]
    for k in range(4):   # (and the run lies across the seam)
        assert len(_stuffed(f["shift%d" % k].scan, CHUNK - 64, CHUNK + 64)) > 30


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


@pytest.mark.gpu
def test_dense_scans_on_the_device(dec):
    """All files as one batch through the GPU entropy stage: the oracle's pixels bit for bit, no file handed back to the host."""
    from helpers import steered_streams as S
    S.decode_on_device(dec, list(files().values()))


@pytest.mark.gpu
def test_dense_scans_counted_on_the_device():
    """The same batch with the dropped bytes counted by the device (HIPJPEG_DEVICE_DESTUFF_COUNT=1, read once per process): the count
    kernel and the compaction must agree on every dense chunk."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_destuff_dense as T\n"
            "from helpers import steered_streams as S\n"
            "from nvimagecodec_amd.lowlevel import BatchDecoder\n"
            "dec = BatchDecoder(0, num_threads=4)\n"
            "S.decode_on_device(dec, list(T.files().values()))\n"
            "dec.close()\n"
            "print('dense ok')\n" % (os.path.dirname(here), here))
    env = dict(os.environ, HIPJPEG_DEVICE_DESTUFF_COUNT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dense ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
