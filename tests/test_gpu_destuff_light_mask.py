"""The destuff kernels of the GPU entropy stage (csrc/gpu_huffman.hip) choose their mask per image: without a restart interval only
the stuffed zeros (FF 00) are looked for, with one the restart markers as well.  That rests on the parser: a scan whose FF Dn
markers are not exactly the ones its restart interval calls for never reaches the kernels, and the counts the parser hands them
(ScanHeader::chunk_drops) are the bytes the chosen mask drops.

Crafted scans (tests/helpers/steered_streams.py): scans of 16,384 and 32,768 raw bytes and 1, 2, 3 and 17 bytes more and less (one
to three chunks); a dropped byte at each of the four positions of a word on a word, a 64-byte lane, a 4,096-byte wave and a chunk
seam; a lane without a drop between two lanes with three each; runs of FF 00 FF 00 [FF 00] across a lane seam; every misalignment
0..3 of a later chunk's destination.  The same seams as restart-interval files with an FF Dn on them.  On the device both kinds go
through one decoder in one process, so both masks run, alone and mixed in one launch; once more in a child process whose device
counts the dropped bytes itself.  On the CPU the parser's counts are compared with a byte-by-byte count of every file."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)

from helpers import steered_streams as S

CHUNK = S.CHUNK
SEAMS = (100, 64 * 3, 4096, CHUNK)   # a word inside a lane, a lane, a wave, a chunk
LENGTHS = (0, 1, 2, 3, 17)


@functools.lru_cache(maxsize=None)
def plain_files():
    out = []
    for base in (CHUNK, 2 * CHUNK):
        for d in sorted({s * x for x in LENGTHS for s in (1, -1)}):
            w = S.Steered(64, 11000 + base // CHUNK * 100 + d)
            for early in range(abs(d) % 4):      # (the second chunk's destination at every misalignment)
                w.ff_at(300 + 90 * early)
            w.ff_at(base - 700)
            w.finish(raw_bytes=base + d)
            out.append(w)
    for seam in SEAMS:
        for k in range(4):                       # the dropped 00 is byte k of the word that starts on the seam
            w = S.Steered(32, 12000 + 4 * seam + k)
            for early in range(k if seam == CHUNK else 0):
                w.ff_at(200 + 110 * early)
            w.ff_at(seam - 1 + k)
            w.ff_at(seam + 500)
            w.finish(raw_bytes=seam + 900 + k)
            out.append(w)
    w = S.Steered(32, 13000)                     # lanes 10 and 12 drop three bytes each, lane 11 none
    for at in (642, 665, 690, 770, 795, 820):
        w.ff_at(at)
    w.finish(raw_bytes=1500)
    assert not any(64 * 11 <= at + 1 < 64 * 12 for _, at in w.placed)
    out.append(w)
    for run, offs in ((2, (-3, -2, -1, 0)), (3, (-5, -3, -1, 0))):
        for d in offs:
            w = S.Steered(16, 13100 + 10 * run + d)
            w.ff_at(64 * 5 + d, run=run)
            w.finish(raw_bytes=64 * 5 + 70 + d % 3)
            out.append(w)
    return out


@functools.lru_cache(maxsize=None)
def restart_files():
    out = []
    for seam in SEAMS:
        for k in range(4):                       # FF Dn with the FF one byte in front of byte k of the seam's word
            w = S.Steered(32, 14000 + 4 * seam + k, restart_interval=1)
            w.rst_at(seam - 1 + k)
            w.rst_at(seam + 400)
            w.finish()
            out.append(w)
    for k, at in enumerate((64 * 3 - 1, 64 * 3, 64 * 3 + 1, 4096, CHUNK - 1, CHUNK, CHUNK + 1)):
        w = S.Steered(32, 14500 + k, restart_interval=1)    # FF 00 FF Dn around the seams
        w.ff_rst_at(at)
        w.finish()
        out.append(w)
    return out


def _byte_by_byte(scan):
    drops = [0] * -(-len(scan) // CHUNK)
    i = 0
    while i + 1 < len(scan):
        if scan[i] == 0xFF and scan[i + 1] == 0x00:
            drops[(i + 1) // CHUNK] += 1
            i += 2
        elif scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            drops[i // CHUNK] += 1
            drops[(i + 1) // CHUNK] += 1
            i += 2
        else:
            i += 1
    return drops


def test_the_parsers_counts_are_the_bytes_the_masks_drop():
    """hipjpegTestScanChunkDrops against a byte-by-byte count, every file.  And what the light mask relies on: a file without a
    restart interval holds no FF Dn, a file with one is the only kind that does."""
    from nvimagecodec_amd import _native as N
    lib = N.load()
    for files, markers in ((plain_files(), False), (restart_files(), True)):
        for w in files:
            assert any(0xD0 <= b <= 0xD7 and a == 0xFF for a, b in zip(w.scan, w.scan[1:])) == markers
            buf = (ctypes.c_uint8 * len(w.jpeg)).from_buffer_copy(w.jpeg)
            out = (ctypes.c_uint32 * 64)()
            n = lib.hipjpegTestScanChunkDrops(ctypes.addressof(buf), len(w.jpeg), 0, out, 64)
            assert n == -(-len(w.scan) // CHUNK), w.placed
            assert list(out)[:n] == _byte_by_byte(w.scan), w.placed


def test_the_files_are_what_they_claim():
    lengths = {len(w.scan) for w in plain_files()}
    assert {base + s * x for base in (CHUNK, 2 * CHUNK) for x in LENGTHS for s in (1, -1)} <= lengths
    dropped = {(at + 1) for w in plain_files() for _, at in w.placed}
    for seam in SEAMS:
        assert {seam + k for k in range(4)} <= dropped, seam
    marked = {at for w in restart_files() for kind, at in w.placed if kind == "rst"}
    for seam in SEAMS:
        assert {seam - 1 + k for k in range(4)} <= marked, seam


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


def _both_masks(dec):
    plain, restart = plain_files(), restart_files()
    S.decode_on_device(dec, plain)
    S.decode_on_device(dec, restart)
    mixed = [w for pair in zip(plain, restart) for w in pair]    # neighbouring workgroups of one launch take different masks
    S.decode_on_device(dec, mixed)
    S.decode_on_device(dec, plain)
    return len(plain) + len(restart)


@pytest.mark.gpu
def test_both_masks_in_one_process(dec):
    _both_masks(dec)


@pytest.mark.gpu
def test_both_masks_counted_on_the_device():
    """HIPJPEG_DEVICE_DESTUFF_COUNT=1 (read once per process): destuff_count_kernel chooses its mask by the same rule."""
    env = dict(os.environ, HIPJPEG_DEVICE_DESTUFF_COUNT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "light mask ok" in r.stdout


if __name__ == "__main__":
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    print("light mask ok", _both_masks(d))
    d.close()
