"""GPU: the block pass (csrc/gpu_huffman.hip, huff_blocks_kernel) runs two 256-lane teams per workgroup, each on one unit of 128 MCUs,
two consecutive units of the same image per workgroup.  These batches put images on every side of that seam: one unit, an even and an
odd number of units (the last workgroup's second team then has no unit), a last unit of a single MCU; consecutive units that belong
to different images, sampling layouts and scans; restart intervals that begin on and next to a unit; truncated streams whose decoded
blocks end inside the first team's unit, exactly between the teams, inside the second team's unit and in a third unit (a team without
blocks must still arrive at the workgroup's barriers); and lookup tables larger than the standard ones, which take the larger dynamic
LDS size.  Pixels are compared bit for bit with the oracle's; every intact file must have been decoded by the GPU entropy stage and
none handed back to the host decoder."""
import random

import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as jc
from helpers import sequential_scans as Q
from helpers import steered_streams as S
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

UNIT = 128                    # MCUs of a block-pass unit (kHuffMcusPerWg)
STANDARD_POOL_BYTES = 13696   # the four Annex K tables as the GPU stage expands them: 6,144 first-level and pair entries + 11 second-level tables


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


_REFS = {}


def _ref(jpeg):
    """The oracle's RGB pixels, computed once per file."""
    if jpeg not in _REFS:
        _REFS[jpeg] = oracle.decode(jpeg)
    return _REFS[jpeg]


def _decode_exact(dec, jpegs):
    import torch
    outs, st = dec.decode(jpegs, gpu_huffman=True)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st)
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
    for k, (j, o) in enumerate(zip(jpegs, outs)):
        got, want = o.cpu().numpy(), _ref(j)
        assert got.shape == want.shape and np.array_equal(got, want), "image %d of %d" % (k, len(jpegs))


def _strip(mcus, sub="420", seed=None, **kw):
    """A picture one MCU high and `mcus` MCUs wide."""
    mw, mh = {"420": (16, 16), "422": (16, 8), "444": (8, 8), "gray": (8, 8)}[sub]
    return oracle.encode(synth_image(mw * mcus, mh, seed=1000 + mcus if seed is None else seed), sub, 90, **kw)


STRIP_MCUS = (1, 127, 128, 129, 255, 256, 257, 383, 384, 385)   # 1, 1, 1, 2, 2, 2, 3, 3, 3, 4 units


@pytest.fixture(scope="module")
def strips():
    return [_strip(n) for n in STRIP_MCUS]


def test_unit_counts_around_the_team_seam_in_one_batch(dec, strips):
    """One unit (second team idle), two (both teams), three (a second workgroup with an idle second team), four; last units of 1, 127
    and 128 MCUs.  In the batch every image's last workgroup is followed by another image's first."""
    assert [-(-n // UNIT) for n in STRIP_MCUS] == [1, 1, 1, 2, 2, 2, 3, 3, 3, 4]
    _decode_exact(dec, strips)


@pytest.mark.parametrize("k", range(len(STRIP_MCUS)), ids=["%d_mcus" % n for n in STRIP_MCUS])
def test_unit_counts_around_the_team_seam_alone(dec, strips, k):
    """Each strip as a batch of its own: the grid's last workgroup is the one with the idle team."""
    _decode_exact(dec, [strips[k]])


def test_consecutive_units_of_different_images_layouts_and_scans(dec):
    """Units per stream, in batch order: 3 | 2 | 3 | 1 | 10, 3, 3 (the three scans) | 3 | 3 | 3 | 1.  Every stream with an odd count is
    followed by a different stream, so a workgroup that took two consecutive units regardless of their image would decode the next
    image's first unit with this image's tables and geometry.  The restart intervals of 128, 127 and 129 MCUs begin on the unit seam,
    one MCU in front of it and one behind."""
    three_scans = Q.recode(oracle.encode(synth_image(16 * 99, 16 * 3, seed=77), "420", 88), [[0], [1], [2]])
    jpegs = [_strip(300, "444"), _strip(130, "gray"), _strip(257, "420", seed=5), _strip(128, "422"), three_scans,
             _strip(300, "420", restart_interval=128), _strip(300, "420", seed=6, restart_interval=127),
             _strip(300, "420", seed=7, restart_interval=129), _strip(1, "420", seed=8)]
    _decode_exact(dec, jpegs)
    _decode_exact(dec, jpegs[::-1])


def _raw_offset(scan, dbytes):
    """Raw offset in a stuffed scan (no markers) behind its first `dbytes` data bytes, a stuffed zero included."""
    i = 0
    for _ in range(dbytes):
        i += 2 if scan[i] == 0xFF else 1
    return i


@pytest.mark.timeout(120)
def test_truncated_streams_that_leave_a_team_without_blocks(dec):
    """A gray strip of 257 MCUs, every block exactly 64 bits, cut so that the decoded blocks end inside unit 0 (block 60), exactly
    between units 0 and 1 (128 whole blocks: the first workgroup's second team has a unit and no block), inside unit 1 (block 200)
    and inside the single block of unit 2; and a 4:2:0 strip of 257 MCUs cut at four places of its scan.  Same statuses as the host
    entropy stage, none of them a success; the intact neighbours in the batch stay exact."""
    import torch
    w = S.Steered(257, 4242)
    w.fixed_blocks(257, 64)
    w.finish()
    assert w.closed == 257 and w.dbits == 257 * 64
    cuts = [w.header + w.scan[:_raw_offset(w.scan, d)] + b"\xff\xd9" for d in (60 * 8 + 3, 128 * 8, 200 * 8 + 5, 256 * 8 + 4)]
    colour = _strip(257, "420", seed=9)
    sos = colour.rfind(b"\xff\xda") + 14
    n = len(colour) - 2 - sos
    cuts += [colour[:sos + n * num // 1000] + b"\xff\xd9" for num in (200, 498, 750, 999)]
    good = [_strip(129), w.jpeg, _strip(300, "444"), colour]
    jpegs = [good[0]] + cuts[:4] + [good[1], good[2]] + cuts[4:] + [good[3]]
    is_good = [j in good for j in jpegs]
    outs = dec.allocate_outputs(jpegs)
    _, st_gpu = dec.decode(jpegs, outs=outs, gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in outs]
    _, st_cpu = dec.decode(jpegs, outs=outs, gpu_huffman=False, check=False)
    torch.cuda.synchronize()
    assert list(st_gpu) == list(st_cpu)
    assert [s == 0 for s in st_gpu] == is_good
    for j, g, ok in zip(jpegs, got, is_good):
        if ok:
            assert np.array_equal(g, _ref(j))


# ---- lookup tables larger than the standard ones
# An AC table with 159 codes of 11 bits behind three short ones: 00 (0,1), 01 EOB, 100 (0,2), then every other (run, size) with size
# 1..10 and ZRL from 10100000000 on.  Two 11-bit codes share a 10-bit prefix, so the GPU stage opens 80 second-level tables.
BIG_BITS = [0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 159, 0, 0, 0, 0, 0]
BIG_VALS = [0x01, 0x00, 0x02] + [s for s in [(r << 4) | n for r in range(16) for n in range(1, 11)] + [0xF0] if s not in (0x01, 0x02)]
assert len(BIG_VALS) == sum(BIG_BITS) == 162


def _pool_bytes(jpeg):
    """Bytes of lookup tables the GPU entropy stage stages for a one-scan file (gpu_huffman_host.cpp table_words): per table a first
    level of 1,024 entries, for AC tables a pair table of 1,024 more, and 64 entries per distinct 10-bit prefix of the longer codes;
    two bytes an entry."""
    words, pos = 0, 2
    while jpeg[pos + 1] != 0xDA:
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        if jpeg[pos + 1] == 0xC4:
            p, end = pos + 4, pos + 2 + n
            while p < end:
                bits = list(jpeg[p + 1:p + 17])
                words += 1024 if jpeg[p] >> 4 == 0 else 2048
                code, prefixes = 0, set()
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        if length > 10:
                            prefixes.add(code >> (length - 10))
                        code += 1
                    code <<= 1
                words += 64 * len(prefixes)
                p += 17 + sum(bits)
        pos += 2 + n
    return 2 * words


def _big_table_file(cols, seed):
    """A gray strip of `cols` blocks coded with the BIG table: short and 11-bit codes mixed, ZRL among them."""
    rng = random.Random(seed)
    ac = jc._codes(BIG_BITS, BIG_VALS)
    dc = jc._codes(*jc.DC_LUMA)
    bw, pred = jc._Bits(), 0
    for _ in range(cols):
        value = rng.randrange(-40, 41)
        nb, bits = jc._magnitude(value - pred)
        pred = value
        bw.put(*dc[nb])
        if nb:
            bw.put(bits, nb)
        z = 1
        while z < 64 and rng.random() < 0.9:
            run = rng.choice((0, 0, 0, 1, 2, 5, 15, 16))
            if z + run > 63:
                break
            if run == 16:
                bw.put(*ac[0xF0])
                z += 16
                continue
            v = rng.choice((1, -1, 2, -3, 5, -9, 17))
            nb, bits = jc._magnitude(v)
            bw.put(*ac[(run << 4) | nb])
            bw.put(bits, nb)
            z += run + 1
        if z < 64:
            bw.put(*ac[0x00])
    bw.flush()
    return S._headers(cols, 1, [2] * 64, BIG_BITS, BIG_VALS) + bytes(bw.out) + b"\xff\xd9"


def test_tables_larger_than_the_standard_pool_beside_standard_ones(dec):
    """The batch's dynamic LDS size is its largest image's: with one such file in it every workgroup, both teams, runs with the larger
    size (one workgroup per CU), the standard-table images too.  300 blocks: three units, the last workgroup's second team idle."""
    big = _big_table_file(300, 31)
    standard = [_strip(129), _strip(300, "444"), _strip(257, "420", seed=5)]
    assert all(_pool_bytes(j) == STANDARD_POOL_BYTES for j in standard)
    assert STANDARD_POOL_BYTES < _pool_bytes(big) <= 24576
    _decode_exact(dec, [standard[0], big, standard[1], standard[2]])
    _decode_exact(dec, [big])
