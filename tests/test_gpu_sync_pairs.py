"""The first sync launch of the GPU entropy stage takes the sync units of an image two at a time (huff_sync_pair_kernel,
csrc/gpu_huffman.hip): 2 x 255 subsequences and the halo per workgroup, even rows from the assumed state, odd rows from their
neighbour's end state, then correction rounds of alternating parity; what it leaves -- states, task lists, incoming[] -- is per unit
as before.  The inputs put the end of the stream on and around every seam of that layout: one-component scans
(helpers/steered_streams.py) of exactly 128 n destuffed bytes, n subsequences, for n = 1, 2, 3 and -1 / +0 / +1 around 255 (the unit
seam inside a pair), 510 (the pair seam), 765 (a trailing single unit) and 1,020.  A stuffed byte makes the raw scan one byte longer
than the destuffed one, so at n = 255 k the planner lays out a unit more than the stream fills: the pair's second unit, or a pair of
its own, that finds nothing to do.

Every case: coefficient tensors equal to the host entropy stage's bit for bit, pixels equal to the oracle's, every image decoded by the
GPU entropy stage, none handed back to the host decoder."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)

import oracle
from helpers import steered_streams as S
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

SUBSEQ_BYTES = 128
OWN = 255                                    # subsequences of a sync unit (kHuffOwn)
LENGTHS = (1, 2, 3, 254, 255, 256, 257, 509, 510, 511, 512, 765, 766, 1021)
UNIT_SEAM, PAIR_SEAM = (254, 255, 256, 257), (509, 510, 511, 512)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scan_of(n):
    """A finished Steered whose destuffed scan is exactly n subsequences long"""
    w = S.Steered(8 if n <= 3 else 64, 52000 + n)
    if n > 3:
        w.ff_at(300 + n % 50)
    w.finish(dbytes=n * SUBSEQ_BYTES)
    assert w.dbits == 8 * n * SUBSEQ_BYTES
    return w


@functools.lru_cache(maxsize=None)
def restart_scan_of(n, interval):
    """n subsequences of 64-bit blocks, sixteen a subsequence, a restart marker every `interval` blocks: the intervals are whole
    bytes, nothing pads them, and the destuffed stream is exactly 128 n bytes"""
    w = S.Steered(240, 53000 + n, restart_interval=interval)
    w.fixed_blocks(16 * n, 64)
    w.finish()
    assert w.dbits == 8 * n * SUBSEQ_BYTES and w.nrst > 0
    return w


def planned_units(jpeg):
    """sync units the planner lays out: from the scan's raw length (the destuffed one is known on the device only)"""
    sos = jpeg.rfind(b"\xff\xda")
    raw = len(jpeg) - 2 - (sos + 2 + int.from_bytes(jpeg[sos + 2:sos + 4], "big"))
    return max(1, -(-(-(-raw * 8 // 1024)) // OWN))


@functools.lru_cache(maxsize=None)
def photo():
    j = oracle.encode(synth_image(640, 480, seed=5), "420", 90)
    scan = j[j.rfind(b"\xff\xda"):]
    nsub = -(-(len(scan) - scan.count(b"\xff\x00")) // SUBSEQ_BYTES)
    assert 2 * OWN < nsub <= 3 * OWN, nsub        # about 600 subsequences: a pair and a single unit
    return j


@functools.lru_cache(maxsize=None)
def reference(jpeg):
    """(host entropy stage's coefficient planes, oracle's RGB pixels): computed once per file, left alone"""
    return lowlevel.decode_coefficients_host(jpeg)[1], oracle.decode(jpeg)


def check(handles, jpegs):
    import torch
    dec, coef = handles
    statuses, images = coef.decode(jpegs)
    torch.cuda.synchronize()
    assert list(statuses) == [0] * len(jpegs)
    assert coef.stats()["gpu_decoded_images"] == len(jpegs)
    for k, (j, im) in enumerate(zip(jpegs, images)):
        want = reference(j)[0]
        assert len(im.coefs) == len(want), k
        for c, (g, w) in enumerate(zip(im.coefs, want)):
            g = g.cpu().numpy()
            assert g.shape == w.shape and g.dtype == w.dtype, (k, c)
            assert np.array_equal(g, w), "file %d of the batch, component %d: first differing coefficient %s" % (k, c, tuple(np.argwhere(g != w)[0]))
    outs, st = dec.decode(jpegs, gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st), list(st)
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
    for k, (j, o) in enumerate(zip(jpegs, outs)):
        got, want = o.cpu().numpy(), reference(j)[1]
        assert got.shape == want.shape and np.array_equal(got, want), "file %d of the batch: first differing pixel %s" % (k, tuple(np.argwhere(got != want)[0]))


@pytest.fixture(scope="module")
def handles():
    import torch
    assert torch.cuda.is_available()
    dec = lowlevel.BatchDecoder(0, num_threads=4)
    coef = lowlevel.BatchCoefficients(device=0, num_threads=4, gpu_huffman=True)
    yield dec, coef
    dec.close()
    coef.close()


def test_every_length_in_one_batch(handles):
    """Pairs begin at odd and at even positions of the batch's unit list, and single units stand at both as well."""
    jpegs = [scan_of(n).jpeg for n in LENGTHS]
    starts, singles, unit = set(), set(), 0
    for j in jpegs:
        n = planned_units(j)
        for first in range(0, n, 2):
            (starts if first + 1 < n else singles).add((unit + first) % 2)
        unit += n
    assert starts == {0, 1} and singles == {0, 1}
    # (the planner's extra unit at the multiples of 255: a second unit, or a pair, that lies behind the stream's end)
    assert planned_units(scan_of(255).jpeg) == 2 and planned_units(scan_of(510).jpeg) == 3 and planned_units(scan_of(765).jpeg) == 4
    check(handles, jpegs)


def test_an_odd_unit_count_in_front_of_another_image(handles):
    a, b = scan_of(511).jpeg, scan_of(512).jpeg
    assert planned_units(a) == 3
    check(handles, [a, b, a])


def test_restart_intervals_record_nothing(handles):
    """With restart intervals no decode records, and round 1 decodes only the rows whose guess was wrong."""
    check(handles, [restart_scan_of(255, 7).jpeg, restart_scan_of(510, 128).jpeg, scan_of(3).jpeg])


def test_a_420_picture_of_a_pair_and_a_single_unit(handles):
    check(handles, [photo(), scan_of(2).jpeg, photo()])


@pytest.fixture(scope="module")
def seam_file(tmp_path_factory):
    jpegs = [scan_of(n).jpeg for n in UNIT_SEAM + PAIR_SEAM]
    path = tmp_path_factory.mktemp("sync_pairs") / "batch.pickle"
    with open(path, "wb") as f:
        pickle.dump((jpegs, [reference(j) for j in jpegs]), f)
    return str(path)


@pytest.mark.parametrize("switch", ["HIPJPEG_TAIL_AFTER=0", "HIPJPEG_TAIL_AFTER=1", "HIPJPEG_TAIL_AFTER=3", "HIPJPEG_POSITION_PASS=1"])
def test_unit_and_pair_seams_under_the_switches(seam_file, switch):
    """The switches are read once per process: a child each.  HIPJPEG_TAIL_AFTER: 1 hands round 1's leftovers to the tail kernel,
    3 runs one generic round behind round 2, 0 runs the rounds to the workgroup's fixpoint and launches no tail kernel."""
    name, value = switch.split("=")
    env = dict(os.environ, HIPJPEG_ENABLE_TEST_HOOKS="1", **{name: value})   # (the hooks: host_fallbacks() answers)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), seam_file], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "sync pairs ok" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    with open(sys.argv[1], "rb") as f:
        _jpegs, _refs = pickle.load(f)
    reference = {j: r for j, r in zip(_jpegs, _refs)}.__getitem__
    _dec = lowlevel.BatchDecoder(0, num_threads=4)
    _coef = lowlevel.BatchCoefficients(device=0, num_threads=4, gpu_huffman=True)
    check((_dec, _coef), _jpegs)
    print("sync pairs ok")
    _dec.close()
    _coef.close()
