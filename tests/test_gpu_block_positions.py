"""GPU: where the blocks start (csrc/gpu_huffman.hip huff_copy_records_kernel).  One kernel numbers the blocks -- every workgroup of
255 subsequences sums the completed-block counts of the image's subsequences in front of it and scans its own -- and copies the
records; the workgroup with the image's last subsequence reports how many blocks the stream completes.  One-component files of
tests/helpers/steered_streams.py put the end of the stream on the seams of that computation; a cut stream must come back with the
host stage's status; and a batch mixes the record path, the walk and the restart walk, also with every subsequence walked
(HIPJPEG_POSITION_PASS=1)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from helpers import decode_position_mix
from helpers import steered_streams as S

pytestmark = pytest.mark.gpu

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "decode_position_mix.py")
SUBSEQ = 128           # destuffed bytes of a subsequence
UNIT_SEAMS = (1, 2, 255, 256, 257, 510, 511)   # subsequences: one and two workgroups of 255, one short, exact, one over


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def seam_files():
    """Destuffed lengths that give exactly UNIT_SEAMS subsequences: the last one full, or holding a single byte."""
    out = []
    for n in UNIT_SEAMS:
        for dbytes in sorted({SUBSEQ * n, SUBSEQ * (n - 1) + 1} - {1}):
            w = S.Steered(8 if dbytes < 1000 else 64, 11000 + dbytes)
            if dbytes > 1000:
                w.ff_at(300 + dbytes % 50)
            w.finish(dbytes=dbytes, padding=dbytes % 8 if dbytes % SUBSEQ else 0)
            assert -(-w.dbits // (8 * SUBSEQ)) == n
            out.append(w)
    return out


def test_stream_ends_on_the_unit_seams(dec):
    assert sorted({-(-w.dbits // (8 * SUBSEQ)) for w in seam_files()}) == list(UNIT_SEAMS)
    S.decode_on_device(dec, seam_files())


def test_cut_streams_get_the_host_status(dec):
    """Streams that end before their last block, cut inside the first workgroup's subsequences, inside the second's and inside the
    third's: decoded_blocks < total_blocks, reported by the workgroup that holds the last subsequence.  Same statuses as through the
    host entropy stage; the whole file beside them decodes."""
    import torch
    whole = next(w for w in seam_files() if w.dbits == 8 * SUBSEQ * 511)
    head = len(whole.jpeg) - len(whole.scan) - 2
    jpegs = [whole.jpeg[:head + keep] + b"\xff\xd9" for keep in (50, 127 * SUBSEQ, 255 * SUBSEQ - 3, 255 * SUBSEQ + 140, 400 * SUBSEQ, 510 * SUBSEQ + 5)]
    jpegs.append(whole.jpeg)
    outs = dec.allocate_outputs(jpegs, "y")
    _, st_gpu = dec.decode(jpegs, fmt="y", outs=outs, gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == len(jpegs) - 1
    got = outs[-1].cpu().numpy().copy()
    _, st_cpu = dec.decode(jpegs, fmt="y", outs=outs, gpu_huffman=False, check=False)
    torch.cuda.synchronize()
    assert list(st_gpu) == list(st_cpu)
    assert [s == 0 for s in st_gpu] == [False] * (len(jpegs) - 1) + [True]
    assert np.array_equal(got, S.pixels(whole))


def test_scan_without_a_byte_beside_whole_ones(dec):
    """A scan of no bytes at all has no subsequence, and still somebody has to report it: same statuses as the host stage."""
    import torch
    whole = seam_files()[0]
    empty = whole.jpeg[:len(whole.jpeg) - len(whole.scan) - 2] + b"\xff\xd9"
    jpegs = [whole.jpeg, empty, seam_files()[1].jpeg]
    _, st_gpu = dec.decode(jpegs, fmt="y", gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    _, st_cpu = dec.decode(jpegs, fmt="y", gpu_huffman=False, check=False)
    torch.cuda.synchronize()
    assert list(st_gpu) == list(st_cpu) and st_gpu[0] == 0 and st_gpu[1] != 0 and st_gpu[2] == 0


def test_records_walk_and_restart_walk_side_by_side(dec):
    decode_position_mix.check(dec)


def test_the_same_batch_with_every_subsequence_walked():
    env = dict(os.environ, HIPJPEG_POSITION_PASS="1")
    r = subprocess.run([sys.executable, HELPER], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "positions ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
