"""The files of tests/test_walk_step_forms.py on the GPU, each scan three sync workgroups and a halo long, so that pass 0, the
correction rounds, the tail kernels' entry and the position pass all walk them: huff_sync_kernel with its select step (the MCU
position as a countdown, the pair entry in the single entry's layout, long codes as steps of their own), the tail and position
kernels with their branches over the same pair table.  Pixels must equal the oracle's bit for bit, and every file must have been
decoded by the GPU entropy stage."""
import numpy as np
import pytest

import oracle
from helpers import steered_streams as ss
from helpers import walk_files as W
from helpers import walk_step_files as F
from test_cmyk import _reference_rgb

pytestmark = pytest.mark.gpu

MIN_BITS = 3 * F.WG_BITS + 1024   # three sync workgroups (3 x 32,640 destuffed bytes) and a halo


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


def _cpu(o):
    return [p.cpu().numpy() for p in o] if isinstance(o, list) else o.cpu().numpy()


def test_every_wrap_of_the_countdown_as_one_batch(dec):
    """1, 3, 4, 6 and 10 blocks per MCU, two to four table classes; three components as planes, four as RGB"""
    import torch
    files = F.sampling_files(MIN_BITS)
    assert all(W.scan_bits(jpeg)[0] >= MIN_BITS and len(jpeg) < 400 * 1024 for _, jpeg, _, _ in files)
    three = [f for f in files if len(f[3]) in (1, 3)]
    four = [f for f in files if len(f[3]) == 4]
    assert len(three) + len(four) == len(files) and four
    planes, _ = dec.decode([f[1] for f in three], fmt="yuv_planar", gpu_huffman=True)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(three) and dec.host_fallbacks() == 0
    for (name, jpeg, _, _), got in zip(three, planes):
        want = oracle.decode_planes(jpeg)
        got = _cpu(got)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), name
    rgb, _ = dec.decode([f[1] for f in four], fmt="rgb", gpu_huffman=True)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(four) and dec.host_fallbacks() == 0
    for (name, jpeg, _, _), got in zip(four, rgb):
        assert np.array_equal(_cpu(got), _reference_rgb(oracle.decode_cmyk(jpeg), False)), name


def test_placed_symbols_as_one_batch(dec):
    """the pair test at its edges, the pair across a subsequence's end and at the stream's, and the long codes: every case in each
    of three sync workgroups' ranges"""
    files = [w for _, w in F.combined()]
    for w in files:
        assert (w.dbits if isinstance(w, ss.Steered) else w.total_bits) >= MIN_BITS and len(w.jpeg) < 400 * 1024
    ss.decode_on_device(dec, files)
