"""The files of tests/test_walk_table_classes.py and tests/test_walk_long_codes.py on the GPU: huff_sync_kernel walks them with the
table selection in registers, a long code as a step of its own and both rare events as selects; the tail and position kernels
with their branches.  Pixels must equal the oracle's bit for bit, and every intact file must have been decoded by the GPU entropy
stage; the damaged one gets the host path's status."""
import numpy as np
import pytest

import oracle
from helpers import steered_streams as ss
from helpers import walk_files as W
from test_cmyk import _reference_rgb

pytestmark = pytest.mark.gpu


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


def test_table_class_files_as_one_batch(dec):
    """one to four table pairs, 1 to 10 MCU positions, one file of two scans; three components as planes, four as RGB"""
    import torch
    files = W.class_files()
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


def test_long_code_files_as_one_batch(dec):
    """every placement of a long code, without and with restart intervals; the largest stream is 257 subsequences"""
    intact = [w for _, w, ok in W.long_code_files() if ok]
    assert max(w.total_bits for w in intact) > 256 * 1024
    ss.decode_on_device(dec, intact)


@pytest.mark.parametrize("name", ["seam_j1_d10", "seam_j255_d10"])
def test_seam_files_alone(dec, name):
    """a long code whose halves lie on either side of a subsequence seam, and of the sync workgroup's seam, each as a batch of one"""
    by_name = {n: w for n, w, _ in W.long_code_files()}
    for tag in ("", "_rst"):
        ss.decode_on_device(dec, [by_name[name + tag]])


def test_damaged_file_gets_the_host_status(dec):
    """a second-level lookup that hits an entry no code owns: the status of the host entropy path, in a batch with intact files"""
    import torch
    files = {n: w for n, w, _ in W.long_code_files()}
    batch = [files["two_in_a_row"], files["damaged_second_level"], files["long_dc"], files["damaged_second_level_rst"]]
    jpegs = [w.jpeg for w in batch]
    _, host = dec.decode(jpegs, fmt="y", gpu_huffman=False, check=False)
    torch.cuda.synchronize()
    outs, gpu = dec.decode(jpegs, fmt="y", gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    assert list(gpu) == list(host) and gpu[0] == 0 and gpu[2] == 0 and gpu[1] != 0 and gpu[3] != 0
    for k in (0, 2):
        assert np.array_equal(outs[k].cpu().numpy(), ss.pixels(batch[k]))
