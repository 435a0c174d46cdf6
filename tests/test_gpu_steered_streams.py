"""GPU: crafted scans (tests/helpers/steered_streams.py) put a chosen byte on every seam of the device-only code of the GPU entropy
stage (csrc/gpu_huffman.hip): a stuffed FF 00 or a restart marker on, in front of and behind the 16-byte pieces, 64-byte lane slices
and 16,384-byte chunks of the destuff kernels; scans that end 1..65 bytes into their last chunk or exactly on it; destuffed streams
that end on and around a subsequence and a sync workgroup's 255 subsequences; 29..32 block starts per subsequence around the 30 slots
of a block-start record; blocks longer than a subsequence; rows of 127..257 blocks around the block-pass groups of 128 MCUs.  Every
file goes through BatchDecoder.decode(fmt="y", gpu_huffman=True) and must give the oracle's pixels bit for bit -- decoded by the GPU
entropy stage, never handed back to the host decoder (helpers/steered_streams.py decode_on_device asserts both for every batch).
tests/test_steered_streams.py shows on the CPU that the files are what they claim and that a destuffing gone wrong at a placed byte
changes the pixels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from helpers import steered_streams as S

pytestmark = pytest.mark.gpu

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "decode_steered.py")


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_family_on_the_device(dec, name):
    """seams: lane and piece seams, one batch of 30 files (first_chunk indexing across images).  chunks: chunk seams with every
    destination misalignment of the later chunks.  last_chunk: the short path of the last chunk.  restart_placed / restart_intervals:
    markers on seams, FF 00 FF Dn, interval boundaries around group and subsequence boundaries.  stream_ends, record_slots,
    long_blocks, strips: see the families' docstrings.  No file's seed had to be changed to keep it off the host decoder."""
    S.decode_on_device(dec, S.family(name))


def test_420_pictures_around_one_block_pass_group(dec):
    """127, 128 and 129 MCUs of six blocks, in one row and in several."""
    import torch
    from nvimagecodec_amd.synth import synth_image
    jpegs = [oracle.encode(synth_image(w, h, seed=40 + k), "420", 90)
             for k, (w, h) in enumerate(((16 * 127, 16), (16 * 128, 16), (16 * 129, 16), (16 * 43, 16 * 3), (16 * 16, 16 * 8)))]
    outs, _ = dec.decode(jpegs, fmt="rgb", gpu_huffman=True)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
    for j, o in zip(jpegs, outs):
        assert np.array_equal(o.cpu().numpy(), oracle.decode(j))


def _block_pass_streams():
    """Every stream tests/test_block_pass_streams.py hands to its check_good()."""
    import test_block_pass_streams as T
    got, keep = [], T.check_good
    T.check_good = got.append
    try:
        T.test_eob_behind_short_symbols()
        T.test_zrl_runs()
        for lead in T.test_all_coefficients_present_no_eob.pytestmark[0].args[1]:
            T.test_all_coefficients_present_no_eob(lead)
        T.test_sixteen_bit_code_behind_a_short_one()
        T.test_last_symbols_at_the_end_of_the_stream()
    finally:
        T.check_good = keep
    return [S.gray_file(blocks) for blocks in got]


def test_block_pass_streams_on_the_device(dec):
    """The streams of tests/test_block_pass_streams.py (ZRL runs, blocks without EOB, the 16-bit code, every alignment of the end
    of the stream) through the block pass itself, not its host emulation."""
    import torch
    jpegs = _block_pass_streams()
    assert len(jpegs) > 35
    outs, _ = dec.decode(jpegs, fmt="y", gpu_huffman=True)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
    for k, (j, o) in enumerate(zip(jpegs, outs)):
        assert np.array_equal(o.cpu().numpy(), oracle.decode(j, oracle.FMT_GRAY)), k


def test_truncated_streams_get_the_host_verdict_on_the_device(dec):
    """The truncation sweep of tests/test_block_pass_streams.py: the scan cut after every byte.  Same statuses through the GPU entropy
    stage and the host one, and only the whole scan decodes."""
    import torch
    from test_block_pass_streams import TRUNCATION_BLOCKS
    scan = S.scan_bits(TRUNCATION_BLOCKS)
    jpegs = [S.gray_file(TRUNCATION_BLOCKS, scan[:keep]) for keep in range(1, len(scan) + 1)]
    outs = dec.allocate_outputs(jpegs, "y")
    _, st_gpu = dec.decode(jpegs, fmt="y", outs=outs, gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    whole = outs[-1].cpu().numpy().copy()
    _, st_cpu = dec.decode(jpegs, fmt="y", outs=outs, gpu_huffman=False, check=False)
    torch.cuda.synchronize()
    assert list(st_gpu) == list(st_cpu)
    assert [s == 0 for s in st_gpu] == [False] * (len(scan) - 1) + [True]
    assert np.array_equal(whole, oracle.decode(jpegs[-1], oracle.FMT_GRAY))


def test_zero_copy_input_at_every_source_alignment(dec):
    """The seam batch from pinned memory: every file copied into one pinned tensor at base offsets 0..15 (mod 16) and passed as a
    slice, so that the kernel that gathers unaligned caller memory sees every source alignment; the scans' lengths cover 0, 1 and 15
    mod 16 for its tail."""
    import torch
    files = S.family("seams")
    assert len(files) >= 16 and {len(w.scan) & 15 for w in files} >= {0, 1, 15}
    starts, pos = [], 0
    for k, w in enumerate(files):
        pos = (pos + 15) // 16 * 16 + k % 16
        starts.append(pos)
        pos += len(w.jpeg)
    pinned = torch.zeros(pos + 64, dtype=torch.uint8).pin_memory()
    assert pinned.data_ptr() % 16 == 0
    for at, w in zip(starts, files):
        pinned[at:at + len(w.jpeg)] = torch.frombuffer(bytearray(w.jpeg), dtype=torch.uint8)
    S.decode_on_device(dec, files, inputs=[pinned[at:at + len(w.jpeg)] for at, w in zip(starts, files)])
    assert dec.stats()["zero_copy_images"] == len(files)


@pytest.mark.parametrize("switches", [{"HIPJPEG_DEVICE_DESTUFF_COUNT": "1"}, {"HIPJPEG_POSITION_PASS": "1"}, {"HIPJPEG_TAIL_AFTER": "0"}],
                         ids=["device_destuff_count", "position_pass", "no_tail"])
def test_placed_bytes_under_switch(switches):
    """The seam, chunk, last-chunk and restart batches in a child process per switch (they are read once per process).  Under
    HIPJPEG_DEVICE_DESTUFF_COUNT=1 the device counts the dropped bytes itself: destuff_count_kernel, its short last piece included,
    meets the placed bytes."""
    env = dict(os.environ)
    env.update(switches)
    r = subprocess.run([sys.executable, HELPER], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "steered ok" in r.stdout
