"""The steered coefficient pictures of tests/helpers/coder_seams.py through the GPU entropy coder (gpu_huffman_encode.hip,
progressive_encode.hip): every case puts a stuffed byte, a marker, a word or a segment end on a boundary of the write, scan, count,
layout or expand kernel (tests/test_coder_seams.py proves where), and the GPU's file must be the host coder's byte for byte -- alone,
mixed into one launch in two orders, behind the GPU decoder and coef_relayout_kernel in a transcode, and read back by the GPU decoder.
A test lists every failing case by name."""
import numpy as np
import pytest

from helpers import coder_seams as CS
from nvimagecodec_amd import lowlevel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def handles(torch_mod):
    gpu = lowlevel.BatchCoefficients(device=0, num_threads=8, gpu_huffman=True, gpu_restart=True, gpu_progressive_restart=True)
    host = lowlevel.BatchCoefficients(device=0, num_threads=8, gpu_huffman=False)
    yield gpu, host
    gpu.close()
    host.close()


@pytest.fixture(scope="module")
def built(torch_mod):
    """name -> (case, reference file, coefficient tensors on the device): built once, left alone"""
    out = {}
    for c in list(CS.cases()) + [c for b in CS.batches() for c in b.cases]:
        if c.name not in out:
            out[c.name] = (c, CS.view(c).file, [torch_mod.from_numpy(a).to("cuda:0") for a in c.coefs])
    return out


def _names(what, wrong):
    """every failing case by name (a string: pytest abbreviates lists)"""
    return f"{what}: {len(wrong)} failing: " + " ".join(str(w) for w in wrong)


def _encode(handle, built, cases):
    per = {k: [c.params[k] for c in cases] for k in ("optimized_huffman", "progressive", "restart_interval")}
    return handle.encode([(c.info, built[c.name][2]) for c in cases], **per)


def _same(handle, built, cases, coded, what):
    """statuses 0, every file the reference, and the GPU coder took `coded` of them; returns the files"""
    statuses, files = _encode(handle, built, cases)
    assert statuses == [0] * len(cases), _names(what, [c.name for c, s in zip(cases, statuses) if s])
    assert handle.stats()["gpu_coded_images"] == coded, what
    wrong = [c.name for c, f in zip(cases, files) if f != built[c.name][1]]
    assert not wrong, _names(what, wrong)
    return files


def test_every_case_alone(handles, built):
    gpu, host = handles
    wrong = []
    for c in CS.cases():
        for handle, coded in ((gpu, 1), (host, 0)):
            statuses, files = _encode(handle, built, [c])
            if statuses != [0] or files[0] != built[c.name][1] or handle.stats()["gpu_coded_images"] != coded:
                wrong.append(f"{c.name}({'gpu' if coded else 'host'})")
    assert not wrong, _names("alone", wrong)


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
def test_one_launch_in_two_orders(handles, built, progressive):
    """W6 for the baseline launch (Annex-K and optimized tables, with and without restart intervals: the images without one take the
    rst_blocks == 0 path of the restart flavours); a file's bytes do not depend on its place in the arena."""
    gpu, _ = handles
    cases = [c for c in CS.cases() if c.params["progressive"] == progressive]
    if not progressive:
        assert [c.name for c in cases] == [c.name for c in CS.batches()[0].cases] and CS.p_mixed_launch(cases)
    _same(gpu, built, cases, len(cases), "as listed")
    order = np.random.default_rng(5).permutation(len(cases))
    _same(gpu, built, [cases[i] for i in order], len(cases), "shuffled")
    _same(gpu, built, cases[::-1], len(cases), "reversed")


@pytest.mark.parametrize("batch", [1, 2], ids=["257", "513"])
def test_more_files_than_layout_lanes(handles, built, batch):
    """E8: each lane of the layout kernel lays out two (three) files, of one and of several segments in turn"""
    gpu, _ = handles
    cases = list(CS.batches()[batch].cases)
    assert len(cases) > CS.UNIT_BLOCKS * batch
    _same(gpu, built, cases, len(cases), "as listed")
    _same(gpu, built, cases[1:] + cases[:1], len(cases), "rotated")


def test_through_the_transcoder(built):
    """decoder -> coef_relayout_kernel -> coder on the same seams: the source is the reference file, the output has the case's coding
    parameters -- the lossless transcode of a file the coder wrote itself, with nothing turned, cut or copied, is that file."""
    t = lowlevel.BatchTranscoder(device=0, num_threads=8, gpu_huffman=True, gpu_restart=True, gpu_progressive_intervals=True,
                                 gpu_progressive_restart=True)
    try:
        cases = [c for c in CS.cases() if c.seams[0][0] in "WE"]
        per = {k: [c.params[k] for c in cases] for k in ("optimized_huffman", "progressive", "restart_interval")}
        statuses, files = t.transcode([built[c.name][1] for c in cases], **per)
        assert statuses == [0] * len(cases), _names("status", [c.name for c, s in zip(cases, statuses) if s])
        wrong = [c.name for c, f in zip(cases, files) if f != built[c.name][1]]
        assert not wrong, _names("transcode", wrong)
        assert t.stats()["gpu_coded_images"] == len(cases)
    finally:
        t.close()


def test_gpu_decoder_reads_the_gpu_written_files(handles, built, torch_mod):
    gpu, _ = handles
    cases = list(CS.cases())
    files = _same(gpu, built, cases, len(cases), "encode")
    statuses, images = gpu.decode(files)
    torch_mod.cuda.synchronize()
    assert statuses == [0] * len(cases), _names("status", [c.name for c, s in zip(cases, statuses) if s])
    assert gpu.stats()["gpu_decoded_images"] > 0
    wrong = [c.name for c, im in zip(cases, images) if not all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(im.coefs, c.coefs))]
    assert not wrong, _names("decode", wrong)
