"""Lossless JPEG (SOF3) with the entropy stage on the GPU: hipjpegDecodeLosslessBatchFlags with HIPJPEG_FLAG_GPU_HUFFMAN against the
goldens libjpeg-turbo produced, against the numpy model on the files that sit on the seams of the entropy kernels
(tests/helpers/lossless_entropy_cases.py, the files of the host twin's tests), and against the same batch decoded with the flag off."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_entropy_cases as EC
from helpers import lossless_files as LF
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(GOLDEN, "manifest_lossless.json")))["lossless"]
GUARD = 0xA5


def golden(name):
    return open(os.path.join(GOLDEN, "lossless", name + ".jpg"), "rb").read()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def decoder(torch):
    d = lowlevel.BatchLosslessDecoder(device=0, num_threads=4, gpu_entropy=True)
    yield d
    d.close()


@pytest.fixture(scope="module")
def host_decoder(torch):
    d = lowlevel.BatchLosslessDecoder(device=0, num_threads=4)
    yield d
    d.close()


@pytest.fixture(scope="module")
def shape():
    return lowlevel.lossless_entropy_shape()


@pytest.fixture(scope="module")
def seams(shape):
    """(name, file, what the model says it decodes to) of every seam file; built once"""
    return [(name, f, LF.model_decode(d, 16, 1, 0, rr)) for name, f, d, rr in EC.seam_cases(shape)]


@pytest.fixture(scope="module")
def ordinary():
    out = []
    for seed, (h, w, n, ps) in enumerate(((40, 90, 1, 1), (70, 33, 3, 6))):
        d = np.random.default_rng(seed + 1).integers(0, 65536, size=(h, w, n))
        out.append((LF.write_differences(d, 16, ps, table=LF.FLAT), LF.model_decode(d, 16, ps)))
    return out


def decode_all(torch, decoder, files, **kw):
    statuses, outs = decoder.decode(files, **kw)
    torch.cuda.synchronize()
    return statuses, [None if o is None else o.cpu().numpy() for o in outs]


def test_all_goldens_in_one_batch(torch, decoder, host_decoder):
    files = [golden(c["name"]) for c in CASES]
    statuses, outs = decode_all(torch, decoder, files)
    assert statuses == [0] * len(files)
    for c, o in zip(CASES, outs):
        got = o if c["dtype"] == "uint16" else (o & 0xFF).astype(np.uint8)
        assert sha(got) == c["sha256"], c["name"]
    stats = decoder.stats()
    assert stats["gpu_images"] == len(files) and stats["host_fallback_images"] == 0
    assert stats["rows_images"] + stats["wavefront_images"] == len(files)
    decode_all(torch, host_decoder, files)
    assert 0 < stats["h2d_bytes"] < host_decoder.stats()["h2d_bytes"]  # only the compressed scans travel
    small = [c for c in CASES if c["dtype"] == "uint8"]
    statuses, outs = decode_all(torch, decoder, [golden(c["name"]) for c in small], dtype=torch.uint8)
    assert statuses == [0] * len(small)
    for c, o in zip(small, outs):
        assert o.dtype == np.uint8 and sha(o) == c["sha256"], c["name"]
    assert decoder.stats()["host_fallback_images"] == 0


@pytest.mark.parametrize("planar", (False, True))
def test_every_seam_file_in_one_batch(torch, decoder, seams, planar):
    statuses, outs = decode_all(torch, decoder, [f for _, f, _ in seams], planar=planar)
    assert statuses == [0] * len(seams)
    for (name, f, want), got in zip(seams, outs):
        assert np.array_equal(np.moveaxis(got, 0, 2) if planar else got, want), name
    stats = decoder.stats()
    assert stats["gpu_images"] == len(seams) and stats["host_fallback_images"] == 0


def framed(torch, h, row_bytes, pitch, offset):
    """A guard-filled device buffer for an h x row_bytes output that lies `offset` bytes in, `pitch` bytes from row to row"""
    return torch.full((offset + pitch * (h - 1) + row_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")


def check_frame(buf, h, row_bytes, pitch, offset, want_rows):
    host = buf.cpu().numpy()
    inside = np.zeros(host.shape, dtype=bool)
    for y in range(h):
        at = offset + y * pitch
        inside[at:at + row_bytes] = True
        if want_rows is not None:
            assert np.array_equal(host[at:at + row_bytes], want_rows[y]), ("row", y)
    if want_rows is None:
        assert (host == GUARD).all(), "a failing image's output was written"
    else:
        assert (host[~inside] == GUARD).all(), "bytes outside the picture were written"


def arena_outputs(torch, wants, offset, planar):
    """-> (raw outputs, frames): every picture at an odd pitch and offset inside guard bytes"""
    raws, frames = [], []
    for want in wants:
        h, w, n = want.shape
        row_bytes = w * 2 * (1 if planar else n)
        pitch = row_bytes + offset + (0 if offset % 2 else 1)
        o = N.LosslessOutput()
        o.sample_bytes, o.planar = 2, int(planar)
        bufs = []
        for c in range(n if planar else 1):
            buf = framed(torch, h, row_bytes, pitch, offset)
            o.plane[c] = buf.data_ptr() + offset
            o.pitch[c] = pitch
            bufs.append(buf)
        raws.append(o)
        frames.append((bufs, h, row_bytes, pitch))
    return raws, frames


@pytest.mark.parametrize("offset,planar", ((1, False), (6, True), (15, False)))
def test_seam_files_at_odd_pitches_inside_guard_frames(torch, decoder, seams, offset, planar):
    picked = [s for s in seams if s[2].shape[0] * s[2].shape[1] < 40000]  # (the longest rows would only make the frames big)
    assert len(picked) >= 20
    raws, frames = arena_outputs(torch, [want for _, _, want in picked], offset, planar)
    statuses, _ = decoder.decode([f for _, f, _ in picked], raw_outputs=raws)
    torch.cuda.synchronize()
    assert statuses == [0] * len(picked)
    assert decoder.stats()["host_fallback_images"] == 0
    for (name, f, want), (bufs, h, row_bytes, pitch) in zip(picked, frames):
        for c, buf in enumerate(bufs):
            rows = want[:, :, c] if planar else want.reshape(h, -1)
            check_frame(buf, h, row_bytes, pitch, offset, [np.ascontiguousarray(r).view(np.uint8) for r in rows])


def test_a_file_that_cannot_synchronise_goes_to_the_host_stage_alone(torch, decoder, shape, ordinary):
    f, d = EC.unsynchronisable(shape)
    files = [ordinary[0][0], f, ordinary[1][0]]
    statuses, outs = decode_all(torch, decoder, files)
    assert statuses == [0, 0, 0]
    assert np.array_equal(outs[0], ordinary[0][1]) and np.array_equal(outs[2], ordinary[1][1])
    assert np.array_equal(outs[1], LF.model_decode(d, 8, 1))
    stats = decoder.stats()
    assert stats["host_fallback_images"] == 1 and stats["gpu_images"] == 2


def test_each_bad_file_fails_alone_between_two_good_ones(torch, decoder, ordinary):
    (good_a, want_a), (good_b, want_b) = ordinary
    for name, bad in EC.bad_cases():
        try:
            lowlevel.decode_lossless_host(bad)
            want_status = 0
        except N.HipJpegError as e:
            want_status = e.status
        info = lowlevel.lossless_info(bad)
        shape_of = np.zeros((info["height"], info["width"], info["num_components"]), dtype=np.uint16)
        raws, frames = arena_outputs(torch, [want_a, shape_of, want_b], 3, False)
        statuses, _ = decoder.decode([good_a, bad, good_b], raw_outputs=raws)
        torch.cuda.synchronize()
        assert statuses == [0, want_status, 0], (name, statuses)
        for k, want in ((0, want_a), (2, want_b)):
            bufs, h, row_bytes, pitch = frames[k]
            check_frame(bufs[0], h, row_bytes, pitch, 3, [np.ascontiguousarray(r).view(np.uint8) for r in want.reshape(h, -1)])
        if want_status != 0:
            bufs, h, row_bytes, pitch = frames[1]
            check_frame(bufs[0], h, row_bytes, pitch, 3, None)


def test_flag_on_and_flag_off_give_the_same_bytes(torch, decoder, host_decoder, shape, seams, ordinary):
    files = [golden(c["name"]) for c in CASES[::9]] + [f for _, f, _ in seams[::3]] + [EC.unsynchronisable(shape)[0]]
    files += [f for _, f in EC.bad_cases()] + [ordinary[0][0], b"junk"]
    st_on, out_on = decode_all(torch, decoder, files)
    st_off, out_off = decode_all(torch, host_decoder, files)
    assert st_on == st_off
    assert 0 in st_on and any(st_on)
    for a, b in zip(out_on, out_off):
        assert (a is None) == (b is None)
        assert a is None or (a.dtype == b.dtype and np.array_equal(a, b))
    on, off = decoder.stats(), host_decoder.stats()
    assert on["gpu_images"] > 0 and on["gpu_images"] + on["host_fallback_images"] >= st_on.count(0)
    assert off["gpu_images"] == 0 and off["host_fallback_images"] == 0 and off["ripple_launches"] == 0


def test_the_measurement_stages_repeat_the_batch(torch, decoder, seams):
    files = [f for _, f, _ in seams[:12]]
    statuses, outs = decoder.decode(files)
    for which in (3, 4, 1, 2):
        decoder.device_stage(which)
    torch.cuda.synchronize()
    for (name, f, want), got in zip(seams, outs):
        assert np.array_equal(got.cpu().numpy(), want), name


# ------------------------------------------------------------------------------------------------------------- plugin and api
def test_the_plugin_option_sends_lossless_samples_through_the_gpu_stage(torch):
    from nvimagecodec_amd import abi as A
    from test_gpu_lossless import plugin_decode
    C = ctypes
    entry = next(c for c in CASES if c["dtype"] == "uint16" and c["components"] == 1)
    lib = A.bind(N.load_host())
    ci = A.init(A.InstanceCreateInfo, A.ST_INSTANCE_CREATE_INFO, load_builtin_modules=1, load_extension_modules=1)
    inst = C.c_void_p()
    assert lib.nvimgcodecInstanceCreate(C.byref(inst), C.byref(ci)) == 0
    ep = A.init(A.ExecutionParams, A.ST_EXECUTION_PARAMS, device_id=0, max_num_cpu_threads=2)
    f = golden(entry["name"])
    h, w = entry["height"], entry["width"]
    try:
        for options, through_gpu in ((b"hipjpeg_decoder:gpu_lossless_entropy=1", 1), (b"", 0)):
            dec = C.c_void_p()
            assert lib.nvimgcodecDecoderCreate(inst, C.byref(dec), C.byref(ep), options) == 0
            before = lowlevel.plugin_lossless_entropy_stats()
            out = torch.zeros((h, w), dtype=torch.uint16, device="cuda:0")
            st = plugin_decode(lib, dec, inst, f, h, w, A.SAMPLEFORMAT_P_Y, 1, 1, A.SAMPLE_DATA_TYPE_UINT16, out.data_ptr(), 2 * w)
            torch.cuda.synchronize()
            lib.nvimgcodecDecoderDestroy(dec)
            assert st == A.PS_SUCCESS
            assert sha(out.cpu().numpy()) == entry["sha256"], options
            after = lowlevel.plugin_lossless_entropy_stats()
            assert after["gpu_images"] - before["gpu_images"] == through_gpu, options
            assert after["host_fallback_images"] == before["host_fallback_images"]
    finally:
        lib.nvimgcodecInstanceDestroy(inst)


def test_api_decoder_reaches_the_option(torch):
    from nvimagecodec_amd import api
    entry = next(c for c in CASES if c["dtype"] == "uint16")
    before = lowlevel.plugin_lossless_entropy_stats()
    with api.Decoder(options=":gpu_lossless_entropy=1") as dec:
        im = dec.decode([golden(entry["name"])], params=api.DecodeParams(allow_any_depth=True, color_spec=api.ColorSpec.UNCHANGED))[0]
        torch.cuda.synchronize()
        assert im is not None and im.dtype == np.uint16
        assert sha(im.cpu()._array) == entry["sha256"]
    assert lowlevel.plugin_lossless_entropy_stats()["gpu_images"] == before["gpu_images"] + 1
