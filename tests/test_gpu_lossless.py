"""Lossless JPEG (SOF3) on the GPU: hipjpegDecodeLosslessBatch against the goldens libjpeg-turbo produced and, on the seams of the two
reconstruction kernels, against the numpy model of tests/helpers/lossless_files.py."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_files as LF
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_lossless.json")))
CASES = MANIFEST["lossless"]
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
    d = lowlevel.BatchLosslessDecoder(device=0, num_threads=4)
    yield d
    d.close()


@pytest.fixture(scope="module")
def shape():
    return lowlevel.lossless_kernel_shape()


def decode_all(torch, decoder, files, **kw):
    statuses, outs = decoder.decode(files, **kw)
    torch.cuda.synchronize()
    return statuses, [None if o is None else o.cpu().numpy() for o in outs]


def noise_file(seed, h, w, n, ps, rr=0, precision=16, pt=0):
    """-> (file, samples the model says it decodes to); noise differences reach every state, wraps included"""
    d = np.random.default_rng(seed).integers(0, 65536, size=(h, w, n))
    return LF.write_differences(d, precision, ps, pt, rr, table=LF.FLAT), LF.model_decode(d, precision, ps, pt, rr)


def test_all_goldens_in_one_batch(torch, decoder):
    files = [golden(c["name"]) for c in CASES]
    statuses, outs = decode_all(torch, decoder, files)
    assert statuses == [0] * len(files)
    for c, o in zip(CASES, outs):
        got = o if c["dtype"] == "uint16" else (o & 0xFF).astype(np.uint8)
        assert sha(got) == c["sha256"], c["name"]
    stats = decoder.stats()
    assert stats["rows_images"] + stats["wavefront_images"] == len(files)
    assert stats["wavefront_images"] >= sum(c["predictor"] != 1 for c in CASES)
    assert stats["h2d_bytes"] > 0
    # the files of eight bits and fewer as bytes
    small = [c for c in CASES if c["dtype"] == "uint8"]
    statuses, outs = decode_all(torch, decoder, [golden(c["name"]) for c in small], dtype=torch.uint8)
    assert statuses == [0] * len(small)
    for c, o in zip(small, outs):
        assert o.dtype == np.uint8 and sha(o) == c["sha256"], c["name"]


@pytest.mark.parametrize("ps", range(1, 8))
def test_every_predictor_on_the_band_and_tile_seams(torch, decoder, shape, ps):
    B = shape["band_rows"]
    assert shape["tile_columns"] == 64 and shape["rows_min_width"] == 64  # the widths below sit on these
    files, wants = [], []
    for h in (1, 2, B - 1, B, B + 1, 2 * B + 1):
        for w in (1, 2, 63, 64, 65, 129):
            f, want = noise_file(ps * 10000 + h * 200 + w, h, w, 1, ps)
            files.append(f)
            wants.append(want)
    statuses, outs = decode_all(torch, decoder, files)
    assert statuses == [0] * len(files)
    for f, want, got in zip(files, wants, outs):
        assert np.array_equal(got, want), (ps, want.shape, np.argwhere(got != want)[:4].tolist())
    stats = decoder.stats()
    if ps == 1:
        assert stats["rows_images"] == 18 and stats["wavefront_images"] == 18  # widths 64, 65, 129 / 1, 2, 63
    else:
        assert stats["rows_images"] == 0


def test_predictor_1_on_the_chunk_seams(torch, decoder, shape):
    K = shape["chunk_samples"]
    files, wants = [], []
    for h in (1, 3):
        for w in (K - 1, K, K + 1, 2 * K + 1):
            for rr in (0, 1):
                f, want = noise_file(h * 100000 + w + rr, h, w, 1, 1, rr)
                files.append(f)
                wants.append(want)
    statuses, outs = decode_all(torch, decoder, files)
    assert statuses == [0] * len(files)
    assert decoder.stats()["rows_images"] == len(files)
    for want, got in zip(wants, outs):
        assert np.array_equal(got, want), (want.shape, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("ps", (1, 2, 4, 7))
def test_restart_intervals_on_the_band_seams(torch, decoder, shape, ps):
    B = shape["band_rows"]
    files, wants = [], []
    # an interval that ends on a band's last row, one that ends on a band's first row, single rows, and one longer than a band
    for rr in (B, B + 1, B // 2, 1, B + B // 2):
        for w in (5, 70):
            f, want = noise_file(ps * 1000 + rr * 7 + w, 2 * B + 3, w, 1, ps, rr)
            files.append(f)
            wants.append(want)
    statuses, outs = decode_all(torch, decoder, files)
    assert statuses == [0] * len(files)
    for want, got in zip(wants, outs):
        assert np.array_equal(got, want), (ps, want.shape)


@pytest.mark.parametrize("planar", (False, True))
def test_three_components_interleaved_and_planar(torch, decoder, shape, planar):
    B = shape["band_rows"]
    files, wants = [], []
    for ps in (1, 5):
        for (h, w) in ((B + 2, 67), (3, 130)):
            f, want = noise_file(ps * 31 + h + w, h, w, 3, ps, precision=12, pt=1)
            files.append(f)
            wants.append(want)
    f4, w4 = noise_file(44, 9, 66, 4, 1)
    f2, w2 = noise_file(22, 9, 11, 2, 6)
    files += [f4, f2]
    wants += [w4, w2]
    statuses, outs = decode_all(torch, decoder, files, planar=planar)
    assert statuses == [0] * len(files)
    for want, got in zip(wants, outs):
        assert np.array_equal(np.moveaxis(got, 0, 2) if planar else got, want), want.shape


def test_uint8_and_uint16_outputs(torch, decoder):
    for precision, pt in ((8, 0), (8, 2), (2, 1), (5, 0)):
        for ps in (1, 3):
            d = np.random.default_rng(precision * 10 + ps).integers(0, 65536, size=(70, 131, 3))
            f = LF.write_differences(d, precision, ps, pt, 0, table=LF.FLAT)
            states = LF.model_states(d, precision, ps, pt)
            st8, o8 = decode_all(torch, decoder, [f], dtype=torch.uint8)
            st16, o16 = decode_all(torch, decoder, [f], dtype=torch.uint16)
            assert st8 == [0] and st16 == [0]
            assert o8[0].dtype == np.uint8 and np.array_equal(o8[0], LF.model_decode(d, precision, ps, pt))
            assert o16[0].dtype == np.uint16 and np.array_equal(o16[0], ((states << pt) & 0xFFFF).astype(np.uint16))
    # bytes are not offered for more than eight bits
    f, _ = noise_file(1, 4, 4, 1, 1, precision=9)
    statuses, outs = decode_all(torch, decoder, [f], dtype=torch.uint8)
    assert N.STATUS_NAMES[statuses[0]] == "UNSUPPORTED" and outs[0] is None


def framed(torch, h, row_bytes, pitch, offset):
    """A guard-filled device buffer and the place of an h x row_bytes output in it: `offset` bytes in, `pitch` bytes from row to row"""
    total = offset + pitch * (h - 1) + row_bytes + 64
    return torch.full((total,), GUARD, dtype=torch.uint8, device="cuda:0")


def check_frame(buf, h, row_bytes, pitch, offset, want_rows):
    host = buf.cpu().numpy()
    inside = np.zeros(host.shape, dtype=bool)
    for y in range(h):
        at = offset + y * pitch
        inside[at:at + row_bytes] = True
        assert np.array_equal(host[at:at + row_bytes], want_rows[y]), ("row", y)
    assert (host[~inside] == GUARD).all(), "bytes outside the picture were written"


@pytest.mark.parametrize("offset", range(1, 16))
def test_odd_pitches_and_offsets_inside_a_guard_frame(torch, decoder, shape, offset):
    B = shape["band_rows"]
    jobs = []  # (file, want H x W x N, sample bytes, planar)
    for ps, (h, w), n, size, planar in ((1, (3, 200), 1, 2, False), (1, (B + 1, 77), 3, 2, False), (1, (2, 70), 3, 1, True), (4, (B + 1, 66), 1, 2, False),
                                        (7, (5, 9), 3, 2, True), (2, (4, 130), 2, 1, False), (1, (2, 2049), 1, 2, False), (1, (2, 136), 1, 1, False)):
        precision = 16 if size == 2 else 8
        f, want = noise_file(offset * 100 + ps + w, h, w, n, ps, precision=precision)
        jobs.append((f, want, size, planar))
    files, raws, frames = [], [], []
    for f, want, size, planar in jobs:
        h, w, n = want.shape
        row_bytes = w * size * (1 if planar else n)
        pitch = row_bytes + offset + (0 if offset % 2 else 1)  # odd pitches too
        o = N.LosslessOutput()
        o.sample_bytes, o.planar = size, int(planar)
        bufs = []
        for c in range(n if planar else 1):
            buf = framed(torch, h, row_bytes, pitch, offset)
            o.plane[c] = buf.data_ptr() + offset
            o.pitch[c] = pitch
            bufs.append(buf)
        files.append(f)
        raws.append(o)
        frames.append((bufs, h, row_bytes, pitch))
    statuses, _ = decoder.decode(files, raw_outputs=raws)
    torch.cuda.synchronize()
    assert statuses == [0] * len(files)
    for (f, want, size, planar), (bufs, h, row_bytes, pitch) in zip(jobs, frames):
        for c, buf in enumerate(bufs):
            rows = want[:, :, c] if planar else want.reshape(h, -1)
            check_frame(buf, h, row_bytes, pitch, offset, [np.ascontiguousarray(r).view(np.uint8) for r in rows])


def test_a_truncated_and_an_unsupported_image_fail_alone(torch, decoder):
    good_a, want_a = noise_file(1, 40, 90, 1, 1)
    good_b, want_b = noise_file(2, 70, 33, 3, 6)
    truncated = good_b[:len(good_b) // 2]
    d = np.zeros((4, 8, 3), dtype=np.int64)
    unsupported = LF.write_differences(d, 8, 1, sampling=[(2, 1), (1, 1), (1, 1)])
    dct = open(os.path.join(GOLDEN, "decode", json.load(open(os.path.join(GOLDEN, "manifest.json")))["decode"][0]["name"] + ".jpg"), "rb").read()
    corrupt = bytearray(golden("rst1_p12_ps3_c1"))
    corrupt[corrupt.index(b"\xff\xd0") + 1] = 0xD5
    info_b = lowlevel.lossless_info(good_b)
    untouched = torch.from_numpy(np.full((info_b["height"], info_b["width"], 3), 0x5A5A, dtype=np.uint16)).to("cuda:0")
    files = [good_a, truncated, unsupported, good_b, dct, bytes(corrupt), b"junk"]
    statuses, outs = decoder.decode(files, outs=[None, untouched, None, None, None, None, None])
    torch.cuda.synchronize()
    assert [N.STATUS_NAMES[s] for s in statuses] == ["SUCCESS", "TRUNCATED", "UNSUPPORTED", "SUCCESS", "UNSUPPORTED", "CORRUPT", "BAD_JPEG"]
    assert np.array_equal(outs[0].cpu().numpy(), want_a) and np.array_equal(outs[3].cpu().numpy(), want_b)
    assert (untouched.cpu().numpy() == 0x5A5A).all()  # a failing image writes nothing
    assert decoder.stats()["rows_images"] + decoder.stats()["wavefront_images"] == 2


def test_batches_follow_each_other_on_a_stream_without_waiting(torch, decoder):
    """more calls than the decoder has staging pages, none synchronised in between"""
    jobs = [noise_file(50 + i, 65 + i, 100 + i, 1, 1 + i % 7) for i in range(5)]
    results = [decoder.decode([f])[1][0] for f, _ in jobs]
    torch.cuda.synchronize()
    for (f, want), got in zip(jobs, results):
        assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------- the plugin route
def plugin_decode_batch(lib, dec, inst, samples, params=None):
    """One nvimgcodecDecoderDecode call.  samples: (data, h, w, fmt, planes, channels, sample_type, buffer_ptr, pitch, color_spec, region)
    each, the last two None for COLORSPEC_UNCHANGED and no region; -> one processing status per sample"""
    from nvimagecodec_amd import abi as A
    C = ctypes
    n = len(samples)
    keep, css, ims = [], [], []
    for data, h, w, fmt, planes, channels, sample_type, buffer_ptr, pitch, color_spec, region in samples:
        arr = np.frombuffer(data, dtype=np.uint8)
        keep.append(arr)
        cs = C.c_void_p()
        assert lib.nvimgcodecCodeStreamCreateFromHostMem(inst, C.byref(cs), arr.ctypes.data, arr.size) == 0
        info = A.init(A.ImageInfo, A.ST_IMAGE_INFO, sample_format=fmt, color_spec=A.COLORSPEC_UNCHANGED if color_spec is None else color_spec,
                      num_planes=planes, buffer=buffer_ptr, buffer_size=pitch * h * planes, buffer_kind=A.BUFFER_KIND_STRIDED_DEVICE, cuda_stream=0)
        for p in range(planes):
            pi = info.plane_info[p]
            pi.width, pi.height, pi.row_stride, pi.num_channels, pi.sample_type = w, h, pitch, channels, sample_type
        if region is not None:
            info.region.struct_type, info.region.struct_size = A.ST_REGION, C.sizeof(A.Region)
            info.region.ndim = 2
            info.region.start[0], info.region.start[1], info.region.end[0], info.region.end[1] = region
        im = C.c_void_p()
        assert lib.nvimgcodecImageCreate(inst, C.byref(im), C.byref(info)) == 0
        css.append(cs)
        ims.append(im)
    dp = params or A.init(A.DecodeParams, A.ST_DECODE_PARAMS)
    fut = C.c_void_p()
    assert lib.nvimgcodecDecoderDecode(dec, (C.c_void_p * n)(*css), (C.c_void_p * n)(*ims), n, C.byref(dp), C.byref(fut)) == 0
    assert lib.nvimgcodecFutureWaitForAll(fut) == 0
    st = (C.c_uint32 * n)()
    cnt = C.c_size_t()
    lib.nvimgcodecFutureGetProcessingStatus(fut, st, C.byref(cnt))
    assert cnt.value == n
    lib.nvimgcodecFutureDestroy(fut)
    for im, cs in zip(ims, css):
        lib.nvimgcodecImageDestroy(im)
        lib.nvimgcodecCodeStreamDestroy(cs)
    return list(st)


def plugin_decode(lib, dec, inst, data, h, w, fmt, planes, channels, sample_type, buffer_ptr, pitch, color_spec=None, params=None, region=None):
    return plugin_decode_batch(lib, dec, inst, [(data, h, w, fmt, planes, channels, sample_type, buffer_ptr, pitch, color_spec, region)], params)[0]


@pytest.fixture(scope="module")
def plugin(torch):
    from nvimagecodec_amd import abi as A
    C = ctypes
    lib = A.bind(N.load_host())
    ci = A.init(A.InstanceCreateInfo, A.ST_INSTANCE_CREATE_INFO, load_builtin_modules=1, load_extension_modules=1)
    inst = C.c_void_p()
    assert lib.nvimgcodecInstanceCreate(C.byref(inst), C.byref(ci)) == 0
    ep = A.init(A.ExecutionParams, A.ST_EXECUTION_PARAMS, device_id=0, max_num_cpu_threads=2)
    dec = C.c_void_p()
    assert lib.nvimgcodecDecoderCreate(inst, C.byref(dec), C.byref(ep), b"") == 0
    yield lib, inst, dec
    lib.nvimgcodecDecoderDestroy(dec)
    lib.nvimgcodecInstanceDestroy(inst)


def test_the_plugin_decodes_lossless_streams_and_says_what_it_does_not(torch, plugin):
    from nvimagecodec_amd import abi as A
    lib, inst, dec = plugin
    U16, U8 = A.SAMPLE_DATA_TYPE_UINT16, A.SAMPLE_DATA_TYPE_UINT8
    gray, want_gray = noise_file(71, 70, 90, 1, 4, precision=12)
    out = torch.zeros((70, 90), dtype=torch.uint16, device="cuda:0")
    assert plugin_decode(lib, dec, inst, gray, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U16, out.data_ptr(), 180) == A.PS_SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_gray[:, :, 0])
    rgb, want_rgb = noise_file(72, 66, 70, 3, 1)
    out = torch.zeros((66, 70, 3), dtype=torch.uint16, device="cuda:0")
    assert plugin_decode(lib, dec, inst, rgb, 66, 70, A.SAMPLEFORMAT_I_UNCHANGED, 1, 3, U16, out.data_ptr(), 420) == A.PS_SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_rgb)
    out = torch.zeros((3, 66, 70), dtype=torch.uint16, device="cuda:0")
    assert plugin_decode(lib, dec, inst, rgb, 66, 70, A.SAMPLEFORMAT_P_UNCHANGED, 3, 1, U16, out.data_ptr(), 140) == A.PS_SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(np.moveaxis(out.cpu().numpy(), 0, 2), want_rgb)
    small, want_small = noise_file(73, 9, 20, 1, 7, precision=8)
    out = torch.zeros((9, 20), dtype=torch.uint8, device="cuda:0")
    assert plugin_decode(lib, dec, inst, small, 9, 20, A.SAMPLEFORMAT_P_Y, 1, 1, U8, out.data_ptr(), 20) == A.PS_SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_small[:, :, 0])
    # the refusal bits (the harness has no other decoder to turn to: the sample fails with them)
    out = torch.zeros((70, 90, 3), dtype=torch.uint16, device="cuda:0")
    ptr = out.data_ptr()
    assert plugin_decode(lib, dec, inst, gray, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U8, ptr, 180) & A.PS_SAMPLE_TYPE_UNSUPPORTED == A.PS_SAMPLE_TYPE_UNSUPPORTED
    assert plugin_decode(lib, dec, inst, gray, 70, 90, A.SAMPLEFORMAT_I_RGB, 1, 3, U16, ptr, 540) & A.PS_SAMPLE_FORMAT_UNSUPPORTED == A.PS_SAMPLE_FORMAT_UNSUPPORTED
    assert plugin_decode(lib, dec, inst, rgb, 66, 70, A.SAMPLEFORMAT_P_Y, 1, 1, U16, ptr, 140) & A.PS_SAMPLE_FORMAT_UNSUPPORTED == A.PS_SAMPLE_FORMAT_UNSUPPORTED
    assert plugin_decode(lib, dec, inst, rgb, 66, 70, A.SAMPLEFORMAT_I_UNCHANGED, 1, 3, U16, ptr, 420, color_spec=A.COLORSPEC_SRGB) & A.PS_COLOR_SPEC_UNSUPPORTED == A.PS_COLOR_SPEC_UNSUPPORTED
    roi = A.init(A.DecodeParams, A.ST_DECODE_PARAMS, enable_roi=1)
    assert plugin_decode(lib, dec, inst, gray, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U16, ptr, 180, params=roi, region=(0, 0, 8, 8)) & A.PS_ROI_UNSUPPORTED == A.PS_ROI_UNSUPPORTED


def test_one_call_holds_dct_and_lossless_samples(torch, plugin):
    """Both kinds interleaved in one nvimgcodecDecoderDecode call, good samples and declined ones: each is reported once, with the status
    and the pixels it has in a call of its own, and a second identical call repeats the first."""
    from conftest import load_decode_case
    from nvimagecodec_amd import abi as A
    lib, inst, dec = plugin
    U16, U8 = A.SAMPLE_DATA_TYPE_UINT16, A.SAMPLE_DATA_TYPE_UINT8
    entries = json.load(open(os.path.join(GOLDEN, "manifest.json")))["decode"]
    (dct_a, want_a), (dct_b, want_b) = (load_decode_case(next(e for e in entries if e["name"] == name))
                                        for name in ("s64x48_420_base_q90", "s50x37_420_base_q90"))
    gray, want_gray = noise_file(71, 70, 90, 1, 4, precision=12)
    rgb, want_rgb = noise_file(72, 66, 70, 3, 1)
    small, want_small = noise_file(73, 9, 20, 1, 7, precision=8)
    cut = gray[:(gray.index(b"\xff\xda") + len(gray)) // 2]  # ends in the middle of the scan
    rgb_of = (A.SAMPLEFORMAT_I_RGB, 1, 3, U8)

    def one_call():
        outs = [torch.zeros(shape, dtype=dtype, device="cuda:0")
                for shape, dtype in (((48, 64, 3), torch.uint8), ((70, 90), torch.uint16), ((66, 70, 3), torch.uint16), ((37, 50, 3), torch.uint8),
                                     ((3, 66, 70), torch.uint16), ((9, 20), torch.uint8), ((70, 90), torch.uint16), ((70, 90), torch.uint16))]
        ptr = [o.data_ptr() for o in outs]
        statuses = plugin_decode_batch(lib, dec, inst, [
            (dct_a, 48, 64) + rgb_of + (ptr[0], 192, A.COLORSPEC_SRGB, None),
            (gray, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U16, ptr[1], 180, None, None),
            (rgb, 66, 70, A.SAMPLEFORMAT_I_UNCHANGED, 1, 3, U16, ptr[2], 420, None, None),
            (dct_b, 37, 50) + rgb_of + (ptr[3], 150, A.COLORSPEC_SRGB, None),
            (rgb, 66, 70, A.SAMPLEFORMAT_P_UNCHANGED, 3, 1, U16, ptr[4], 140, None, None),
            (small, 9, 20, A.SAMPLEFORMAT_P_Y, 1, 1, U8, ptr[5], 20, None, None),
            (gray, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U8, ptr[6], 180, None, None),   # twelve bits are not offered as bytes
            (cut, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U16, ptr[7], 180, None, None)])
        torch.cuda.synchronize()
        return statuses, [o.cpu().numpy() for o in outs]

    double_reports = lib.hipjpegTestDoubleReports()
    statuses, outs = one_call()
    assert statuses[:6] == [A.PS_SUCCESS] * 6
    assert statuses[6] & A.PS_SAMPLE_TYPE_UNSUPPORTED == A.PS_SAMPLE_TYPE_UNSUPPORTED
    assert statuses[7] == A.PS_IMAGE_CORRUPTED  # what the decoder said of it before both routes shared their sample path
    assert np.array_equal(outs[0], want_a) and np.array_equal(outs[3], want_b)
    assert np.array_equal(outs[1], want_gray[:, :, 0])
    assert np.array_equal(outs[2], want_rgb) and np.array_equal(np.moveaxis(outs[4], 0, 2), want_rgb)
    assert np.array_equal(outs[5], want_small[:, :, 0])
    assert not outs[6].any()  # a declined sample writes nothing
    again, outs_again = one_call()
    assert again == statuses
    for a, b in zip(outs, outs_again):
        assert np.array_equal(a, b)
    assert lib.hipjpegTestDoubleReports() == double_reports


def test_a_lossless_file_is_read_through_the_read_fallback(torch, tmp_path):
    """File streams offer no map(): the lossless route reads the bitstream into a copy of its own, as the DCT route does
    (test_gpu_plugin.py::test_read_from_file_uses_read_fallback)."""
    from nvimagecodec_amd import api
    rgb, want_rgb = noise_file(72, 66, 70, 3, 1)
    p = tmp_path / "x.jpg"
    p.write_bytes(rgb)
    with api.Decoder() as dec:
        im = dec.read(str(p), params=api.DecodeParams(allow_any_depth=True, color_spec=api.ColorSpec.UNCHANGED))
        torch.cuda.synchronize()
        assert im is not None and im.dtype == np.uint16
        assert np.array_equal(im.cpu()._array, want_rgb)


def test_api_decoder_with_allow_any_depth(torch):
    from nvimagecodec_amd import api
    f12, want12 = noise_file(81, 67, 130, 3, 6, precision=12, pt=1)
    f16, want16 = noise_file(82, 5, 70, 1, 1)
    dct = open(os.path.join(GOLDEN, "decode", json.load(open(os.path.join(GOLDEN, "manifest.json")))["decode"][0]["name"] + ".jpg"), "rb").read()
    with api.Decoder() as dec:
        unchanged = api.DecodeParams(allow_any_depth=True, color_spec=api.ColorSpec.UNCHANGED)
        images = dec.decode([f12, f16], params=unchanged)
        torch.cuda.synchronize()
        assert images[0] is not None and images[1] is not None
        assert images[0].precision == 12 and images[1].precision == 16
        assert images[0].dtype == np.uint16 and images[0].shape == (67, 130, 3) and images[1].shape == (5, 70, 1)
        assert np.array_equal(images[0].cpu()._array, want12) and np.array_equal(images[1].cpu()._array, want16)
        # default parameters: a lossless stream of more than eight bits stays declined, a DCT file beside it decodes as ever
        both = dec.decode([f12, dct])
        assert both[0] is None and both[1] is not None
