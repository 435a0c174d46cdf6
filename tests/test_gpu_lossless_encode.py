"""hipjpegEncodeLosslessBatch on the GPU: the kernels write libjpeg-turbo's files byte for byte (the goldens of
tests/golden/make_golden_lossless_encode.py), equal the host twin on every seam of their shape, and what they write decodes back
through both entropy stages of the lossless decoder."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_encode_model as M
from helpers import lossless_encode_seams as S
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel as LL

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_lossless_encode.json")))["lossless_encode"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def encoder(torch_mod):
    enc = LL.BatchLosslessEncoder(device=0, num_threads=2)
    yield enc
    enc.close()


def _tensor(torch, s, planar):
    a = np.ascontiguousarray(s.transpose(2, 0, 1) if planar else s)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda().view(torch.uint16 if a.dtype == np.uint16 else torch.uint8)


def _golden_batch(torch):
    images, per = [], {k: [] for k in ("precision", "predictor", "point_transform", "restart_rows", "planar")}
    for i, e in enumerate(MANIFEST):
        planar = i % 3 == 1
        images.append(_tensor(torch, M.case_samples(e), planar))
        for k in ("precision", "predictor", "point_transform", "restart_rows"):
            per[k].append(e[k])
        per["planar"].append(planar)
    return images, per


def test_mixed_batch_equals_the_goldens_and_a_bad_image_disturbs_nothing(torch_mod, encoder):
    torch = torch_mod
    images, per = _golden_batch(torch)
    mid = len(images) // 2
    images.insert(mid, images[0])
    for k, v in (("precision", 17), ("predictor", 1), ("point_transform", 0), ("restart_rows", 0), ("planar", False)):
        per[k].insert(mid, v)
    statuses, files = encoder.encode(images, **per)
    assert statuses[mid] == 1 and files[mid] is None
    del statuses[mid], files[mid]
    assert statuses == [0] * len(MANIFEST)
    for e, data in zip(MANIFEST, files):
        assert len(data) == e["bytes"] and hashlib.sha256(data).hexdigest() == e["sha256"], e["name"]
    st = encoder.stats()
    assert st["gpu_images"] == len(MANIFEST) and st["waits"] == 2 and st["bit_buffer_bytes"] > sum(e["scan_bytes"] for e in MANIFEST) // 2
    # a second batch on the same handle takes the next page and writes the same bytes; so does the one that takes the first page again
    del images[mid]
    for k in per:
        del per[k][mid]
    for _ in range(3):
        again_statuses, again = encoder.encode(images, **per)
        assert again_statuses == [0] * len(MANIFEST) and again == files


def test_seams_equal_the_host_twin(torch_mod, encoder):
    torch = torch_mod
    shape = LL.lossless_encode_shape()
    cases = S.cases(shape) + S.searched_cases(shape)
    raw, keep, want = [], [], []
    for c in cases:
        x, n, bufs = M.padded_input(N, c["samples"], c["planar"], c["pad"], c["offset"])
        want.append(M.encode_raw_host("hipjpegEncodeLosslessGpuAlgorithmHost", x, n, c["precision"], c["predictor"], c["point_transform"],
                                      c["restart_rows"])[1])
        # the same bytes, pitches and offsets in device memory
        dev = [torch.from_numpy(b).cuda() for b in bufs]
        for k, d in enumerate(dev):
            x.plane[k] = d.data_ptr() + c["offset"]
        keep.append((bufs, dev))
        raw.append((x, n))
    statuses, files = M.encode_raw_batch(encoder, raw, [c["precision"] for c in cases], [c["predictor"] for c in cases],
                                         [c["point_transform"] for c in cases], [c["restart_rows"] for c in cases])
    assert statuses == [0] * len(cases)
    for c, data, w in zip(cases, files, want):
        assert data == w, c["name"]
    assert encoder.stats() == {"gpu_images": len(cases), "waits": 2, "bit_buffer_bytes": encoder.stats()["bit_buffer_bytes"]}


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_round_trip_through_the_lossless_decoder(torch_mod, encoder, gpu_entropy):
    torch = torch_mod
    entries = [e for e in MANIFEST if e["kind"] == "random"][::3] + [e for e in MANIFEST if not e["stored"]]
    samples = [M.case_samples(e) for e in entries]
    statuses, files = encoder.encode([_tensor(torch, s, False) for s in samples], [e["precision"] for e in entries], [e["predictor"] for e in entries],
                                     [e["point_transform"] for e in entries], [e["restart_rows"] for e in entries])
    assert statuses == [0] * len(entries)
    dec = LL.BatchLosslessDecoder(device=0, num_threads=2, gpu_entropy=gpu_entropy)
    try:
        for e, s, data in zip(entries, samples, files):
            dst, outs = dec.decode([data], dtype=torch.uint8 if s.dtype == np.uint8 else torch.uint16)
            torch.cuda.synchronize()
            assert dst == [0], e["name"]
            got = outs[0].cpu()
            got = got.view(torch.int16).numpy().view(np.uint16) if s.dtype == np.uint16 else got.numpy()
            assert np.array_equal(got, M.expected(s, e["point_transform"])), e["name"]
    finally:
        dec.close()


def test_too_many_bits_for_uint32_offsets_is_unsupported_before_any_launch(torch_mod, encoder):
    x = N.LosslessEncodeInput()
    x.plane[0], x.pitch[0], x.sample_bytes, x.planar, x.width, x.height = 256, 24000, 2, 0, 12000, 12000  # never dereferenced
    statuses, files = M.encode_raw_batch(encoder, [(x, 1)], [16], [1], [0], [0])
    assert statuses == [3] and files == [None] and encoder.stats()["gpu_images"] == 0 and encoder.stats()["waits"] == 0


# ------------------------------------------------------------------------------------------------------------- plugin and Python API
def _plugin_encode(torch, samples, sample_format, encoding, precision=0, options="", dev=None, stream=None, encoder=None):
    """One image through nvimgcodecEncoderEncode of the host harness -> (processing status, file or None).  dev: the device tensor to code
    instead of an upload of `samples` (which then only give the shape); stream: the image's cuda_stream (default: the current stream's);
    encoder: an api.Encoder to use, and leave open, instead of one made here."""
    import contextlib
    import ctypes as C
    from nvimagecodec_amd import abi as A
    from nvimagecodec_amd import api
    from nvimagecodec_amd.api import _api, _check, _fill_image_info
    lib, inst = _api()
    s = M.as_hwn(samples)
    h, w, n = s.shape
    planar = sample_format in (A.SAMPLEFORMAT_P_Y, A.SAMPLEFORMAT_P_RGB, A.SAMPLEFORMAT_P_UNCHANGED)
    if dev is None:
        dev = _tensor(torch, s, planar)
    size = s.itemsize
    info = A.ImageInfo()
    _fill_image_info(info, h, w, n, sample_format, A.COLORSPEC_GRAY if n == 1 else A.COLORSPEC_SRGB, dev.data_ptr(), w * size * (1 if planar else n),
                     A.BUFFER_KIND_STRIDED_DEVICE, torch.cuda.current_stream().cuda_stream if stream is None else stream, planar=planar,
                     subsampling=A.SAMPLING_GRAY if n == 1 else A.SAMPLING_444)
    for p in range(info.num_planes):
        info.plane_info[p].sample_type = A.SAMPLE_DATA_TYPE_UINT16 if size == 2 else A.SAMPLE_DATA_TYPE_UINT8
        info.plane_info[p].precision = precision
    image = C.c_void_p()
    _check(lib.nvimgcodecImageCreate(inst, C.byref(image), C.byref(info)), "nvimgcodecImageCreate")
    out_info = A.ImageInfo()
    _fill_image_info(out_info, h, w, n, sample_format, info.color_spec, None, 0, A.BUFFER_KIND_STRIDED_HOST, None, subsampling=info.chroma_subsampling)
    out_info.codec_name = b"jpeg"
    ji = A.init(A.JpegImageInfo, A.ST_JPEG_IMAGE_INFO, encoding=encoding)
    out_info.struct_next = C.addressof(ji)
    sink = {"buf": None, "size": 0}

    def resize(ctx, nbytes):
        if sink["buf"] is None or nbytes > len(sink["buf"]):
            nb = C.create_string_buffer(nbytes)
            if sink["buf"] is not None:
                C.memmove(nb, sink["buf"], len(sink["buf"]))
            sink["buf"] = nb
        sink["size"] = nbytes
        return C.addressof(sink["buf"])

    cb = A.ResizeBufferFn(resize)
    cs = C.c_void_p()
    _check(lib.nvimgcodecCodeStreamCreateToHostMem(inst, C.byref(cs), None, cb, C.byref(out_info)), "nvimgcodecCodeStreamCreateToHostMem")
    ep = A.init(A.EncodeParams, A.ST_ENCODE_PARAMS, quality=90.0, target_psnr=50.0)
    fut = C.c_void_p()
    with (contextlib.nullcontext(encoder) if encoder is not None else api.Encoder(max_num_cpu_threads=2, options=options)) as enc:
        _check(lib.nvimgcodecEncoderEncode(enc._h, (C.c_void_p * 1)(image), (C.c_void_p * 1)(cs), 1, C.byref(ep), C.byref(fut)), "nvimgcodecEncoderEncode")
        _check(lib.nvimgcodecFutureWaitForAll(fut), "nvimgcodecFutureWaitForAll")
        st = (C.c_uint32 * 1)()
        count = C.c_size_t()
        lib.nvimgcodecFutureGetProcessingStatus(fut, st, C.byref(count))
        lib.nvimgcodecFutureDestroy(fut)
    data = C.string_at(sink["buf"], sink["size"]) if st[0] == A.PS_SUCCESS and sink["buf"] is not None else None
    lib.nvimgcodecImageDestroy(image)
    lib.nvimgcodecCodeStreamDestroy(cs)
    return st[0], data


def _golden(name):
    e = next(e for e in MANIFEST if e["name"] == name)
    return e, M.case_samples(e), open(os.path.join(GOLDEN, "lossless_encode", name + ".jpg"), "rb").read()


def test_plugin_route_writes_the_librarys_goldens(torch_mod):
    from nvimagecodec_amd import abi as A
    e, s, want = _golden("smooth_p8_c3")  # I_RGB uint8, stored as it is: what cjpeg -lossless writes from RGB
    assert (e["precision"], e["predictor"], e["point_transform"], e["restart_rows"]) == (8, 1, 0, 0)
    st, data = _plugin_encode(torch_mod, s, A.SAMPLEFORMAT_I_RGB, A.JPEG_ENCODING_LOSSLESS_HUFFMAN)
    assert st == A.PS_SUCCESS and data == want
    st, data = _plugin_encode(torch_mod, s, A.SAMPLEFORMAT_P_RGB, A.JPEG_ENCODING_LOSSLESS_HUFFMAN)
    assert st == A.PS_SUCCESS and data == want
    e, s, want = _golden("ssss16_p16")  # P_Y uint16
    assert (e["precision"], e["predictor"], e["point_transform"], e["restart_rows"], e["components"]) == (16, 1, 0, 0, 1)
    st, data = _plugin_encode(torch_mod, s, A.SAMPLEFORMAT_P_Y, A.JPEG_ENCODING_LOSSLESS_HUFFMAN)
    assert st == A.PS_SUCCESS and data == want
    # predictor, point transform and precision come from the options and from plane_info[0].precision
    e, s, want = _golden("one_row_p12")
    st, data = _plugin_encode(torch_mod, s, A.SAMPLEFORMAT_I_RGB, A.JPEG_ENCODING_LOSSLESS_HUFFMAN, precision=12,
                              options="hipjpeg_encoder:lossless_predictor=%d hipjpeg_encoder:lossless_point_transform=%d" % (e["predictor"], e["point_transform"]))
    assert st == A.PS_SUCCESS and data == want
    # a UINT16 image asked for as baseline is refused as before; BGR has no lossless meaning here
    st, data = _plugin_encode(torch_mod, s, A.SAMPLEFORMAT_I_RGB, A.JPEG_ENCODING_BASELINE_DCT)
    assert data is None and st & A.PS_SAMPLE_TYPE_UNSUPPORTED == A.PS_SAMPLE_TYPE_UNSUPPORTED
    st, data = _plugin_encode(torch_mod, s, A.SAMPLEFORMAT_I_BGR, A.JPEG_ENCODING_LOSSLESS_HUFFMAN)
    assert data is None and st & A.PS_SAMPLE_FORMAT_UNSUPPORTED == A.PS_SAMPLE_FORMAT_UNSUPPORTED


def test_api_encoder_lossless_decodes_back_through_api_decoder(torch_mod, tmp_path):
    from nvimagecodec_amd import api
    torch = torch_mod
    e, s, want = _golden("noisy_p16_c3")
    params = api.EncodeParams(jpeg_encode_params=api.JpegEncodeParams(lossless=True, predictor=e["predictor"]))
    assert api.JpegEncodeParams().lossless is False and api.JpegEncodeParams().predictor == 1 and api.JpegEncodeParams().point_transform == 0
    with api.Encoder(max_num_cpu_threads=2) as enc, api.Decoder(max_num_cpu_threads=2) as dec:
        data = enc.encode(_tensor(torch, s, False), params=params)
        # restart rows are the encoder's option, not a parameter: the golden has them, this file does not
        assert data == M.model_file(s, 16, e["predictor"], 0, 0)
        back = dec.decode(data, params=api.DecodeParams(allow_any_depth=True, color_spec=api.ColorSpec.UNCHANGED))
        got = back.cpu()._array
        assert got.dtype == np.uint16 and np.array_equal(got, s)
        # uint8 from host memory, 12 significant bits in uint16 with a point transform, and write()
        e8, s8, want8 = _golden("smooth_p8_c1")
        assert enc.encode(s8, params=api.EncodeParams(jpeg_encode_params=api.JpegEncodeParams(lossless=True))) == want8
        e12, s12, want12 = _golden("one_row_p12")
        p12 = api.EncodeParams(jpeg_encode_params=api.JpegEncodeParams(lossless=True, predictor=e12["predictor"], point_transform=e12["point_transform"]))
        path = str(tmp_path / "p12.jpg")
        assert enc.write(path, api.Image(_tensor(torch, s12, False), api.ImageBufferKind.STRIDED_DEVICE, precision=12), params=p12) == path
        assert open(path, "rb").read() == want12
        # defaults unchanged: the same uint8 picture without the flag is a DCT file
        plain = enc.encode(_tensor(torch, M.case_samples(next(x for x in MANIFEST if x["name"] == "smooth_p8_c3")), False))
        assert plain is not None and b"\xff\xc0" in plain[:700] and b"\xff\xc3" not in plain[:200]
