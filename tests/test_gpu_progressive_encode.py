"""Progressive (SOF2) output on the GPU entropy coder (progressive_encode.hip): with gpu_huffman every progressive image without a
restart interval is coded on the device, and every file equals the host coder's -- itself pinned to libjpeg-turbo's files."""
import ctypes
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "manifest_encode_prog.json")) as _f:
    _MP = json.load(_f)["encode_progressive"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def encoders(torch_mod):
    from nvimagecodec_amd.lowlevel import BatchEncoder
    gpu, host = BatchEncoder(0, num_threads=4, gpu_huffman=True), BatchEncoder(0, num_threads=4, gpu_huffman=False)
    yield gpu, host
    gpu.close()
    host.close()


def _load(e):
    rgb = np.fromfile(os.path.join(GOLDEN, e["input"]), dtype=np.uint8).reshape(e["height"], e["width"], 3)
    with open(os.path.join(GOLDEN, "encode_prog", e["name"] + ".jpg"), "rb") as f:
        return rgb, f.read()


def test_restart_free_goldens_are_coded_on_the_device(encoders, torch_mod):
    gpu, _ = encoders
    for gray in (False, True):
        cases = [(e, *_load(e)) for e in _MP if e["restart"] == 0 and (e["sub"] == "gray") == gray]
        feed = [torch_mod.from_numpy(np.ascontiguousarray(c[1][:, :, 0] if gray else c[1])).cuda() for c in cases]
        out = gpu.encode(feed, subsampling=[c[0]["sub"] for c in cases], quality=[c[0]["quality"] for c in cases],
                         input_format="gray" if gray else "rgb", progressive=True)
        assert gpu.stats()["gpu_entropy_images"] == len(cases)
        for (e, _, jpeg), got in zip(cases, out):
            assert got == jpeg, e["name"]


def test_mixed_batch_routes_and_matches_the_host_coder(encoders, torch_mod):
    """One hipjpegEncodeBatchEntropy call over progressive, baseline, optimized and restart-interval images (baseline and
    progressive): the GPU coder takes every image without a restart interval, and every file equals the host coder's."""
    from nvimagecodec_amd import _native as N
    from nvimagecodec_amd.lowlevel import _enc_params
    gpu, host = encoders
    torch = torch_mod
    kinds = [(0, 0, 1), (0, 0, 0), (0, 1, 0), (2, 0, 0), (3, 0, 1)]  # (restart interval, optimized, progressive)
    imgs = [torch.from_numpy(synth_image(33 + 20 * k, 47 + 9 * k, seed=k)).cuda() for k in range(10)]

    def run(enc, flags):
        n = len(imgs)
        I, P = (N.EncodeInput * n)(), (N.EncodeParams * n)()
        for i, t in enumerate(imgs):
            I[i].plane[0], I[i].pitch[0], I[i].height, I[i].width = t.data_ptr(), t.stride(0), t.shape[0], t.shape[1]
            r, o, p = kinds[i % len(kinds)]
            P[i] = _enc_params("420", 80, "rgb", r, o, p)
        st = (ctypes.c_int * n)()
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert N.load().hipjpegEncodeBatchDevice(enc._h, I, P, n, st, s) == 0
        assert N.load().hipjpegEncodeBatchEntropy(enc._h, flags, st) == 0 and list(st) == [0] * n
        enc._n = n
        return enc.bitstreams()

    want = run(host, 0)
    got = run(gpu, N.FLAG_GPU_HUFFMAN)
    assert gpu.stats()["gpu_entropy_images"] == sum(1 for i in range(len(imgs)) if kinds[i % len(kinds)][0] == 0)
    assert got == want


def test_1080p_equals_pillow(encoders, torch_mod):
    gpu, _ = encoders
    im = synth_image(1920, 1080, seed=77)
    prog = gpu.encode([torch_mod.from_numpy(im).cuda()], "420", 90, progressive=True)[0]
    assert gpu.stats()["gpu_entropy_images"] == 1
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow not available")
    b = io.BytesIO()
    Image.fromarray(im).save(b, "JPEG", quality=90, subsampling=2, progressive=True)
    assert prog == b.getvalue()


def test_gray_yuv_4k_and_long_runs(encoders, torch_mod):
    """Gray input, P_YUV input, a 4K picture, and a flat picture of more than 32,767 luma blocks: the runs of its AC scans are cut
    at 0x7FFF on the device."""
    gpu, host = encoders
    torch = torch_mod
    from test_gpu_encode import _planes_like_libjpeg
    rgb = synth_image(320, 200, seed=3)
    g = torch.from_numpy(np.ascontiguousarray(rgb[:, :, 1])).cuda()
    assert gpu.encode([g], "gray", 90, input_format="gray", progressive=True) == host.encode([g], "gray", 90, input_format="gray", progressive=True)
    assert gpu.stats()["gpu_entropy_images"] == 1
    planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in _planes_like_libjpeg(rgb, 2, 2)]
    assert (gpu.encode([planes], "420", 90, input_format="yuv_planar", progressive=True) ==
            host.encode([planes], "420", 90, input_format="yuv_planar", progressive=True))
    assert gpu.stats()["gpu_entropy_images"] == 1
    big = torch.from_numpy(synth_image(3840, 2160, seed=9)).cuda()
    assert gpu.encode([big], "444", 95, progressive=True) == host.encode([big], "444", 95, progressive=True)
    flat = torch.full((1600, 1600, 3), 128, dtype=torch.uint8).cuda()  # 40,000 luma blocks, every AC coefficient zero
    for sub in ("420", "gray"):
        fmt = "gray" if sub == "gray" else "rgb"
        f = flat[:, :, 0].contiguous() if sub == "gray" else flat
        assert gpu.encode([f], sub, 75, input_format=fmt, progressive=True) == host.encode([f], sub, 75, input_format=fmt, progressive=True)
        assert gpu.stats()["gpu_entropy_images"] == 1


def test_submit_wait_three_batches_in_flight(encoders, torch_mod):
    gpu, _ = encoders
    torch = torch_mod
    batches = [[torch.from_numpy(synth_image(97 + 16 * k, 61 + 8 * k, seed=10 * k + j)).cuda() for j in range(4)] for k in range(3)]
    want = [gpu.encode(b, "420", 88, progressive=True) for b in batches]
    for b in batches:
        gpu.submit(b, "420", 88, progressive=True)
    for w in want:
        st, got = gpu.wait()
        assert st == [0] * len(w) and got == w


def test_plugin_progressive_output_equals_the_host_coders(torch_mod):
    from nvimagecodec_amd import api
    dev = torch_mod.from_numpy(synth_image(200, 120, seed=4)).cuda()
    params = api.EncodeParams(quality=90, chroma_subsampling=api.ChromaSubsampling.CSS_420, jpeg_encode_params=api.JpegEncodeParams(progressive=True))
    out = []
    for opts in ("", "hipjpeg_encoder:gpu_huffman=0"):
        with api.Encoder(max_num_cpu_threads=2, options=opts) as enc:
            out.append(enc.encode(api.as_image(dev), "jpeg", params))
    assert out[0] is not None and b"\xff\xc2" in out[0][:700] and out[0] == out[1]
