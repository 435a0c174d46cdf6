"""Progressive output with restart intervals on the GPU entropy coder (progressive_encode.hip, the RST flavour of its kernels): with
gpu_huffman and gpu_progressive_restart every progressive image is coded on the device whatever its restart interval, and every file
equals the host coder's -- itself pinned to libjpeg-turbo's files (jcphuff.c emit_restart)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from nvimagecodec_amd.synth import synth_image
from test_restart_encode_algorithm import SIZES, SUBS, intervals, mcu_grid

pytestmark = pytest.mark.gpu

_STUFFED_BEFORE_MARKER = re.compile(rb"\xff\x00\xff[\xd0-\xd7]")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def encoders(torch_mod):
    from nvimagecodec_amd.lowlevel import BatchEncoder
    gpu = BatchEncoder(0, num_threads=4, gpu_huffman=True, gpu_progressive_restart=True)
    host = BatchEncoder(0, num_threads=4, gpu_huffman=False)
    yield gpu, host
    gpu.close()
    host.close()


def _same(gpu, host, feed, sub, q, fmt="rgb", rst=0, what=None):
    want = host.encode(feed, sub, q, fmt, restart_interval=rst, progressive=True)
    got = gpu.encode(feed, sub, q, fmt, restart_interval=rst, progressive=True)
    assert gpu.stats()["gpu_entropy_images"] == len(feed), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, i)
    return want


@pytest.mark.parametrize("q", [50, 100])
def test_grid_in_mixed_shape_batches(encoders, torch_mod, q):
    """Every sampling x size of the algorithm test in one batch per interval kind (0, 1, 2, 3, 7, one MCU row, the MCU count, more,
    65535): each image with its own interval."""
    gpu, host = encoders
    colour = [(sub, w, h) for sub in SUBS if sub != "gray" for (w, h) in SIZES]
    rgbs = [torch_mod.from_numpy(synth_image(w, h, seed=w * 7 + h)).cuda() for (_, w, h) in colour]
    grays = [torch_mod.from_numpy(np.ascontiguousarray(synth_image(w, h, seed=w * 7 + h)[:, :, 1])).cuda() for (w, h) in SIZES]
    for kind in range(9):
        _same(gpu, host, rgbs, [s for (s, _, _) in colour], q, "rgb", [intervals(w, h, s)[kind] for (s, w, h) in colour], ("colour", kind))
        _same(gpu, host, grays, "gray", q, "gray", [intervals(w, h, "gray")[kind] for (w, h) in SIZES], ("gray", kind))


def test_intervals_0_1_and_one_row_in_one_call(encoders, torch_mod):
    """The RST flavour of the kernels meets scans with rst_blocks == 0."""
    gpu, host = encoders
    shapes = [(97, 61), (64, 48), (200, 120), (33, 65), (320, 208), (17, 13)]
    imgs = [torch_mod.from_numpy(synth_image(w, h, seed=w + h)).cuda() for (w, h) in shapes]
    rst = [(0, 1, mcu_grid(w, h, "420")[0])[i % 3] for i, (w, h) in enumerate(shapes)]
    assert rst.count(0) == 2 and rst.count(1) == 2
    _same(gpu, host, imgs, "420", 85, "rgb", rst, "mixed intervals")


def test_golden_files_are_libjpeg_turbos(encoders, torch_mod):
    """The three goldens with a restart interval (4:2:0 r = 7, 4:4:4 r = 1, gray r = 5), one call."""
    gpu, _ = encoders
    with open(os.path.join(GOLDEN, "manifest_encode_prog.json")) as f:
        entries = [e for e in json.load(f)["encode_progressive"] if e["restart"]]
    assert len(entries) == 3
    for e in entries:
        rgb = np.fromfile(os.path.join(GOLDEN, e["input"]), dtype=np.uint8).reshape(e["height"], e["width"], 3)
        gray = e["sub"] == "gray"
        feed = torch_mod.from_numpy(np.ascontiguousarray(rgb[:, :, 0]) if gray else rgb).cuda()  # gray inputs hold the plane three times
        got = gpu.encode([feed], e["sub"], e["quality"], "gray" if gray else "rgb", restart_interval=e["restart"], progressive=True)[0]
        assert gpu.stats()["gpu_entropy_images"] == 1
        with open(os.path.join(GOLDEN, "encode_prog", e["name"] + ".jpg"), "rb") as f:
            assert got == f.read(), e["name"]


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "rgb_planar", "bgr_planar", "gray", "yuv_planar"])
def test_every_forward_kernel(encoders, torch_mod, fmt):
    from test_gpu_encode import _planes_like_libjpeg
    gpu, host = encoders
    torch = torch_mod
    rgb = synth_image(320, 208, seed=21)
    if fmt == "rgb":
        feed = [torch.from_numpy(rgb).cuda()]
    elif fmt == "bgr":
        feed = [torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])).cuda()]
    elif fmt == "rgb_planar":
        feed = [torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))).cuda()]
    elif fmt == "bgr_planar":
        feed = [torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1].transpose(2, 0, 1))).cuda()]
    elif fmt == "gray":
        feed = [torch.from_numpy(np.ascontiguousarray(rgb[:, :, 1])).cuda()]
    else:
        feed = [[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in _planes_like_libjpeg(rgb, 2, 2)]]
    sub = "gray" if fmt == "gray" else "420"
    for r in (1, 3, mcu_grid(320, 208, sub)[0]):
        _same(gpu, host, feed, sub, 90, fmt, r, (fmt, r))


def test_fast_path_of_the_run_walk_meets_interval_ends(encoders, torch_mod):
    """A flat gray 1024 x 1024: 16,384 empty blocks per AC scan, which the runs kernel takes 64 at a time -- except where one of the
    64 ends an interval; 100 is no multiple of 64, so the interval ends fall on every position of a step."""
    gpu, host = encoders
    flat = torch_mod.full((1024, 1024), 128, dtype=torch_mod.uint8).cuda()
    _same(gpu, host, [flat], "gray", 90, "gray", 100, "flat, r = 100")


def test_run_cut_at_0x7fff_inside_an_interval(encoders, torch_mod):
    """A flat gray 1472 x 1472: 33,856 empty blocks per AC scan and r = 33000: the run is cut at 0x7FFF, the interval end flushes the
    rest, the scan's end the last 856."""
    gpu, host = encoders
    flat = torch_mod.full((1472, 1472), 128, dtype=torch_mod.uint8).cuda()
    _same(gpu, host, [flat], "gray", 90, "gray", 33000, "flat, r = 33000")


def test_noise_at_quality_100(encoders, torch_mod):
    """Stuffed FF bytes next to unstuffed markers; several 4 KB chunks and 256-block units per scan."""
    gpu, host = encoders
    noise = torch_mod.from_numpy(np.random.default_rng(640).integers(0, 256, size=(480, 640, 3), dtype=np.uint8)).cuda()
    for r in (1, mcu_grid(640, 480, "420")[0]):
        want = _same(gpu, host, [noise], "420", 100, "rgb", r, ("noise", r))
        scans = want[0].split(b"\xff\xda")[1:]
        assert any(_STUFFED_BEFORE_MARKER.search(s) for s in scans), "the host coder's file has no stuffed 0xFF in front of a marker"
        assert max(len(s) for s in scans) > 3 * 4096


def test_mixed_batch_routes_by_flag(encoders, torch_mod):
    """The six kinds of test_gpu_restart_encode.py::test_mixed_batch_routes_by_flag in one call: FLAG_GPU_HUFFMAN |
    FLAG_GPU_PROGRESSIVE_RESTART takes all but baseline + restart; all three flags take every image; the new flag alone means nothing."""
    from nvimagecodec_amd import _native as N
    from nvimagecodec_amd.lowlevel import _enc_params
    gpu, host = encoders
    torch = torch_mod
    kinds = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (3, 1, 0), (3, 0, 1)]  # (restart interval, optimized, progressive)
    imgs = [torch.from_numpy(synth_image(33 + 20 * k, 47 + 9 * k, seed=k)).cuda() for k in range(12)]

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
    got = run(gpu, N.FLAG_GPU_HUFFMAN | N.FLAG_GPU_PROGRESSIVE_RESTART)
    assert gpu.stats()["gpu_entropy_images"] == sum(1 for i in range(len(imgs)) if not (kinds[i % 6][0] and not kinds[i % 6][2])) == 8
    assert got == want
    got = run(gpu, N.FLAG_GPU_HUFFMAN | N.FLAG_GPU_RESTART_INTERVALS | N.FLAG_GPU_PROGRESSIVE_RESTART)
    assert gpu.stats()["gpu_entropy_images"] == len(imgs)
    assert got == want
    assert run(gpu, N.FLAG_GPU_PROGRESSIVE_RESTART) == want  # no meaning alone: the host coder's route


def test_submit_wait_three_batches_in_flight(encoders, torch_mod):
    gpu, host = encoders
    torch = torch_mod
    batches = [[torch.from_numpy(synth_image(97 + 16 * k, 61 + 8 * k, seed=10 * k + j)).cuda() for j in range(4)] for k in range(3)]
    rst = [[1, 2, 7, 0], [5, 0, 1, 3], [9, 1, 1, 65535]]
    want = [host.encode(b, "420", 88, restart_interval=r, progressive=True) for b, r in zip(batches, rst)]
    for b, r in zip(batches, rst):
        gpu.submit(b, "420", 88, restart_interval=r, progressive=True)
    for w in want:
        st, got = gpu.wait()
        assert st == [0] * len(w) and got == w
        assert gpu.stats()["gpu_entropy_images"] == len(w)


def test_transcoder_and_coefficient_tensors(torch_mod):
    """hipjpegTranscodeBatch and hipjpegEncodeCoefficientsBatch honour the flag: a progressive target with restart_interval = 3 is
    coded on the device, and the bytes are transcode_host's."""
    from nvimagecodec_amd import lowlevel
    sources = [oracle.encode(synth_image(w, h, seed=w), sub, 85) for (w, h, sub) in ((200, 120, "420"), (97, 61, "444"), (64, 48, "gray"))]
    want = [lowlevel.transcode_host(s, progressive=True, restart_interval=3) for s in sources]
    for on in (True, False):
        t = lowlevel.BatchTranscoder(device=0, num_threads=4, gpu_huffman=True, gpu_progressive_restart=on)
        try:
            statuses, files = t.transcode(sources, progressive=True, restart_interval=3)
            assert statuses == [0] * len(sources) and files == want
            assert t.stats()["gpu_coded_images"] == (len(sources) if on else 0)
        finally:
            t.close()
        c = lowlevel.BatchCoefficients(device=0, num_threads=4, gpu_huffman=True, gpu_progressive_restart=on)
        try:
            statuses, images = c.decode(sources)
            assert statuses == [0] * len(sources)
            statuses, files = c.encode(images, progressive=True, restart_interval=3)
            assert statuses == [0] * len(sources) and files == want
            assert c.stats()["gpu_coded_images"] == (len(sources) if on else 0)
        finally:
            c.close()


def test_plugin_option(torch_mod):
    from nvimagecodec_amd import api, lowlevel
    shapes = [(200, 120), (64, 48), (333, 217)]
    dev = [torch_mod.from_numpy(synth_image(w, h, seed=w)).cuda() for (w, h) in shapes]
    params = api.EncodeParams(quality=90, chroma_subsampling=api.ChromaSubsampling.CSS_420, jpeg_encode_params=api.JpegEncodeParams(progressive=True))
    out = []
    for opts in ("hipjpeg_encoder:restart_rows=1 hipjpeg_encoder:gpu_progressive_restart=1", "hipjpeg_encoder:restart_rows=1",
                 "hipjpeg_encoder:restart_rows=1 hipjpeg_encoder:gpu_huffman=0"):
        with api.Encoder(max_num_cpu_threads=2, options=opts) as enc:
            out.append(enc.encode([api.as_image(d) for d in dev], "jpeg", params))
    assert out[0] == out[1] == out[2]
    for (w, h), b in zip(shapes, out[0]):
        assert b is not None and b"\xff\xc2" in b[:700]
        assert lowlevel.get_image_info(b)["restart_interval"] == mcu_grid(w, h, "420")[0]
