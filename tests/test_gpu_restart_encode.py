"""Restart-interval output on the GPU entropy coder (gpu_huffman_encode.hip, huffman_encode_core.h): with gpu_huffman and
gpu_restart every baseline image is coded on the device whatever its restart interval, and every file equals the host coder's --
itself pinned to libjpeg-turbo's files."""
import ctypes
import io
import re

import numpy as np
import pytest

import oracle
from nvimagecodec_amd.synth import synth_image
from test_restart_encode_algorithm import QUALITIES, SIZES, SUBS, intervals, mcu_grid

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
    gpu = BatchEncoder(0, num_threads=4, gpu_huffman=True, gpu_restart=True)
    host = BatchEncoder(0, num_threads=4, gpu_huffman=False)
    yield gpu, host
    gpu.close()
    host.close()


def _scan(jpeg):
    return jpeg[jpeg.index(b"\xff\xda"):]


def _same(gpu, host, feed, sub, q, fmt="rgb", rst=0, opt=False, what=None):
    want = host.encode(feed, sub, q, fmt, restart_interval=rst, optimized_huffman=opt)
    got = gpu.encode(feed, sub, q, fmt, restart_interval=rst, optimized_huffman=opt)
    assert gpu.stats()["gpu_entropy_images"] == len(feed), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, i)
    return want


@pytest.mark.parametrize("opt", [False, True], ids=["annex_k", "optimized"])
@pytest.mark.parametrize("q", QUALITIES)
def test_grid_in_mixed_shape_batches(encoders, torch_mod, q, opt):
    """Every sampling x size of the algorithm test in one batch per interval kind (0, 1, 2, 3, 7, one MCU row, the MCU count, more,
    65535): each image with its own interval."""
    gpu, host = encoders
    colour = [(sub, w, h) for sub in SUBS if sub != "gray" for (w, h) in SIZES]
    rgbs = [torch_mod.from_numpy(synth_image(w, h, seed=w * 7 + h)).cuda() for (_, w, h) in colour]
    grays = [torch_mod.from_numpy(np.ascontiguousarray(synth_image(w, h, seed=w * 7 + h)[:, :, 1])).cuda() for (w, h) in SIZES]
    for kind in range(9):
        _same(gpu, host, rgbs, [s for (s, _, _) in colour], q, "rgb", [intervals(w, h, s)[kind] for (s, w, h) in colour], opt, ("colour", kind))
        _same(gpu, host, grays, "gray", q, "gray", [intervals(w, h, "gray")[kind] for (w, h) in SIZES], opt, ("gray", kind))


def test_annex_k_files_are_libjpeg_turbos(encoders, torch_mod):
    gpu, _ = encoders
    for sub in SUBS:
        if sub == "gray":
            continue
        for (w, h) in SIZES:
            rgb = synth_image(w, h, seed=w * 7 + h)
            for r in intervals(w, h, sub):
                got = gpu.encode([torch_mod.from_numpy(rgb).cuda()], sub, 90, restart_interval=r)[0]
                assert got == oracle.encode(rgb, sub, 90, restart_interval=r), (sub, w, h, r)


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
        for opt in (False, True):
            want = _same(gpu, host, feed, sub, 90, fmt, r, opt, (fmt, r, opt))
            if fmt in ("rgb", "bgr", "rgb_planar", "bgr_planar", "yuv_planar") and not opt:
                assert want[0] == oracle.encode(rgb, "420", 90, restart_interval=r)


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_full_size_pictures(encoders, torch_mod, w, h):
    gpu, host = encoders
    torch = torch_mod
    row = mcu_grid(w, h, "420")[0]
    pic = torch.from_numpy(synth_image(w, h, seed=77)).cuda()
    noise = torch.from_numpy(np.random.default_rng(w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)).cuda()
    flat = torch.full((h, w, 3), 128, dtype=torch.uint8).cuda()
    for r in (1, row):
        for opt in (False, True):
            _same(gpu, host, [pic], "420", 90, "rgb", r, opt, ("picture", r, opt))
            _same(gpu, host, [flat], "420", 90, "rgb", r, opt, ("flat", r, opt))
            want = _same(gpu, host, [noise], "420", 100, "rgb", r, opt, ("noise", r, opt))
            assert _STUFFED_BEFORE_MARKER.search(_scan(want[0])), "the host coder's file has no stuffed 0xFF in front of a marker"
    if (w, h) == (1920, 1080):
        try:
            from PIL import Image
        except ImportError:
            pytest.skip("Pillow not available")
        im = synth_image(w, h, seed=77)
        for kw, r in ((dict(restart_marker_blocks=1), 1), (dict(restart_marker_rows=1), row)):
            b = io.BytesIO()
            Image.fromarray(im).save(b, "JPEG", quality=90, subsampling=2, **kw)
            assert gpu.encode([pic], "420", 90, restart_interval=r)[0] == b.getvalue(), kw


def test_mixed_batch_routes_by_flag(encoders, torch_mod):
    """Baseline, optimized, progressive, baseline + restart, optimized + restart, progressive + restart in one call: with both flags the
    GPU coder takes all but progressive + restart; with FLAG_GPU_HUFFMAN alone, the images without a restart interval as before."""
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
    got = run(gpu, N.FLAG_GPU_HUFFMAN | N.FLAG_GPU_RESTART_INTERVALS)
    assert gpu.stats()["gpu_entropy_images"] == sum(1 for i in range(len(imgs)) if not (kinds[i % 6][0] and kinds[i % 6][2]))
    assert got == want
    got = run(gpu, N.FLAG_GPU_HUFFMAN)
    assert gpu.stats()["gpu_entropy_images"] == sum(1 for i in range(len(imgs)) if kinds[i % 6][0] == 0)
    assert got == want
    assert run(gpu, N.FLAG_GPU_RESTART_INTERVALS) == want  # no meaning alone: the host coder's route


def test_submit_wait_three_batches_in_flight(encoders, torch_mod):
    gpu, host = encoders
    torch = torch_mod
    batches = [[torch.from_numpy(synth_image(97 + 16 * k, 61 + 8 * k, seed=10 * k + j)).cuda() for j in range(4)] for k in range(3)]
    rst = [[1, 2, 7, 0], [5, 0, 1, 3], [9, 1, 1, 65535]]
    want = [host.encode(b, "420", 88, restart_interval=r) for b, r in zip(batches, rst)]
    for b, r in zip(batches, rst):
        gpu.submit(b, "420", 88, restart_interval=r)
    for w in want:
        st, got = gpu.wait()
        assert st == [0] * len(w) and got == w
        assert gpu.stats()["gpu_entropy_images"] == len(w)


def _plugin_encode(api, dev, options, css=None, quality=90):
    params = api.EncodeParams(quality=quality, chroma_subsampling=css if css is not None else api.ChromaSubsampling.CSS_420)
    with api.Encoder(max_num_cpu_threads=2, options=options) as enc:
        return enc.encode([api.as_image(d) for d in dev], "jpeg", params)


def test_plugin_options(torch_mod):
    from nvimagecodec_amd import api, lowlevel
    shapes = [(200, 120), (64, 48), (333, 217)]
    imgs = [synth_image(w, h, seed=w) for (w, h) in shapes]
    dev = [torch_mod.from_numpy(i).cuda() for i in imgs]
    got = _plugin_encode(api, dev, "hipjpeg_encoder:restart_interval=5")
    assert got == _plugin_encode(api, dev, "hipjpeg_encoder:restart_interval=5 hipjpeg_encoder:gpu_huffman=0")
    for im, b in zip(imgs, got):
        assert lowlevel.get_image_info(b)["restart_interval"] == 5
        assert b == oracle.encode(im, "420", 90, restart_interval=5)
    # in MCU rows; wins over restart_interval
    for opts in ("hipjpeg_encoder:restart_rows=1", "hipjpeg_encoder:restart_interval=5 hipjpeg_encoder:restart_rows=1"):
        got = _plugin_encode(api, dev, opts)
        assert got == _plugin_encode(api, dev, opts + " hipjpeg_encoder:gpu_huffman=0")
        for (w, h), im, b in zip(shapes, imgs, got):
            assert lowlevel.get_image_info(b)["restart_interval"] == mcu_grid(w, h, "420")[0]
            assert b == oracle.encode(im, "420", 90, restart_interval=mcu_grid(w, h, "420")[0])
    # rows x MCUs per row beyond 65535: the interval is 65535 on both routes
    got = _plugin_encode(api, dev, "hipjpeg_encoder:restart_rows=65535")
    assert got == _plugin_encode(api, dev, "hipjpeg_encoder:restart_rows=65535 hipjpeg_encoder:gpu_huffman=0")
    assert [lowlevel.get_image_info(b)["restart_interval"] for b in got] == [65535] * len(got)
    # what does not parse or is out of range is ignored
    for opts in ("hipjpeg_encoder:restart_interval=70000", "hipjpeg_encoder:restart_interval=x", "hipjpeg_encoder:restart_rows=-1",
                 "hipjpeg_encoder:restart_interval=5x"):
        got = _plugin_encode(api, dev, opts)
        assert [lowlevel.get_image_info(b)["restart_interval"] for b in got] == [0] * len(got), opts
        assert got == [oracle.encode(im, "420", 90) for im in imgs]


def test_plugin_restart_rows_equals_pillow(torch_mod):
    from nvimagecodec_amd import api
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow not available")
    im = synth_image(640, 360, seed=8)
    b = io.BytesIO()
    Image.fromarray(im).save(b, "JPEG", quality=90, subsampling=2, restart_marker_rows=1)
    assert _plugin_encode(api, [torch_mod.from_numpy(im).cuda()], "hipjpeg_encoder:restart_rows=1")[0] == b.getvalue()


def test_round_trip_through_the_gpu_decoder(encoders, torch_mod):
    from nvimagecodec_amd.lowlevel import BatchDecoder
    gpu, _ = encoders
    shapes = [(320, 240, "420", 1), (123, 77, "444", 3), (640, 480, "422", 40), (250, 250, "420", 16)]
    feed = [torch_mod.from_numpy(synth_image(w, h, seed=w + h)).cuda() for (w, h, _, _) in shapes]
    for opt in (False, True):
        jpegs = gpu.encode(feed, [s for (_, _, s, _) in shapes], 90, restart_interval=[r for (_, _, _, r) in shapes], optimized_huffman=opt)
        assert gpu.stats()["gpu_entropy_images"] == len(shapes)
        dec = BatchDecoder(device=0, num_threads=2)
        outs, statuses = dec.decode(jpegs, fmt="rgb", gpu_huffman=True)
        torch_mod.cuda.synchronize()
        assert all(int(x) == 0 for x in statuses) and dec.stats()["gpu_entropy_images"] == len(jpegs)
        for j, o in zip(jpegs, outs):
            assert np.array_equal(o.cpu().numpy(), oracle.decode(j))
        dec.close()


def test_short_campaign(monkeypatch, capsys):
    """A short run of tests/campaigns/fuzz_restart_encode.py (random pictures, samplings, intervals and tables, GPU route against host coder)."""
    import os
    import runpy
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "campaigns", "fuzz_restart_encode.py")
    monkeypatch.setattr(sys, "argv", [script, "9", "3"])
    runpy.run_path(script, run_name="__main__")
    assert "every file equal to the host coder's" in capsys.readouterr().out.splitlines()[-1]
