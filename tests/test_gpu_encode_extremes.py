"""The encode device stage (encode_kernels.hip) and the GPU entropy coders on saturated pixels and at the ends of the quality scale.

Every other encode test feeds synth_image pictures (pixels in 24..232, qualities 50..95) or compares one route of the product with
another.  Here every kernel form -- forward_pair_kernel interleaved and planar, the one-lane forward_kernel, forward_planes_kernel --
takes the pictures of helpers/extreme_images.py (flat 0 / 255, 1-pixel and 8-pixel checkerboards, the colour-conversion extremes side by
side, {0,255} random, full-range noise) at qualities 1, 50 and 100, and is compared with the CPU oracle alone: coefficients with
oracle.forward, whole files with oracle.encode, which tests/test_encode_extremes.py pins to libjpeg-turbo's files on this very content.
What that reaches: Cb / Cr of exactly 0 and 255 next to each other (the unmasked 4:4:4 chroma packing), row-pass outputs of -4096 (the
16-bit column pass's bound), DC = -1024 with divisor 8 and |AC| near 1023 (the quantizer's largest numerators), divisor 2040 (its largest
rounding error), DC differences of category 11 and blocks without a zero (the entropy coders' longest codes)."""
import functools
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers.extreme_images import PATTERNS, dqt_tables, extreme_image, extremes_reached

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "quant_tables_q1_100.json")) as _f:
    _QT = json.load(_f)["tables"]

SIZES = ((8, 8), (17, 13), (40, 24), (257, 66), (264, 70))  # one block, ragged edges, a small interior, one block past a 32-block tile
QUALITIES = (1, 50, 100)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def enc(torch_mod):
    """the device stage under test; entropy coding on the host (the GPU coders have their own tests below)"""
    from nvimagecodec_amd.lowlevel import BatchEncoder
    e = BatchEncoder(0, num_threads=4, gpu_huffman=False)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _image(pattern, w, h):
    im = extreme_image(pattern, w, h, seed=31 * w + h)
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def _ref(pattern, w, h, sub, q, gray=False):
    """(oracle.forward's coefficients, oracle.encode's file), computed once per case and shared by the tests"""
    rgb = _image(pattern, w, h)
    if gray:
        rgb = np.repeat(rgb[:, :, 1:2], 3, axis=2)
    return oracle.forward(rgb, sub, q)[0], oracle.encode(rgb, sub, q)


def _dev(torch, a):
    """a fresh contiguous copy on the device (the shared pictures stay read-only)"""
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def _cases():
    return [(p, w, h, q) for p in PATTERNS for (w, h) in SIZES for q in QUALITIES]


def _check(enc, streams, cases, sub, what, gray=False):
    for i, (p, w, h, q) in enumerate(cases):
        ref_coefs, ref_file = _ref(p, w, h, sub, q, gray)
        got = enc.coefficients(i)
        assert len(got) == len(ref_coefs)
        for c, (g, r) in enumerate(zip(got, ref_coefs)):
            rh, rw = g.shape[:2]
            assert np.array_equal(g, r[:rh, :rw]), f"{what}: {p} {w}x{h} {sub} q{q} component {c}"
        assert streams[i] == ref_file, f"{what}: {p} {w}x{h} {sub} q{q} file"


def _one_lane(enc, *args, **kw):
    os.environ["HIPJPEG_ENCODE_ONE_LANE_KERNEL"] = "1"
    try:
        return enc.encode(*args, **kw)
    finally:
        del os.environ["HIPJPEG_ENCODE_ONE_LANE_KERNEL"]


@pytest.mark.parametrize("sub", ["420", "422", "444"])
@pytest.mark.parametrize("fmt", ["rgb", "bgr"])
def test_pair_kernel_interleaved(enc, torch_mod, fmt, sub):
    """forward_pair_kernel<HS, VS, false>: contiguous tensors, and tight views at odd storage offsets (unaligned 8-byte fetches)"""
    torch = torch_mod
    cases = _cases()
    feed, tight = [], []
    for k, (p, w, h, q) in enumerate(cases):
        im = _image(p, w, h)
        src = _dev(torch, im[:, :, ::-1] if fmt == "bgr" else im)
        feed.append(src)
        buf = torch.zeros(h * w * 3 + 64, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(buf, (h, w, 3), (w * 3, 3, 1), storage_offset=(1, 3, 5, 7)[k % 4])
        view.copy_(src)
        tight.append(view)
    quals = [c[3] for c in cases]
    for what, vs in (("contiguous", feed), ("tight, odd offset", tight)):
        streams = enc.encode(vs, subsampling=sub, quality=quals, input_format=fmt)
        _check(enc, streams, cases, sub, f"pair kernel {fmt} {what}")


@pytest.mark.parametrize("sub", ["420", "422", "444"])
@pytest.mark.parametrize("fmt", ["rgb_planar", "bgr_planar"])
def test_pair_kernel_planar(enc, torch_mod, fmt, sub):
    """forward_pair_kernel<HS, VS, true>: CHW tensors"""
    torch = torch_mod
    cases = _cases()
    feed = [_dev(torch, (_image(p, w, h)[:, :, ::-1] if fmt == "bgr_planar" else _image(p, w, h)).transpose(2, 0, 1)) for (p, w, h, q) in cases]
    streams = enc.encode(feed, subsampling=sub, quality=[c[3] for c in cases], input_format=fmt)
    _check(enc, streams, cases, sub, f"pair kernel {fmt}")


@pytest.mark.parametrize("sub", ["440", "411", "410", "gray", "420", "422", "444"])
def test_one_lane_kernel(enc, torch_mod, sub):
    """forward_kernel: the samplings only it takes and gray input; 4:2:0 / 4:2:2 / 4:4:4 with HIPJPEG_ENCODE_ONE_LANE_KERNEL"""
    torch = torch_mod
    cases = _cases()
    quals = [c[3] for c in cases]
    if sub == "gray":
        feed = [_dev(torch, _image(p, w, h)[:, :, 1]) for (p, w, h, q) in cases]
        streams = enc.encode(feed, subsampling="gray", quality=quals, input_format="gray")
        _check(enc, streams, cases, "gray", "one-lane kernel, gray input", gray=True)
        return
    feed = [_dev(torch, _image(p, w, h)) for (p, w, h, q) in cases]
    if sub in ("420", "422", "444"):
        streams = _one_lane(enc, feed, subsampling=sub, quality=quals, input_format="rgb")
    else:
        streams = enc.encode(feed, subsampling=sub, quality=quals, input_format="rgb")
    _check(enc, streams, cases, sub, "one-lane kernel")


@pytest.mark.parametrize("sub,hs,vs", [("420", 2, 2), ("422", 2, 1), ("444", 1, 1)])
def test_planes_kernel(enc, torch_mod, sub, hs, vs):
    """forward_planes_kernel (yuv_planar): planes of 0, of 255, {0,255} random and full-range noise at ragged sizes, against
    oracle.forward_planes through the coefficients and tables of the file"""
    torch = torch_mod
    cases, planes = [], []
    for fill in ("black", "white", "random01", "noise"):
        for (w, h) in SIZES:
            cw, ch = (w + hs - 1) // hs, (h + vs - 1) // vs
            # three independent planes: channel k of a picture of the plane's size
            pl = [np.ascontiguousarray(extreme_image(fill, w, h, seed=w + h)[:, :, 0]),
                  np.ascontiguousarray(extreme_image(fill, cw, ch, seed=w + h + 1)[:, :, 1]),
                  np.ascontiguousarray(extreme_image(fill, cw, ch, seed=w + h + 2)[:, :, 2])]
            for q in QUALITIES:
                cases.append((fill, w, h, q))
                planes.append(pl)
    feed = [[torch.from_numpy(p).cuda() for p in pl] for pl in planes]
    streams = enc.encode(feed, subsampling=sub, quality=[c[3] for c in cases], input_format="yuv_planar")
    for (fill, w, h, q), pl, s in zip(cases, planes, streams):
        ref, (ql, qc) = oracle.forward_planes(pl, w, h, sub, q)
        got, qts = oracle.decode_coefficients(s)
        for c in range(3):
            assert np.array_equal(got[c], ref[c]), (fill, w, h, sub, q, c)
            assert np.array_equal(qts[c], ql if c == 0 else qc), (fill, w, h, sub, q, c)


@pytest.mark.parametrize("sub", ["444", "411"])
@pytest.mark.parametrize("pattern", ["noise", "random01"])
def test_quantizer_at_every_quality(enc, torch_mod, pattern, sub):
    """one 64x64 picture per quality 1..100: the multiply-high division by every divisor the tables hold (8 .. 2040) -- 4:4:4 through the
    pair kernel's quantizer (column_pass_quantize), 4:1:1 through the one-lane kernel's (fdct_quantize); {0,255} random has the largest
    numerators, noise the most varied ones"""
    torch = torch_mod
    quals = list(range(1, 101))
    imgs = [extreme_image(pattern, 64, 64, seed=900 + q) for q in quals]
    streams = enc.encode([torch.from_numpy(im).cuda() for im in imgs], subsampling=sub, quality=quals, input_format="rgb")
    for i, (im, q) in enumerate(zip(imgs, quals)):
        ref, _ = oracle.forward(im, sub, q)
        got = enc.coefficients(i)
        for c, (g, r) in enumerate(zip(got, ref)):
            assert np.array_equal(g, r[:g.shape[0], :g.shape[1]]), (pattern, sub, q, c)
        assert dqt_tables(streams[i]) == {0: _QT[str(q)]["luma"], 1: _QT[str(q)]["chroma"]}, (pattern, sub, q)
        assert streams[i] == oracle.encode(im, sub, q), (pattern, sub, q)


# ---- the GPU entropy coders on this content.  block_checker and primaries bring the DC differences of category 11, checker1 and stripes4
# the AC magnitudes of category 10 (838 and 924), {0,255} random and noise the blocks without a zero
_ENTROPY_CASES = [(p, w, h, sub, q) for p in ("block_checker", "primaries", "random01", "noise", "checker1", "stripes4") for (w, h) in ((40, 24), (264, 70))
                  for sub in ("420", "444") for q in (1, 100)]


@pytest.fixture(scope="module")
def coders(torch_mod):
    from nvimagecodec_amd.lowlevel import BatchEncoder
    gpu = BatchEncoder(0, num_threads=4, gpu_huffman=True, gpu_restart=True)
    host = BatchEncoder(0, num_threads=4, gpu_huffman=False)
    yield gpu, host
    gpu.close()
    host.close()


@pytest.fixture(scope="module")
def entropy_feed(torch_mod):
    return [_dev(torch_mod, _image(p, w, h)) for (p, w, h, sub, q) in _ENTROPY_CASES]


def _encode_entropy_cases(e, feed, **kw):
    return e.encode(feed, subsampling=[c[3] for c in _ENTROPY_CASES], quality=[c[4] for c in _ENTROPY_CASES], input_format="rgb", **kw)


def _assert_keeps_coefficients(stream, p, w, h, sub, q, what):
    ref, _ = _ref(p, w, h, sub, q)
    got, _ = oracle.decode_coefficients(stream)
    hs, vs = {"444": (1, 1), "420": (2, 2)}[sub]
    real = [((w + 7) // 8, (h + 7) // 8)] + [(((w + hs - 1) // hs + 7) // 8, ((h + vs - 1) // vs + 7) // 8)] * 2
    for c, ((rw, rh), g, r) in enumerate(zip(real, got, ref)):
        assert np.array_equal(g[:rh, :rw], r[:rh, :rw]), (what, p, w, h, sub, q, c)


def test_the_entropy_cases_reach_the_longest_codes():
    """what goes through each coder below: a DC difference of category 11 and AC magnitudes of category 10 (4:4:4 cases, where scan order
    is raster order; printed for the record)"""
    dc, ac, cbs, crs = extremes_reached([(_image(p, w, h), _ref(p, w, h, sub, q)[0]) for (p, w, h, sub, q) in _ENTROPY_CASES if sub == "444"])
    print(f"largest |DC difference| {dc}, largest |AC| {ac}")
    assert dc >= 1024 and ac >= 512
    assert {0, 255} <= cbs and {0, 255} <= crs


def test_gpu_coder_baseline(coders, entropy_feed):
    gpu, _ = coders
    streams = _encode_entropy_cases(gpu, entropy_feed)
    assert gpu.stats()["gpu_entropy_images"] == len(_ENTROPY_CASES)
    for (p, w, h, sub, q), s in zip(_ENTROPY_CASES, streams):
        assert s == _ref(p, w, h, sub, q)[1], (p, w, h, sub, q)


@pytest.mark.parametrize("interval", [1, 3])
def test_gpu_coder_restart_intervals(coders, entropy_feed, interval):
    gpu, _ = coders
    streams = _encode_entropy_cases(gpu, entropy_feed, restart_interval=interval)
    assert gpu.stats()["gpu_entropy_images"] == len(_ENTROPY_CASES)
    for (p, w, h, sub, q), s in zip(_ENTROPY_CASES, streams):
        assert s == oracle.encode(_image(p, w, h), sub, q, restart_interval=interval), (p, w, h, sub, q, interval)


@pytest.mark.parametrize("mode", ["optimized_huffman", "progressive"])
def test_gpu_coder_own_tables_and_progressive(coders, entropy_feed, mode):
    """the oracle writes neither: the files must decode to oracle.forward's coefficients and equal the host coder's byte for byte"""
    gpu, host = coders
    got = _encode_entropy_cases(gpu, entropy_feed, **{mode: True})
    assert gpu.stats()["gpu_entropy_images"] == len(_ENTROPY_CASES)
    want = _encode_entropy_cases(host, entropy_feed, **{mode: True})
    assert host.stats()["gpu_entropy_images"] == 0
    for (p, w, h, sub, q), g, wnt in zip(_ENTROPY_CASES, got, want):
        _assert_keeps_coefficients(g, p, w, h, sub, q, mode)
        assert g == wnt, (mode, p, w, h, sub, q)
        assert oracle.read_info(g)["sof"] == (0xC2 if mode == "progressive" else 0xC0)


def test_round_trip_through_the_gpu_decoder(coders, entropy_feed, torch_mod):
    """the quality-100 files of `primaries` and `block_checker` (every sample of the decode clamps or nearly does), decoded by the GPU
    decoder with either entropy stage: oracle.decode of the same bytes"""
    from nvimagecodec_amd.lowlevel import BatchDecoder
    gpu, _ = coders
    streams = _encode_entropy_cases(gpu, entropy_feed)
    files = [s for (p, w, h, sub, q), s in zip(_ENTROPY_CASES, streams) if q == 100 and p in ("primaries", "block_checker")]
    assert len(files) == 8
    dec = BatchDecoder(0, 4)
    try:
        for gpu_huffman in (False, True):
            outs, statuses = dec.decode(files, gpu_huffman=gpu_huffman)
            torch_mod.cuda.synchronize()
            assert list(statuses) == [0] * len(files)
            for f, o in zip(files, outs):
                assert np.array_equal(o.cpu().numpy(), oracle.decode(f))
    finally:
        dec.close()
