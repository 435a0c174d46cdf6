"""Decoding at 1/2, 1/4 and 1/8 scale on the GPU (hipjpegDecodeBatchSetScales), pinned bit for bit to libjpeg-turbo driven through its C
API with scale_denom set (tests/golden/manifest_scaled.json, tests/golden/make_golden_scaled.py): every decode golden, every sampling
layout, the 43 out-of-gamut vectors and the tiny files of tests/golden/scaled, at every denominator, with ISLOW and IFAST, fancy and plain
upsampling, through the host and the GPU entropy stage.  Four-component frames and the layouts the library itself refuses report
UNSUPPORTED."""
import ctypes as C

import numpy as np
import pytest

from helpers import scaled_goldens as S
from helpers.geometry import upright
from nvimagecodec_amd import _native as N

pytestmark = pytest.mark.gpu

_JPEGS = {}


def _jpeg(e):
    if e["name"] not in _JPEGS:
        _JPEGS[e["name"]] = S.jpeg(e)
    return _JPEGS[e["name"]]


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


def _cpu(o):
    import torch
    torch.cuda.synchronize()
    return None if o is None else o.cpu().numpy()


# more than 10 blocks per MCU: the header parser's BAD_JPEG, at every scale (see _check)
_PARSER_REFUSES = {"y42c21_83x61": 2, "y24c12_83x61": 2}


def _check(entries, denoms, outs, statuses, ifast=False, fancy=True, what=""):
    """Every image: the manifest's hash, or UNSUPPORTED where the library refuses the (file, denominator) and for four-component frames.
    One departure from "refused means UNSUPPORTED": two of the three layouts the library refuses (more than 10 blocks per MCU) never get
    past the header parser, which calls them BAD_JPEG at full size too (tests/test_sampling_layouts.py pins that); a scale does not change
    the parser's verdict, so those two files, by name, must report BAD_JPEG at every scale.  Every other refused entry, the third layout
    (a fractional ratio) among them, must be UNSUPPORTED."""
    for e, d, o, s in zip(entries, denoms, outs, statuses):
        want_status, want = S.expected(e, d, ifast, fancy)
        if e["name"] in _PARSER_REFUSES:
            assert want_status == S.UNSUPPORTED and want is None
            want_status = _PARSER_REFUSES[e["name"]]
        assert s == want_status, (what, e["name"], d, s)
        if want is not None:
            got = _cpu(o)
            sc = e["scales"][str(d)]
            assert got.shape == (sc["height"], sc["width"], 3), (what, e["name"], d, got.shape)
            assert S.sha(got) == want, (what, e["name"], d)


# ---- 1. parity: one batch of ALL manifest files per setting
@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
@pytest.mark.parametrize("ifast", [False, True], ids=["islow", "ifast"])
@pytest.mark.parametrize("fancy", [True, False], ids=["fancy", "plain"])
@pytest.mark.parametrize("denom", S.DENOMS)
def test_every_file_equals_libjpeg_turbo(dec, denom, fancy, ifast, gpu_huffman):
    jpegs = [_jpeg(e) for e in S.FILES]
    outs, st = dec.decode(jpegs, fmt="rgb", fancy=fancy, fast_idct=ifast, gpu_huffman=gpu_huffman, scales=[denom] * len(jpegs), check=False)
    assert len(S.FILES) == 310 and sum(1 for e in S.FILES if e["set"] == "gamut") == 43
    _check(S.FILES, [denom] * len(jpegs), outs, st, ifast, fancy)
    if gpu_huffman:
        assert dec.stats()["gpu_entropy_images"] > 100


# ---- 2. denominators 1, 2, 4, 8 interleaved in one batch
@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
def test_mixed_batch(dec, gpu_huffman):
    entries = [e for e in S.FILES if e["set"] in ("decode", "scaled") and e["name"] != "c2_1920x1080_420_base_q90"][::3]
    jpegs = [_jpeg(e) for e in entries]
    denoms = [(1, 2, 4, 8)[i % 4] for i in range(len(jpegs))]
    plain, st0 = dec.decode(jpegs, fmt="rgb", gpu_huffman=gpu_huffman)
    plain = [_cpu(o).copy() for o in plain]
    outs, st = dec.decode(jpegs, fmt="rgb", gpu_huffman=gpu_huffman, scales=denoms)
    for e, d, o, p in zip(entries, denoms, outs, plain):
        if d == 1:
            assert np.array_equal(_cpu(o), p), e["name"]
        else:
            assert S.sha(_cpu(o)) == S.expected(e, d)[1], (e["name"], d)


# ---- 3. the other output formats
_TINY = [e for e in S.FILES if e["set"] == "scaled"]


@pytest.mark.parametrize("denom", S.DENOMS)
def test_formats_are_rearrangements_of_rgb(dec, denom):
    """bgr / planar: the channels of the interleaved RGB result (test 1 pins it).  y: the library's own JCS_GRAYSCALE decode at the scale,
    which the generator records for the scaled/ set ("y_sha256") -- for gray AND colour files."""
    jpegs = [_jpeg(e) for e in _TINY]
    scales = [denom] * len(jpegs)
    rgb = [_cpu(o).copy() for o in dec.decode(jpegs, fmt="rgb", scales=scales)[0]]
    for gh in (False, True):
        for fmt, view in (("bgr", lambda a: a[:, :, ::-1]), ("rgb_planar", lambda a: a.transpose(2, 0, 1)), ("bgr_planar", lambda a: a[:, :, ::-1].transpose(2, 0, 1))):
            outs, _ = dec.decode(jpegs, fmt=fmt, scales=scales, gpu_huffman=gh)
            for e, o, r in zip(_TINY, outs, rgb):
                assert np.array_equal(_cpu(o), view(r)), (e["name"], fmt, gh)
        outs, _ = dec.decode(jpegs, fmt="y", scales=scales, gpu_huffman=gh)
        for e, o in zip(_TINY, outs):
            assert S.sha(_cpu(o)) == e["scales"][str(denom)]["y_sha256"], (e["name"], gh)


# ---- 4. geometry: regions and the eight orientations, in scaled-picture coordinates
@pytest.mark.parametrize("denom", S.DENOMS)
def test_regions_and_orientations(dec, denom):
    """Expected: the window of the untransformed scaled pixels (test 1 pins them), brought upright by tests/helpers/geometry.py."""
    names = [e["name"] for e in S.FILES if e["name"].startswith("t33x17_")] + ["h130x70_420_opt_q75", "h130x70_444_opt_q75", "r130x70_420_prog_rst7"]
    entries = [S.by_name(n) for n in names]
    jpegs = [_jpeg(e) for e in entries]
    scales = [denom] * len(jpegs)
    full = [_cpu(o).copy() for o in dec.decode(jpegs, fmt="rgb", scales=scales)[0]]
    for gh in (False, True):
        for orientation in range(1, 9):
            transforms = []
            for k, f in enumerate(full):
                H, W = f.shape[:2]
                # whole picture, an inner window, a corner window, one pixel -- in turn
                roi = [None, (W // 4, H // 4, W - W // 4 or 1, H - H // 4 or 1), (max(W - 3, 0), max(H - 2, 0), W, H), (0, 0, 1, 1)][(k + orientation) % 4]
                if roi is not None and (roi[2] <= roi[0] or roi[3] <= roi[1]):
                    roi = None
                transforms.append((roi, orientation))
            for fmt in ("rgb", "bgr_planar"):
                outs, _ = dec.decode(jpegs, fmt=fmt, scales=scales, transforms=transforms, gpu_huffman=gh)
                for e, o, f, (roi, _) in zip(entries, outs, full, transforms):
                    x0, y0, x1, y1 = roi or (0, 0, f.shape[1], f.shape[0])
                    want = upright(f[y0:y1, x0:x1], orientation)
                    if fmt == "bgr_planar":
                        want = want[:, :, ::-1].transpose(2, 0, 1)
                    assert np.array_equal(_cpu(o), want), (e["name"], orientation, roi, fmt, gh)
    # a region that fits the full-size picture only is outside the scaled one
    _, st = dec.decode(jpegs[-1:], fmt="rgb", scales=[denom], transforms=[((0, 0, 130, 70), 1)], check=False, outs=dec.allocate_outputs(jpegs[-1:]))
    assert st == [S.INVALID_ARGUMENT]


# ---- 5. refusals and plumbing
def test_refusals_and_plumbing(dec):
    import torch
    lib = N.load()
    good = S.by_name("h130x70_420_opt_q75")
    j = _jpeg(good)
    cmyk = next(e for e in S.FILES if e.get("components") == 4)
    # raw planes and four components at a scale: UNSUPPORTED; at denominator 1 both decode as before
    outs = dec.allocate_outputs([j], fmt="yuv_planar")
    assert dec.decode([j], fmt="yuv_planar", outs=outs, scales=[2], check=False)[1] == [S.UNSUPPORTED]
    assert dec.decode([j], fmt="yuv_planar", outs=outs, scales=[1], check=False)[1] == [S.SUCCESS]
    assert dec.decode([_jpeg(cmyk), j], fmt="rgb", scales=[2, 2], check=False)[1] == [S.UNSUPPORTED, S.SUCCESS]
    assert dec.decode([_jpeg(cmyk)], fmt="rgb", scales=[1], check=False)[1] == [S.SUCCESS]
    # a denominator that is none of 1, 2, 4, 8: that image alone
    outs = dec.allocate_outputs([j] * 4, scales=[2, 1, 1, 8])
    _, st = dec.decode([j] * 4, outs=outs, scales=[2, 3, 0, 8], check=False)
    assert st == [S.SUCCESS, S.INVALID_ARGUMENT, S.INVALID_ARGUMENT, S.SUCCESS]
    assert S.sha(_cpu(outs[0])) == S.expected(good, 2)[1] and S.sha(_cpu(outs[3])) == S.expected(good, 8)[1]
    # a count that differs from the batch's size fails the call and drops the scales ...
    dec.set_scales([2, 2, 2], 3)
    with pytest.raises(N.HipJpegError):
        dec.decode([j, j])
    # ... and scales are consumed by one batch: the next is a full-size decode
    full = _cpu(dec.decode([j])[0][0]).copy()
    assert full.shape == (70, 130, 3)
    half, _ = dec.decode([j], scales=[2])
    again, _ = dec.decode([j])
    assert _cpu(half[0]).shape == (35, 65, 3) and np.array_equal(_cpu(again[0]), full)
    # NULL takes them back
    dec.set_scales([2], 1)
    dec.set_scales(None, 0)
    assert np.array_equal(_cpu(dec.decode([j])[0][0]), full)
    # the three batch calls that take no scales refuse pending ones (before they look at anything else) and drop them
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    calls = (lambda: lib.hipjpegTranscodeBatch(dec._h, None, None, 0, None, 0, None, stream),
             lambda: lib.hipjpegDecodeCoefficientsBatch(dec._h, None, None, 0, None, 0, None, stream),
             lambda: lib.hipjpegCoefficientsToPixelsBatch(dec._h, None, None, 0, None, 0, 0, None, stream))
    for call in calls:
        dec.set_scales([2, 2, 2], 3)
        assert call() == S.INVALID_ARGUMENT
        # (were the three scales still pending, this batch of one would be refused for its count)
        assert np.array_equal(_cpu(dec.decode([j])[0][0]), full)


# ---- 6. damaged neighbours through the GPU entropy stage
def test_damaged_files_beside_good_ones(dec):
    import os
    import random
    good = [S.by_name(n) for n in ("h130x70_420_opt_q75", "h320x200_444_opt_q75", "c4_1280x720_422_base_q90", "h320x200_gray_opt_q98")]
    with open(os.path.join(S.GOLDEN, "damaged", "padding_block_damage.jpg"), "rb") as f:
        damaged = [f.read()]
    rng = random.Random(11)
    for e in good[:3]:  # bit flips inside the entropy-coded data
        b = bytearray(_jpeg(e))
        sos = bytes(b).rfind(b"\xff\xda")
        for _ in range(3):
            k = rng.randrange(sos + 20, len(b) - 2)
            b[k] ^= 1 << rng.randrange(8)
            if b[k] == 0xFF:
                b[k] = 0xFE
        damaged.append(bytes(b))
        damaged.append(_jpeg(e)[:len(b) // 2])  # and a truncated one
    batch, entries = [], []
    for i, d in enumerate(damaged):
        batch += [_jpeg(good[i % 4]), d]
        entries += [good[i % 4], None]
    _, st_full = dec.decode(batch, fmt="rgb", gpu_huffman=True, check=False)
    outs, st = dec.decode(batch, fmt="rgb", gpu_huffman=True, check=False, scales=[2] * len(batch))
    assert st == st_full and any(s != 0 for s in st)
    assert dec.stats()["gpu_entropy_images"] > 0
    for e, o, s in zip(entries, outs, st):
        if e is not None:
            assert s == 0 and S.sha(_cpu(o)) == S.expected(e, 2)[1], e["name"]
    # the host entropy stage agrees on the statuses, and on the pixels of what decodes
    outs_h, st_h = dec.decode(batch, fmt="rgb", gpu_huffman=False, check=False, scales=[2] * len(batch))
    assert st_h == st
    for a, b, s in zip(outs, outs_h, st):
        if s == 0:
            assert np.array_equal(_cpu(a), _cpu(b))


# ---- 7. Submit / Wait three deep
def test_submit_wait_three_deep(dec):
    entries = [e for e in S.FILES if e["set"] in ("scaled", "gamut")]
    jpegs = [_jpeg(e) for e in entries]
    batches = []
    for denom in S.DENOMS:
        scales = [denom] * len(jpegs)
        outs = dec.allocate_outputs(jpegs, scales=scales)
        dec.submit(jpegs, outs, gpu_huffman=True, scales=scales)
        batches.append((denom, outs))
    for denom, outs in batches:
        st = dec.wait(check=False)
        _check(entries, [denom] * len(jpegs), outs, st, what="submit")


# ---- 7b. the plugin option, the Python API and the command line tool
@pytest.mark.parametrize("denom", S.DENOMS)
def test_plugin_option_through_the_host_harness(denom):
    """hipjpeg_decoder:scale_denom=N through nvimgcodecDecoderDecode of the host harness: the caller's image has the scaled size; raw
    planes are declined (SAMPLE_FORMAT_UNSUPPORTED)."""
    import torch
    from nvimagecodec_amd import abi as A
    from test_gpu_plugin import _c_api_decode, _setup
    lib = A.bind(N.load_host())
    inst, d = _setup(lib, options=b"hipjpeg_decoder:scale_denom=%d" % denom)
    for name in ("h130x70_420_opt_q75", "t17x9_422_prog"):
        e = S.by_name(name)
        sc = e["scales"][str(denom)]
        h, w = sc["height"], sc["width"]
        buf = np.zeros((h, w, 3), dtype=np.uint8)
        assert _c_api_decode(lib, inst, d, _jpeg(e), h, w, A.SAMPLEFORMAT_I_RGB, 1, 3, buf.ctypes.data, w * 3, A.BUFFER_KIND_STRIDED_HOST) == A.PS_SUCCESS
        torch.cuda.synchronize()
        assert S.sha(buf) == sc["rgb_sha256"], (name, denom)
        planes = np.zeros((3, h, w), dtype=np.uint8)
        st = _c_api_decode(lib, inst, d, _jpeg(e), h, w, A.SAMPLEFORMAT_P_YUV, 3, 1, planes.ctypes.data, w, A.BUFFER_KIND_STRIDED_HOST)
        assert st != A.PS_SUCCESS and (st & A.PS_SAMPLE_FORMAT_UNSUPPORTED) == A.PS_SAMPLE_FORMAT_UNSUPPORTED, hex(st)
    lib.nvimgcodecDecoderDestroy(d)
    lib.nvimgcodecInstanceDestroy(inst)


@pytest.mark.parametrize("options,denom", [(":scale_denom=2", 2), ("hipjpeg_decoder:scale_denom=8", 8), (":fancy_upsampling=1 :scale_denom=4", 4)])
def test_python_api_sizes_its_images(options, denom):
    import torch
    from nvimagecodec_amd import api
    entries = [S.by_name(n) for n in ("h130x70_420_opt_q75", "t7x5_444_base", "c5_640x360_444_prog_q90", "t33x17_gray_prog")]
    with api.Decoder(max_num_cpu_threads=4, options=options) as d:
        imgs = d.decode([_jpeg(e) for e in entries])
        torch.cuda.synchronize()
        for e, im in zip(entries, imgs):
            got = np.asarray(im.cpu()._array)
            sc = e["scales"][str(denom)]
            assert got.shape[:2] == (sc["height"], sc["width"]), (e["name"], got.shape)
            want = sc["y_sha256"] if got.shape[2] == 1 else sc["rgb_sha256"]
            assert S.sha(got) == want, e["name"]


def _fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_hipimtrans_scale(dec, tmp_path):
    """hipimtrans --scale 1/2 on two files: the checksums it writes (FNV-1a of the decoded RGB bytes) are those of the pixels the manifest
    pins; --scale does not go with --lossless."""
    import os
    import subprocess
    tool = os.path.join(os.path.dirname(N.LIB_PATH), "hipimtrans")
    assert os.path.exists(tool), "build the tool: make -C nvimagecodec_amd/csrc"
    src = tmp_path / "in"
    src.mkdir()
    entries = [S.by_name("h130x70_420_opt_q75"), S.by_name("c5_640x360_444_prog_q90")]
    for e in entries:
        (src / (e["name"] + ".jpg")).write_bytes(_jpeg(e))
    sums = tmp_path / "sums.txt"
    p = subprocess.run([tool, "-i", str(src), "--devices", "0", "-b", "2", "-w", "0", "--scale", "1/2", "--checksums", str(sums)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = dict(line.split() for line in sums.read_text().splitlines())
    outs, _ = dec.decode([_jpeg(e) for e in entries], scales=[2, 2])
    for e, o in zip(entries, outs):
        px = _cpu(o)
        assert S.sha(px) == S.expected(e, 2)[1]
        assert int(got[e["name"] + ".jpg"], 16) == _fnv1a(px.tobytes()), e["name"]
    p = subprocess.run([tool, "-i", str(src), "-o", str(tmp_path), "--lossless", "--scale", "1/2"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--scale" in p.stderr
    p = subprocess.run([tool, "-i", str(src), "--scale", "1/3"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "1/2, 1/4 or 1/8" in p.stderr
