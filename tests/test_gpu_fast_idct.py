"""The fast integer IDCT on the GPU (HIPJPEG_FLAG_FAST_IDCT; plugin option hipjpeg_decoder:fast_idct=1), bit-exact against the hashes of
tests/golden/manifest_fast_idct.json (libjpeg-turbo's JDCT_IFAST, x86-64 SIMD routine) and the numpy restatement of tests/helpers/ifast_idct.py,
through every path the pixel kernels serve."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_decode_case
from fake_plugin import FakeDecoderPlugin
from helpers import ifast_idct
from helpers.geometry import upright
from nvimagecodec_amd import _native
from nvimagecodec_amd import abi as A

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "manifest_fast_idct.json")) as _f:
    _M = json.load(_f)
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _ISLOW = {e["name"]: e for e in json.load(_f)["decode"]}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _jpeg(entry):
    return load_decode_case(_ISLOW[entry["name"]])[0]


def _read(*parts):
    with open(os.path.join(GOLDEN, *parts), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


def _cpu(outs):
    import torch
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
@pytest.mark.parametrize("fancy", [True, False], ids=["fancy", "plain"])
def test_every_decode_golden(dec, fancy, gpu_huffman):
    jpegs = [_jpeg(e) for e in _M["decode"]]
    key = "rgb_sha256" if fancy else "plain_rgb_sha256"
    rgb = _cpu(dec.decode(jpegs, fmt="rgb", fancy=fancy, gpu_huffman=gpu_huffman, fast_idct=True)[0])
    bad = [e["name"] for e, o in zip(_M["decode"], rgb) if _sha(o) != e[key]]
    assert not bad, bad
    bgr = _cpu(dec.decode(jpegs, fmt="bgr", fancy=fancy, gpu_huffman=gpu_huffman, fast_idct=True)[0])
    assert all(np.array_equal(b, r[:, :, ::-1]) for b, r in zip(bgr, rgb))
    planar = _cpu(dec.decode(jpegs, fmt="rgb_planar", fancy=fancy, gpu_huffman=gpu_huffman, fast_idct=True)[0])
    assert all(np.array_equal(p, r.transpose(2, 0, 1)) for p, r in zip(planar, rgb))


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
def test_luma_and_yuv_planes_equal_the_restatement(dec, gpu_huffman):
    jpegs = [_jpeg(e) for e in _M["decode"]]
    ys = _cpu(dec.decode(jpegs, fmt="y", gpu_huffman=gpu_huffman, fast_idct=True)[0])
    yuv = dec.decode(jpegs, fmt="yuv_planar", gpu_huffman=gpu_huffman, fast_idct=True)[0]
    for e, j, y, planes in zip(_M["decode"], jpegs, ys, yuv):
        ref = ifast_idct.planes(j)
        assert np.array_equal(y.reshape(ref[0].shape), ref[0]), e["name"]
        got = [p.cpu().numpy() for p in planes]
        assert len(got) == len(ref), e["name"]
        for c, r in enumerate(ref):
            assert np.array_equal(got[c], r), (e["name"], c)


def test_out_of_gamut_vectors(dec):
    names = [g["name"] for g in _M["gamut"]]
    jpegs = [_read("gamut", n + ".jpg") for n in names]
    gray = [g["mode"] == "L" for g in _M["gamut"]]
    for gpu_huffman in (False, True):
        y = _cpu(dec.decode([j for j, g in zip(jpegs, gray) if g], fmt="y", gpu_huffman=gpu_huffman, fast_idct=True)[0])
        rgb = _cpu(dec.decode([j for j, g in zip(jpegs, gray) if not g], fmt="rgb", gpu_huffman=gpu_huffman, fast_idct=True)[0])
        gi, ci = iter(y), iter(rgb)
        bad = []
        for g, is_gray in zip(_M["gamut"], gray):
            o = next(gi).reshape(g["height"], g["width"]) if is_gray else next(ci)
            if _sha(o) != g["simd_sha256"]:
                bad.append(g["name"])
        assert not bad, (gpu_huffman, bad)


def _reference_rgb(cmyk, adobe):
    """extensions/libjpeg_turbo/jpeg_mem.cpp:303-313 (as tests/test_cmyk.py)"""
    c, m, y, k = [cmyk[:, :, i].astype(np.int32) for i in range(4)]
    if adobe:
        return np.stack([(k * c) // 255, (k * m) // 255, (k * y) // 255], axis=2).astype(np.uint8)
    return np.stack([(255 - k) * (255 - c) // 255, (255 - k) * (255 - m) // 255, (255 - k) * (255 - y) // 255], axis=2).astype(np.uint8)


def test_cmyk(dec):
    jpegs = [_read("cmyk", e["name"] + ".jpg") for e in _M["cmyk"]]
    outs = _cpu(dec.decode(jpegs, fmt="rgb", fast_idct=True)[0])
    for e, j, o in zip(_M["cmyk"], jpegs, outs):
        samples = ifast_idct.cmyk_samples(j)
        assert _sha(samples) == e["cmyk_sha256"], e["name"]
        assert np.array_equal(o, _reference_rgb(samples, e["kind"] != "plain")), e["name"]


def test_regions_of_interest_and_orientation(dec):
    by_name = {e["name"]: e for e in _M["decode"]}
    for fancy in (True, False):
        rois = [r for r in _M["roi"] if r["fancy"] == fancy]
        jpegs = [_jpeg(by_name[r["name"]]) for r in rois]
        tr = [((x, y, x + w, y + h), 1) for (x, y, w, h) in (r["roi"] for r in rois)]
        outs = _cpu(dec.decode(jpegs, fmt="rgb", fancy=fancy, transforms=tr, fast_idct=True)[0])
        bad = [(r["name"], r["roi"]) for r, o in zip(rois, outs) if _sha(o) != r["rgb_sha256"]]
        assert not bad, (fancy, bad)
    entries = [e for e in _M["decode"] if e["width"] >= 16 and e["height"] >= 16][:24]
    jpegs = [_jpeg(e) for e in entries]
    full = _cpu(dec.decode(jpegs, fmt="rgb", fast_idct=True)[0])
    for o in range(2, 9):
        outs = _cpu(dec.decode(jpegs, fmt="rgb", transforms=[(None, o)] * len(jpegs), fast_idct=True)[0])
        for e, f, g in zip(entries, full, outs):
            assert np.array_equal(g, upright(f, o)), (e["name"], o)


def test_full_size_goldens_are_covered():
    names = {e["name"] for e in _M["decode"]}
    assert "c2_1920x1080_420_base_q90" in names and "c5_640x360_444_prog_q90" in names


def test_one_handle_alternates_islow_and_ifast(dec):
    entries = [e for e in _M["decode"] if e["name"].startswith(("c", "s", "r"))][:40]
    jpegs = [_jpeg(e) for e in entries]
    for gpu_huffman in (True, False):
        for fast, key in ((False, "islow"), (True, "ifast"), (False, "islow"), (True, "ifast")):
            outs = _cpu(dec.decode(jpegs, fmt="rgb", gpu_huffman=gpu_huffman, fast_idct=fast)[0])
            for e, o in zip(entries, outs):
                want = _ISLOW[e["name"]]["rgb_sha256"] if key == "islow" else e["rgb_sha256"]
                assert _sha(o) == want, (e["name"], key, gpu_huffman)


def test_submit_and_host_stage_take_the_flag(dec):
    import torch
    entries = [e for e in _M["decode"] if e["name"].startswith("c")][:8]
    jpegs = [_jpeg(e) for e in entries]
    outs = dec.allocate_outputs(jpegs, "rgb", None)
    dec.submit(jpegs, outs, fmt="rgb", fast_idct=True)
    dec.wait()
    torch.cuda.synchronize()
    assert [_sha(o.cpu().numpy()) for o in outs] == [e["rgb_sha256"] for e in entries]
    outs = dec.allocate_outputs(jpegs, "rgb", None)
    assert all(s == 0 for s in dec.host_stage(jpegs, outs, fmt="rgb", fast_idct=True))
    dec.transfer()
    dec.device_stage()
    torch.cuda.synchronize()
    assert [_sha(o.cpu().numpy()) for o in outs] == [e["rgb_sha256"] for e in entries]


def _setup(lib, extra_plugins=(), options=b""):
    ci = A.init(A.InstanceCreateInfo, A.ST_INSTANCE_CREATE_INFO, load_builtin_modules=1, load_extension_modules=1)
    inst = C.c_void_p()
    assert lib.nvimgcodecInstanceCreate(C.byref(inst), C.byref(ci)) == 0
    for p in extra_plugins:
        assert lib.nvimgcodecExtensionCreate(inst, None, C.byref(p.ext_desc)) == 0
    ep = A.init(A.ExecutionParams, A.ST_EXECUTION_PARAMS, device_id=0, max_num_cpu_threads=2)
    d = C.c_void_p()
    assert lib.nvimgcodecDecoderCreate(inst, C.byref(d), C.byref(ep), options) == 0
    return inst, d


@pytest.mark.parametrize("options", [b"hipjpeg_decoder:fast_idct=1", b":fast_idct=1 hipjpeg_decoder:fast_idct=1",
                                     b"hipjpeg_decoder:fast_idct=1 :fast_idct=1"])
def test_plugin_named_option_decodes_here(options):
    import torch
    from test_gpu_plugin import _c_api_decode
    lib = A.bind(_native.load_host())
    e = next(x for x in _M["decode"] if x["name"] == "s50x37_420_base_q90")
    jpeg = _jpeg(e)
    cpu = FakeDecoderPlugin("cpu_fallback", priority=A.PRIORITY_NORMAL, fill=0x42)
    inst, d = _setup(lib, extra_plugins=[cpu], options=options)
    buf = np.zeros((37, 50, 3), dtype=np.uint8)
    assert _c_api_decode(lib, inst, d, jpeg, 37, 50, A.SAMPLEFORMAT_I_RGB, 1, 3, buf.ctypes.data, 150, A.BUFFER_KIND_STRIDED_HOST) == A.PS_SUCCESS
    torch.cuda.synchronize()
    assert cpu.count("decode") == 0
    assert _sha(buf) == e["rgb_sha256"]
    lib.nvimgcodecDecoderDestroy(d)
    lib.nvimgcodecInstanceDestroy(inst)


def test_python_api_option():
    import torch
    from nvimagecodec_amd import api
    names = ["s50x37_420_base_q90", "c2_1920x1080_420_base_q90", "c5_640x360_444_prog_q90"]
    entries = [next(x for x in _M["decode"] if x["name"] == n) for n in names]
    with api.Decoder(max_num_cpu_threads=4, options="hipjpeg_decoder:fast_idct=1") as d:
        imgs = d.decode([_jpeg(e) for e in entries])
        torch.cuda.synchronize()
        for e, im in zip(entries, imgs):
            assert _sha(np.asarray(im.cpu()._array)) == e["rgb_sha256"], e["name"]
