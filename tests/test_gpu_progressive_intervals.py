"""Progressive (SOF2) files whose scans all have restart intervals on the GPU entropy stage (csrc/progressive_intervals.hip: a lane per
restart interval finds the block start positions and the DC planes, the replay kernel builds the blocks), opt-in by
gpu_progressive_intervals / HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS.  Bit-exact against the goldens and the oracle; with the flag off such
files keep the host entropy stage as before."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case
from helpers import progressive_restart_files as P

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _M = json.load(_f)
_RST = [e for e in _M["decode"] if e["progressive"] and "_rst" in e["name"]]


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


def _sync():
    import torch
    torch.cuda.synchronize()


def _have_pillow():
    try:
        import PIL  # noqa: F401
    except ImportError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def _interval_files():
    """[(id, file, golden RGB or None)]: every input of tests/test_progressive_intervals.py the interval kernels take.  Only
    libjpeg-turbo's 27 files need Pillow; where it is missing the goldens, the coder's own files and the helper files run all the same."""
    files = [(e["name"],) + load_decode_case(e) for e in _RST]
    if _have_pillow():
        files += [(n, j, None) for n, j in P.pillow_files()]
    files += [(n, j, None) for n, j in P.transcode_products(GOLDEN)]
    files += [(n, P.helper_file(n)[0], None) for n in sorted(P.HELPER_CASES)]
    return tuple(files)


@functools.lru_cache(maxsize=None)
def _mixed_batch():
    """-> (files, reference pixels, interval-eligible count, GPU entropy images with the flag off): the interval files, the file whose
    luma AC scans have different intervals (host entropy stage either way), 8 progressive goldens without restart markers (the walk) and
    8 baseline goldens"""
    files = list(_interval_files())
    files.append(("different_intervals", P.helper_file(P.DIFFERENT_INTERVALS)[0], None))
    others = [e for e in _M["decode"] if e["progressive"] and "_rst" not in e["name"]][:8] + [e for e in _M["decode"] if not e["progressive"]][:8]
    files += [(e["name"],) + load_decode_case(e) for e in others]
    refs = tuple(rgb if rgb is not None else oracle.decode(j) for _, j, rgb in files)
    return tuple(j for _, j, _ in files), refs, len(_interval_files()), len(others)


def test_mixed_batch_takes_the_interval_kernels(dec):
    jpegs, refs, n_interval, n_others = _mixed_batch()
    assert n_interval == 4 + 12 + len(P.HELPER_CASES) + (27 if _have_pillow() else 0)
    outs, st = dec.decode(list(jpegs), fmt="rgb", gpu_huffman=True, gpu_progressive_intervals=True, check=False)
    _sync()
    assert all(s == 0 for s in st), st
    stats = dec.stats()
    assert stats["interval_images"] == n_interval
    assert stats["gpu_entropy_images"] == len(jpegs) - 1
    assert stats["interval_takeovers"] == 0  # the kernels vouched for every image: none was left to the host decoder
    assert dec.host_fallbacks() == 0
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert np.array_equal(o.cpu().numpy(), r), i


def test_the_same_batch_with_the_flag_off_keeps_the_host_entropy_stage(dec):
    jpegs, refs, _, n_others = _mixed_batch()
    outs, st = dec.decode(list(jpegs), fmt="rgb", gpu_huffman=True, check=False)
    _sync()
    assert all(s == 0 for s in st), st
    stats = dec.stats()
    assert stats["interval_images"] == 0 and stats["interval_takeovers"] == 0
    assert stats["gpu_entropy_images"] == n_others
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert np.array_equal(o.cpu().numpy(), r), i
    # the flag alone means nothing
    outs, st = dec.decode(list(jpegs[:6]), fmt="rgb", gpu_huffman=False, gpu_progressive_intervals=True)
    _sync()
    assert dec.stats()["interval_images"] == 0 and dec.stats()["gpu_entropy_images"] == 0
    for o, r in zip(outs, refs):
        assert np.array_equal(o.cpu().numpy(), r)


@pytest.mark.parametrize("fmt", ["bgr", "rgb_planar", "y", "yuv_planar"])
def test_interval_files_in_every_output_format(dec, fmt):
    """The DC planes and the coefficient blocks feed every flavour of the pixel kernels."""
    jpegs = [load_decode_case(next(e for e in _RST if e["name"] == n))[0] for n in ("r130x70_420_prog_rst1", "r130x70_444_prog_rst7")]
    jpegs.append(P.helper_file("gray_500_intervals")[0])
    outs, _ = dec.decode(jpegs, fmt=fmt, gpu_huffman=True, gpu_progressive_intervals=True)
    _sync()
    assert dec.stats()["interval_images"] == len(jpegs) and dec.stats()["interval_takeovers"] == 0 and dec.host_fallbacks() == 0
    for n, (j, o) in enumerate(zip(jpegs, outs)):
        if fmt == "yuv_planar":
            for a, b in zip(o, oracle.decode_planes(j)):
                assert np.array_equal(a.cpu().numpy(), b), n
            continue
        ref = oracle.decode(j, {"bgr": oracle.FMT_BGR, "rgb_planar": oracle.FMT_RGB, "y": oracle.FMT_GRAY}[fmt])
        if fmt == "rgb_planar":
            ref = ref.transpose(2, 0, 1)
        assert np.array_equal(o.cpu().numpy(), ref), (n, fmt)


def test_damaged_interval_streams_get_the_host_path_statuses(dec):
    """Bit flips inside the scans, 96 files: the interval route and the host route must report the same status per image and, where
    both decode, the same pixels (the kernels hand anything they cannot vouch for to the host entropy decoder).  Which images the
    kernels take and which of those they flag is what their code says on the host (hipjpegEntropyDecodeGpuIntervalAlgorithmHost)."""
    from nvimagecodec_amd import _native as N
    from nvimagecodec_amd import lowlevel
    base = [load_decode_case(e)[0] for e in _RST] + [P.helper_file(n)[0] for n in ("bands_cut_anywhere", "dc_recut_per_component")]
    rng = random.Random(4242)
    damaged = []
    for _ in range(96):
        j = bytearray(rng.choice(base))
        first_sos = j.find(b"\xff\xda")
        for _ in range(rng.randrange(1, 3)):
            k = rng.randrange(first_sos + 14, len(j) - 2)
            j[k] ^= 1 << rng.randrange(8)
        damaged.append(bytes(j))
    outs_h = dec.allocate_outputs(damaged, "rgb")
    outs_g = dec.allocate_outputs(damaged, "rgb")
    keep = [i for i, o in enumerate(outs_h) if o is not None]
    damaged = [damaged[i] for i in keep]
    outs_h = [outs_h[i] for i in keep]
    outs_g = [outs_g[i] for i in keep]
    _, st_h = dec.decode(damaged, outs=outs_h, check=False, gpu_huffman=False)
    _sync()
    _, st_g = dec.decode(damaged, outs=outs_g, check=False, gpu_huffman=True, gpu_progressive_intervals=True)
    _sync()
    verdicts = []  # of the kernels' algorithm on the host: 0 accepted, 5 (CORRUPT) flagged, 2 / 3 / 4 (header level) not an interval image
    for j in damaged:
        try:
            lowlevel.entropy_decode_gpu_interval_algorithm_host(j)
            verdicts.append(0)
        except N.HipJpegError as e:
            verdicts.append(e.status)
    assert set(verdicts) <= {0, 2, 3, 4, 5}
    taken = sum(1 for v in verdicts if v in (0, 5))
    flagged = sum(1 for v in verdicts if v == 5)
    assert taken > len(damaged) // 2 and 0 < flagged < taken  # the damage leaves most of them eligible; both verdicts occur
    assert dec.stats()["interval_images"] == taken
    assert dec.stats()["interval_takeovers"] == flagged
    assert flagged >= sum(1 for v, s in zip(verdicts, st_g) if v in (0, 5) and s != 0)  # every interval image that failed was flagged first
    assert st_h == st_g
    assert any(s != 0 for s in st_h) and any(s == 0 for s in st_h)
    for s, a, b in zip(st_h, outs_h, outs_g):
        if s == 0:
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_interval_files_through_the_pipelined_entry_points(dec):
    """submit / wait, three batches in flight, two batches of interval files in turn"""
    import torch
    files = [j for _, j, _ in _interval_files()]
    batches = [files[0::2][:12], files[1::2][:12]]
    refs = [[oracle.decode(j) for j in b] for b in batches]
    dec.set_pipeline_depth(3)
    submitted = []
    for k in range(6):
        if k >= 3:
            assert all(s == 0 for s in dec.wait())
            assert dec.stats()["interval_takeovers"] == 0
        submitted.append(dec.allocate_outputs(batches[k % 2], "rgb"))
        dec.submit(batches[k % 2], submitted[-1], gpu_huffman=True, gpu_progressive_intervals=True)
    for _ in range(3):
        assert all(s == 0 for s in dec.wait())
        assert dec.stats()["interval_takeovers"] == 0  # (of the batch that wait settled)
    torch.cuda.synchronize()
    for k, outs in enumerate(submitted):
        for r, o in zip(refs[k % 2], outs):
            assert np.array_equal(o.cpu().numpy(), r), k


def test_coefficient_tensors_of_interval_files():
    import torch
    from nvimagecodec_amd import lowlevel
    jpegs = [load_decode_case(next(e for e in _RST if e["name"] == "r130x70_420_prog_rst7"))[0], P.helper_file("three_bit_planes")[0]]
    want = [lowlevel.decode_coefficients_host(j) for j in jpegs]
    for flag in (True, False):
        bc = lowlevel.BatchCoefficients(device=0, num_threads=2, gpu_huffman=True, gpu_progressive_intervals=flag)
        statuses, images = bc.decode(jpegs)
        torch.cuda.synchronize()
        assert statuses == [0, 0]
        assert bc.stats()["gpu_decoded_images"] == (2 if flag else 0) and bc.stats()["interval_takeovers"] == 0
        for (info, coefs), im in zip(want, images):
            assert len(coefs) == len(im.coefs)
            for a, b in zip(coefs, im.coefs):
                assert np.array_equal(np.asarray(a).reshape(b.shape), b.cpu().numpy())
        bc.close()


def test_transcode_of_interval_files_decodes_them_on_the_gpu():
    import torch
    from nvimagecodec_amd import lowlevel
    jpegs = [load_decode_case(e)[0] for e in _RST]
    want = [lowlevel.transcode_host(j) for j in jpegs]
    for flag in (True, False):
        tc = lowlevel.BatchTranscoder(device=0, num_threads=2, gpu_huffman=True, gpu_progressive_intervals=flag)
        statuses, files = tc.transcode(jpegs)
        torch.cuda.synchronize()
        assert list(statuses) == [0] * len(jpegs)
        assert tc.stats()["gpu_decoded_images"] == (len(jpegs) if flag else 0) and tc.stats()["interval_takeovers"] == 0
        assert files == want
        tc.close()


def test_plugin_option_gpu_progressive_intervals():
    """hipjpeg_decoder:gpu_progressive_intervals=1 is a known option and the file decodes to the golden pixels"""
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd import _native
    from nvimagecodec_amd import abi as A
    lib = A.bind(_native.load_host())
    messages = []

    def on_message(severity, category, data, user):
        messages.append(data.contents.message.decode(errors="replace") if data.contents.message else "")
        return 0

    cb = A.DebugCallback(on_message)
    messenger = A.init(A.DebugMessengerDesc, A.ST_DEBUG_MESSENGER_DESC, message_severity=0xFFFF, message_category=0xFFFF, user_callback=cb)
    ci = A.init(A.InstanceCreateInfo, A.ST_INSTANCE_CREATE_INFO, load_builtin_modules=1, load_extension_modules=1)
    inst = C.c_void_p()
    assert lib.nvimgcodecInstanceCreate(C.byref(inst), C.byref(ci)) == 0
    dm = C.c_void_p()
    assert lib.nvimgcodecDebugMessengerCreate(inst, C.byref(dm), C.byref(messenger)) == 0
    ep = A.init(A.ExecutionParams, A.ST_EXECUTION_PARAMS, device_id=0, max_num_cpu_threads=2)
    dec = C.c_void_p()
    assert lib.nvimgcodecDecoderCreate(inst, C.byref(dec), C.byref(ep), b"hipjpeg_decoder:gpu_progressive_intervals=1") == 0
    jpeg, rgb = load_decode_case(next(e for e in _RST if e["name"] == "r130x70_420_prog_rst7"))
    h, w = rgb.shape[:2]
    buf = np.zeros((h, w, 3), dtype=np.uint8)
    arr = np.frombuffer(jpeg, dtype=np.uint8)
    cs = C.c_void_p()
    assert lib.nvimgcodecCodeStreamCreateFromHostMem(inst, C.byref(cs), arr.ctypes.data, arr.size) == 0
    info = A.init(A.ImageInfo, A.ST_IMAGE_INFO, sample_format=A.SAMPLEFORMAT_I_RGB, color_spec=A.COLORSPEC_SRGB, num_planes=1, buffer=buf.ctypes.data,
                  buffer_size=w * 3 * h, buffer_kind=A.BUFFER_KIND_STRIDED_HOST, cuda_stream=0)
    pi = info.plane_info[0]
    pi.width, pi.height, pi.row_stride, pi.num_channels, pi.sample_type = w, h, w * 3, 3, A.SAMPLE_DATA_TYPE_UINT8
    im = C.c_void_p()
    assert lib.nvimgcodecImageCreate(inst, C.byref(im), C.byref(info)) == 0
    dp = A.init(A.DecodeParams, A.ST_DECODE_PARAMS)
    fut = C.c_void_p()
    assert lib.nvimgcodecDecoderDecode(dec, (C.c_void_p * 1)(cs), (C.c_void_p * 1)(im), 1, C.byref(dp), C.byref(fut)) == 0
    assert lib.nvimgcodecFutureWaitForAll(fut) == 0
    st = (C.c_uint32 * 1)()
    n = C.c_size_t()
    lib.nvimgcodecFutureGetProcessingStatus(fut, st, C.byref(n))
    lib.nvimgcodecFutureDestroy(fut)
    lib.nvimgcodecImageDestroy(im)
    lib.nvimgcodecCodeStreamDestroy(cs)
    assert st[0] == A.PS_SUCCESS
    assert np.array_equal(buf, rgb)
    assert not any("unknown option" in m and "gpu_progressive_intervals'" in m for m in messages), messages
    lib.nvimgcodecDecoderDestroy(dec)
    lib.nvimgcodecInstanceDestroy(inst)
