"""Lossless transcode on the device: hipjpegTranscodeBatch = entropy decode (GPU or host pool) -> coef_relayout_kernel -> entropy
coder (GPU or host pool).  Whatever route an image takes, its file is the one hipjpegTranscodeHost writes (tests/test_transcode_host.py
pins that one against libjpeg-turbo's files and the oracle), byte for byte."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from helpers import sequential_scans as S
from helpers import transcode_cases as T
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(N.LIB_PATH), "hipimtrans")
_DECODE = T.golden_files("decode")


@functools.lru_cache(maxsize=None)
def _host_files(target):
    """transcode_host of every decode golden, once per target"""
    return tuple(lowlevel.transcode_host(d, **T.TARGETS[target]) for _, d in _DECODE)


def _takes_gpu_decoder(data):
    """the existing predicate: the GPU entropy decoder's algorithm does not call the stream UNSUPPORTED"""
    try:
        lowlevel.entropy_decode_gpu_algorithm_host(data)
    except N.HipJpegError as e:
        if e.status == T.UNSUPPORTED:
            return False
        raise
    return True


@functools.lru_cache(maxsize=None)
def _gpu_decodable():
    return sum(_takes_gpu_decoder(d) for _, d in _DECODE)


@pytest.fixture(scope="module")
def transcoder():
    t = lowlevel.BatchTranscoder(device=0, num_threads=8, gpu_huffman=True, gpu_restart=True)
    yield t
    t.close()


def _check(transcoder, sources, **kw):
    """both routes give transcode_host's files"""
    want = [lowlevel.transcode_host(s, **kw) for s in sources]
    for gpu in (True, False):
        statuses, files = transcoder.transcode(sources, gpu_huffman=gpu, **kw)
        assert statuses == [0] * len(sources), (gpu, statuses)
        for i, (a, b) in enumerate(zip(files, want)):
            assert a == b, (gpu, i, kw)
    return want


@pytest.mark.parametrize("target", list(T.TARGETS))
def test_all_decode_goldens_in_one_batch(transcoder, target):
    sources = [d for _, d in _DECODE]
    want = _host_files(target)
    statuses, files = transcoder.transcode(sources, **T.TARGETS[target])
    assert statuses == [0] * len(sources)
    bad = [n for (n, _), a, b in zip(_DECODE, files, want) if a != b]
    assert not bad, bad
    st = transcoder.stats()
    assert st["gpu_decoded_images"] == _gpu_decodable()
    assert st["gpu_coded_images"] == len(sources)  # no restart interval, or baseline with one under gpu_restart: the GPU coder takes all
    assert st["relayout_blocks"] == sum(rh * rw for _, d in _DECODE for rh, rw in T.real_area(d))
    statuses, files = transcoder.transcode(sources, gpu_huffman=False, **T.TARGETS[target])
    assert statuses == [0] * len(sources) and list(files) == list(want)
    st = transcoder.stats()
    assert st["gpu_decoded_images"] == 0 and st["gpu_coded_images"] == 0


def _img(w, h, sub, seed, q=88, **kw):
    return oracle.encode(synth_image(w, h, seed=seed), sub, q, **kw)


def test_small_shapes(transcoder):
    gray8 = oracle.encode(synth_image(8, 8, seed=3), "gray", 90)
    sources = [gray8,
               _img(33, 47, "420", 4), _img(50, 37, "420", 5),        # real grid smaller than the padded grid both ways
               _img(129, 70, "422", 6), _img(129, 70, "411", 7),      # more than one 128-MCU unit, ragged last unit
               _img(2049, 16, "444", 8)]                              # a long row: 257 blocks per row, the last wave ragged
    for kw in T.TARGETS.values():
        _check(transcoder, sources, **kw)


def test_multiscan_restart_and_progressive_sources(transcoder):
    base = _img(40, 40, "420", 9)
    multiscan = S.recode(base, [[0], [1], [2]])
    restart = _img(40, 40, "420", 10, restart_interval=2)
    progressive = next(d for _, d in _DECODE if lowlevel.get_image_info(d)["sof_marker"] == 0xC2 and _takes_gpu_decoder(d))
    sources = [multiscan, restart, progressive]
    for kw in (T.TARGETS["optimized"], T.TARGETS["progressive"], T.TARGETS["annexk_rst3"]):
        want = _check(transcoder, sources, **kw)
        assert want[0] == lowlevel.transcode_host(base, **kw)  # the scan layout of the source leaves no trace
    statuses, _ = transcoder.transcode(sources)
    assert statuses == [0, 0, 0] and transcoder.stats()["gpu_decoded_images"] == 3


def test_source_below_the_hybrid_threshold_is_host_decoded_dense():
    t = lowlevel.BatchTranscoder(device=0, num_threads=2, gpu_huffman=True)
    try:
        t.set_hybrid_huffman_threshold(100 * 100)
        sources = [_img(64, 48, "420", 11), _img(640, 480, "420", 12), _img(97, 31, "444", 13)]
        for kw in (T.TARGETS["annexk"], T.TARGETS["progressive"]):
            statuses, files = t.transcode(sources, **kw)
            assert statuses == [0, 0, 0]
            assert files == [lowlevel.transcode_host(s, **kw) for s in sources]
            assert t.stats()["gpu_decoded_images"] == 1 and t.stats()["gpu_coded_images"] == 3
    finally:
        t.close()


def test_mixed_batch_failures_leave_their_neighbours_alone(transcoder):
    cmyk = T.golden_files("cmyk")[0][1]
    out_of_range = next(d for _, d in T.golden_files("gamut") if T.expected_eligible(d) == (True, False))
    whole = _DECODE[0][1]
    truncated = whole[: len(whole) * 2 // 3]
    good = list(range(0, 40, 4))
    sources, expect, want = [], [], []
    for k, g in enumerate(good):
        sources.append(_DECODE[g][1])
        expect.append(T.SUCCESS)
        want.append(_host_files("optimized")[g])
        if k % 3 == 0:
            for bad, st in ((cmyk, T.UNSUPPORTED), (out_of_range, T.UNSUPPORTED), (truncated, T.TRUNCATED)):
                sources.append(bad)
                expect.append(st)
                want.append(None)
    for gpu in (True, False):
        statuses, files = transcoder.transcode(sources, gpu_huffman=gpu, **T.TARGETS["optimized"])
        assert statuses == expect, gpu
        assert files == want, gpu
    # and the handle is as good as new
    clean = [d for _, d in _DECODE[:32]]
    statuses, files = transcoder.transcode(clean, **T.TARGETS["progressive"])
    assert statuses == [0] * 32 and files == list(_host_files("progressive")[:32])


def test_refused_while_a_submit_is_in_flight_on_the_handle():
    """the call takes a decode page and the encode batch for itself"""
    import ctypes

    import torch
    enc = lowlevel.BatchEncoder(device=0, num_threads=2, gpu_huffman=True)
    try:
        src = _DECODE[0][1]
        a = np.frombuffer(src, dtype=np.uint8)
        ptrs, lens = (ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_size_t * 1)(a.size)
        P, statuses = (N.TranscodeParams * 1)(), (ctypes.c_int * 1)()
        stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        call = lambda: N.load().hipjpegTranscodeBatch(enc._h, ptrs, lens, 1, P, N.FLAG_GPU_HUFFMAN, statuses, stream)
        enc.submit([torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda:0")], "420", 90)
        assert call() == 1  # INVALID_ARGUMENT
        enc.wait()
        assert call() == 0 and statuses[0] == 0
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        assert N.load().hipjpegEncodeGetBitstream(enc._h, 0, ctypes.byref(p), ctypes.byref(n)) == 0
        assert ctypes.string_at(p, n.value) == lowlevel.transcode_host(src)
    finally:
        enc.close()


@pytest.mark.parametrize("target", ["optimized", "progressive"])
def test_pixels_survive(target):
    """the same pixel kernels on the same coefficients"""
    picked = [i for i, (_, d) in enumerate(_DECODE) if lowlevel.get_image_info(d)["subsampling"] in (0, 2, 6)]
    sources = [_DECODE[i][1] for i in picked]
    outs = [_host_files(target)[i] for i in picked]
    t = lowlevel.BatchTranscoder(device=0, num_threads=8)
    try:
        statuses, files = t.transcode(sources, **T.TARGETS[target])
        assert statuses == [0] * len(sources) and files == outs
    finally:
        t.close()
    dec = lowlevel.BatchDecoder(device=0, num_threads=8)
    try:
        a, sa = dec.decode(sources, fmt="rgb", gpu_huffman=True)
        a = [x.cpu().numpy() for x in a]
        b, sb = dec.decode(files, fmt="rgb", gpu_huffman=True)
        b = [x.cpu().numpy() for x in b]
    finally:
        dec.close()
    assert list(sa) == [0] * len(sources) and list(sb) == [0] * len(sources)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), _DECODE[picked[i]][0]


def test_hipimtrans_lossless(tmp_path):
    assert os.path.exists(TOOL), "build the tool: make -C nvimagecodec_amd/csrc"
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    picked = _DECODE[::13][:10]
    for name, data in picked:
        (src / (name + ".jpg")).write_bytes(data)
    (src / "zz_cmyk.jpg").write_bytes(T.golden_files("cmyk")[0][1])
    p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst), "-b", "4", "-w", "1", "--lossless", "--jpeg_encoding", "progressive_dct"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Total images: 11 (failed: 0, unsupported: 1)" in p.stdout and "zz_cmyk.jpg" in p.stderr
    assert "Avg transcoding speed  (in images per sec):" in p.stdout
    for name, data in picked:
        assert (dst / (name + ".jpg")).read_bytes() == lowlevel.transcode_host(data, progressive=True), name
    assert not (dst / "zz_cmyk.jpg").exists()
    # -q / -s have no meaning without pixels
    for extra in (["-q", "80"], ["-s", "444"]):
        p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst), "--lossless"] + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "--lossless" in p.stderr
