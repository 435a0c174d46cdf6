"""Drop chroma, crop and copy metadata on the device: hipjpegTranscodeBatch with hipjpegTranscodeBatchSetRegions and the new flags.
Images cropped at an origin go through coef_transform_kernel (turned or not), the others through coef_relayout_kernel; whichever entropy
routes an image takes, its file is the one hipjpegTranscodeHostRegion writes for the same request (tests/test_transcode_crop_host.py pins
that one against the numpy model), byte for byte.  The shapes are the smallest at which the kernel's addressing can go wrong: one block
from an inner origin, one MCU under every turn, the source's ragged edge, a right edge off the block grid, rows of 256 blocks (a unit
ends exactly at a row end) and their transpose (units end mid-column)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from helpers import crop_model as C
from helpers import transcode_cases as T
from helpers import transform_model as M
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(N.LIB_PATH), "hipimtrans")
_DECODE = T.golden_files("decode")
ROUTES = {"optimized": T.TARGETS["optimized"], "progressive": T.TARGETS["progressive"], "restart": dict(optimized_huffman=True, restart_interval=3)}


def _host(data, **kw):
    """(status, file) of the host route"""
    try:
        return T.SUCCESS, lowlevel.transcode_host(data, **kw)
    except N.HipJpegError as e:
        return e.status, None


@pytest.fixture(scope="module")
def transcoder():
    t = lowlevel.BatchTranscoder(device=0, num_threads=8, gpu_huffman=True, gpu_restart=True)
    yield t
    t.close()


def _img(w, h, sub, seed, q=88):
    return oracle.encode(synth_image(w, h, seed=seed), sub, q)


@functools.lru_cache(maxsize=None)
def _cases():
    """[(source, region, orientation, extra keywords, expected status)]"""
    gray24, mcu48, ragged, wide422 = _img(24, 24, "gray", 61), _img(48, 48, "420", 62), _img(50, 37, "420", 63), _img(64, 48, "422", 64)
    long444, wide411, src420 = _img(2049, 16, "444", 65), _img(129, 70, "411", 66), _img(80, 64, "420", 67)
    cases = [(gray24, (8, 8, 16, 16), 1, {}, T.SUCCESS)]                                       # one output block from block origin (1, 1)
    cases += [(mcu48, (16, 16, 32, 32), k, {}, T.SUCCESS) for k in range(1, 9)]                 # one MCU, every orientation
    cases += [(ragged, (16, 16, 50, 37), 1, {}, T.SUCCESS),                                     # the source's own ragged edge
              (wide422, (16, 0, 37, 29), 1, {}, T.SUCCESS),                                     # a right edge inside the source, off the block grid
              (long444, (8, 0, 2049, 16), 1, {}, T.SUCCESS),                                    # 256 blocks per row: a unit ends at a row end
              (long444, (8, 8, 2049, 16), 6, dict(trim=True), T.SUCCESS),                       # its transpose: units end mid-column
              (wide411, (32, 8, 129, 70), 2, dict(trim=True), T.SUCCESS), (wide411, (32, 8, 129, 70), 4, dict(trim=True), T.SUCCESS),
              (wide411, (32, 8, 129, 70), 3, dict(trim=True), T.SUCCESS), (wide411, (32, 8, 129, 70), 5, dict(trim=True), T.UNSUPPORTED),
              (src420, (8, 8, 72, 60), 1, dict(grayscale=True), T.SUCCESS), (src420, (8, 8, 72, 60), 7, dict(grayscale=True, trim=True), T.SUCCESS),
              (src420, (21, 13, 70, 50), 1, dict(expand=True), T.SUCCESS), (src420, (21, 13, 70, 50), 8, dict(expand=True, trim=True), T.SUCCESS),
              (src420, (21, 13, 70, 50), 1, {}, T.UNSUPPORTED), (src420, (8, 8, 72, 60), 1, {}, T.UNSUPPORTED)]
    return cases


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_small_shapes(transcoder, route):
    """one call per case (trim / grayscale / expand are per call), each for gpu_huffman on and off"""
    for k, (src, region, orientation, extra, status) in enumerate(_cases()):
        kw = dict(ROUTES[route], orientation=orientation, region=region, **extra)
        want = _host(src, **kw)
        model = C.expected(src, orientation, extra.get("trim", False), region, extra.get("grayscale", False), extra.get("expand", False))
        assert want[0] == status == model["status"], (k, want[0])
        for gpu in (True, False):
            statuses, files = transcoder.transcode([src, src], gpu_huffman=gpu, **kw)
            assert statuses == [status] * 2 and files == [want[1]] * 2, (route, k, gpu)
            if status == T.SUCCESS:
                assert transcoder.stats()["relayout_blocks"] == 2 * model["blocks"]


def test_mixed_batch():
    """identity, cropped, cropped and turned, gray, copy-markers with a turn, an invalid region, an unaligned origin, a truncated file and
    a host-decoded image (below the hybrid threshold) interleaved in one batch"""
    t = lowlevel.BatchTranscoder(device=0, num_threads=4, gpu_huffman=True)
    try:
        t.set_hybrid_huffman_threshold(100 * 100)
        big = [_img(160 + 16 * k, 128, "420", 70 + k) for k in range(6)]
        small = _img(64, 48, "444", 80)  # host-decoded
        tagged = big[4][:20] + M.exif_segment(6, True) + b"\xff\xe2\x00\x08ICC_PR" + b"\xff\xfe\x00\x05hi!" + big[4][20:]
        assert big[4][2:20] == C.JFIF_APP0
        sources = [big[0], big[1], small, big[2], big[3], tagged, big[5], big[0], small[:len(small) * 2 // 3], small, tagged]
        regions = [None, (16, 32, 150, 100), (8, 16, 60, 48), (32, 16, 192, 112), (0, 0, 0, 0), None, (16, 16, 300, 64), (8, 16, 100, 100),
                   (16, 16, 64, 48), (0, 0, 64, 48), (32, 32, 128, 96)]
        orientations = [1, 1, 1, 6, 1, 6, 1, 1, 1, 3, 8]
        gray = [False, False, False, False, True, False, False, False, False, False, True]
        markers = [False, False, False, False, False, True, False, False, False, False, True]
        want = [_host(s, optimized_huffman=True, orientation=o, region=r, grayscale=g, copy_markers=m, trim=True)
                for s, r, o, g, m in zip(sources, regions, orientations, gray, markers)]
        assert [st for st, _ in want] == [0, 0, 0, 0, 0, 0, C.INVALID_ARGUMENT, T.UNSUPPORTED, T.TRUNCATED, 0, 0]
        model = [C.expected(s, o, True, r, g) if k != 8 else None for k, (s, r, o, g) in enumerate(zip(sources, regions, orientations, gray))]
        blocks = sum(m["blocks"] for m, (st, _) in zip(model, want) if st == 0)
        assert [m["status"] for m in model if m is not None] == [st for k, (st, _) in enumerate(want) if k != 8]
        assert lowlevel.exif_orientation(want[5][1]) == 1 and lowlevel.exif_orientation(want[10][1]) == 1 and b"ICC_PR" in want[10][1]
        for gpu in (True, False):
            statuses, files = t.transcode(sources, optimized_huffman=True, orientation=orientations, region=regions, grayscale=gray, copy_markers=markers,
                                          trim=True, gpu_huffman=gpu)
            assert statuses == [st for st, _ in want], gpu
            assert files == [f for _, f in want], gpu
            assert t.stats()["relayout_blocks"] == blocks
            if gpu:  # the six big pictures that are written, and the two big ones whose regions are refused after decoding
                assert 6 <= t.stats()["gpu_decoded_images"] <= 8
        assert files[0] == lowlevel.transcode_host(sources[0], optimized_huffman=True)  # identity images give today's bytes
        # the regions were consumed by that batch; a count that differs from the batch's size is refused
        statuses, files = t.transcode(sources[:2], optimized_huffman=True)
        assert files == [lowlevel.transcode_host(s, optimized_huffman=True) for s in sources[:2]]
        R = (N.TranscodeRegion * 3)()
        assert N.load().hipjpegTranscodeBatchSetRegions(t._h, R, 3) == 0
        with pytest.raises(N.HipJpegError) as e:
            t.transcode(sources[:2], optimized_huffman=True)
        assert e.value.status == C.INVALID_ARGUMENT
        statuses, _ = t.transcode(sources[:2], optimized_huffman=True)
        assert statuses == [0, 0]
    finally:
        t.close()


def _croppable():
    out = []
    for name, data in _DECODE:
        try:
            region = C.recipe_region(data)
        except Exception:
            region = None
        if region is not None:
            out.append((name, data, region))
    return out


@pytest.mark.parametrize("orientation", range(1, 9))
def test_all_croppable_decode_goldens_in_one_batch(transcoder, orientation):
    picked = _croppable()
    sources, regions = [d for _, d, _ in picked], [r for _, _, r in picked]
    model = [C.expected(d, orientation, True, r) for d, r in zip(sources, regions)]
    want = [_host(d, optimized_huffman=True, orientation=orientation, trim=True, region=r) for d, r in zip(sources, regions)]
    for gpu in (True, False):
        statuses, files = transcoder.transcode(sources, optimized_huffman=True, orientation=orientation, trim=True, region=regions, gpu_huffman=gpu)
        assert statuses == [m["status"] for m in model], gpu
        bad = [n for (n, _, _), a, (_, b) in zip(picked, files, want) if a != b]
        assert not bad, (gpu, bad)
        assert transcoder.stats()["relayout_blocks"] == sum(m["blocks"] for m in model if m["status"] == T.SUCCESS)


def test_grayscale_and_markers_over_the_goldens(transcoder):
    sources = [d for _, d in _DECODE[::2]]
    tagged = [d[:2] + M.exif_segment(1 + k % 8, k % 2 == 0) + b"\xff\xfe\x00\x04ok" + d[2:] for k, d in enumerate(sources)]
    for kw in (dict(optimized_huffman=True, grayscale=True), dict(progressive=True, grayscale=True, copy_markers=True, from_exif=True, trim=True)):
        want = [_host(d, **kw) for d in tagged]
        assert sum(st == 0 for st, _ in want) >= 40
        for gpu in (True, False):
            statuses, files = transcoder.transcode(tagged, gpu_huffman=gpu, **kw)
            assert statuses == [st for st, _ in want] and files == [f for _, f in want], (kw, gpu)


def test_pixels_on_the_device(transcoder):
    """Decoding the cropped files without fancy upsampling = decoding the sources with the same region through
    hipjpegDecodeBatchSetTransforms, exactly: the region starts on an iMCU, so every sample goes through the same arithmetic."""
    picked = [(d, r) for _, d, r in _croppable() if C.expected(d, 1, False, r)["status"] == T.SUCCESS]
    assert len(picked) >= 75
    sources, regions = [d for d, _ in picked], [r for _, r in picked]
    statuses, files = transcoder.transcode(sources, optimized_huffman=True, region=regions)
    assert statuses == [0] * len(picked)
    dec = lowlevel.BatchDecoder(device=0, num_threads=8)
    try:
        a, sa = dec.decode(files, fmt="rgb", fancy=False, gpu_huffman=True)
        a = [x.cpu().numpy() for x in a]
        b, sb = dec.decode(sources, fmt="rgb", fancy=False, gpu_huffman=True, transforms=[(r, 1) for r in regions])
        b = [x.cpu().numpy() for x in b]
    finally:
        dec.close()
    assert list(sa) == [0] * len(picked) and list(sb) == [0] * len(picked)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)


def test_hipimtrans_crop_grayscale_copy_markers(tmp_path):
    assert os.path.exists(TOOL), "build the tool: make -C nvimagecodec_amd/csrc"
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    picked = [(n, d) for n, d in _DECODE if oracle.read_info(d)["ncomp"] == 3 and min(oracle.read_info(d)["width"], oracle.read_info(d)["height"]) >= 48
              and _host(d, grayscale=True)[0] == 0][::3][:10]
    assert len(picked) == 10
    tagged = {}
    for k, (name, data) in enumerate(picked):
        tagged[name] = data[:2] + M.exif_segment(6, k % 2 == 0) + b"\xff\xfe\x00\x06note" + data[2:]
        (src / (name + ".jpg")).write_bytes(tagged[name])
    p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst), "-b", "4", "-w", "1", "--lossless", "--crop", "29x31+11+8", "--expand", "--grayscale",
                        "--copy-markers", "--orientation", "6", "--trim", "--optimized_huffman", "true"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Total images: 10 (failed: 0, unsupported: 0)" in p.stdout
    for name, _ in picked:
        want = lowlevel.transcode_host(tagged[name], optimized_huffman=True, orientation=6, trim=True, region=(11, 8, 40, 39), expand=True, grayscale=True,
                                       copy_markers=True)
        assert (dst / (name + ".jpg")).read_bytes() == want, name
        assert lowlevel.exif_orientation(want) == 1 and b"note" in want and oracle.read_info(want)["ncomp"] == 1
    for extra in (["--crop", "16x16+0+0"], ["--expand"], ["--grayscale"], ["--copy-markers"]):
        p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst)] + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "--lossless" in p.stderr
    p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst), "--lossless", "--crop", "16x16"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
