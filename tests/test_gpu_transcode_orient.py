"""Lossless turns on the device: hipjpegTranscodeBatch with an orientation per image.  Turned images go through coef_transform_kernel,
the others through coef_relayout_kernel; whichever entropy routes an image takes, its file is the one hipjpegTranscodeHost writes for
the same orientation (tests/test_transcode_orient_host.py pins that one against the numpy model), byte for byte."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from helpers import sequential_scans as S
from helpers import transcode_cases as T
from helpers import transform_model as M
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(N.LIB_PATH), "hipimtrans")
_DECODE = T.golden_files("decode")
ORIENTATIONS = range(2, 9)


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


def _img(w, h, sub, seed, q=88, **kw):
    return oracle.encode(synth_image(w, h, seed=seed), sub, q, **kw)


@functools.lru_cache(maxsize=None)
def _small_shapes():
    return (oracle.encode(synth_image(8, 8, seed=3), "gray", 90),   # one block
            _img(16, 16, "420", 14),                                 # one MCU: the mirror happens inside it
            _img(48, 32, "422", 15), _img(32, 48, "440", 16),        # 2x1 <-> 1x2
            _img(33, 47, "420", 4), _img(50, 37, "420", 5),          # ragged both ways
            _img(129, 70, "411", 7),                                 # mirrors only: transposing 4x1 is refused
            _img(2049, 16, "444", 8))                                # 257 blocks per row <-> 2 per row over 257 rows: units end mid-row


@pytest.mark.parametrize("target", ["optimized", "progressive"])
@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_small_shapes(transcoder, orientation, target):
    sources = list(_small_shapes())
    kw = dict(T.TARGETS[target], orientation=orientation, trim=orientation != 5)
    want = [_host(s, **kw) for s in sources]
    refused = [i for i, (st, _) in enumerate(want) if st != T.SUCCESS]
    assert refused == ([6] if orientation in M.TRANSPOSES else []) and all(want[i][0] == T.UNSUPPORTED for i in refused)
    for gpu in (True, False):
        statuses, files = transcoder.transcode(sources, gpu_huffman=gpu, **kw)
        assert statuses == [st for st, _ in want], (gpu, statuses)
        for i, (a, (_, b)) in enumerate(zip(files, want)):
            assert a == b, (gpu, i, kw)
    if target == "optimized":  # the ragged pictures turn untrimmed only when nothing is mirrored; perfect mode refuses them otherwise
        statuses, _ = transcoder.transcode(sources[4:6], orientation=orientation)
        assert statuses == [T.SUCCESS if orientation == 5 else T.UNSUPPORTED] * 2


@pytest.mark.parametrize("orientation", ORIENTATIONS)
def test_all_decode_goldens_in_one_batch(transcoder, orientation):
    sources = [d for _, d in _DECODE]
    model = [M.expected(d, orientation, True) for d in sources]
    want = [_host(d, optimized_huffman=True, orientation=orientation, trim=True) for d in sources]
    for gpu in (True, False):
        statuses, files = transcoder.transcode(sources, optimized_huffman=True, orientation=orientation, trim=True, gpu_huffman=gpu)
        assert statuses == [m["status"] for m in model], gpu
        bad = [n for (n, _), a, (_, b) in zip(_DECODE, files, want) if a != b]
        assert not bad, (gpu, bad)
        assert transcoder.stats()["relayout_blocks"] == sum(m["blocks"] for m in model if m["status"] == T.SUCCESS)


def test_mixed_batch():
    """identity and the seven turns interleaved, with a refused, a truncated and a host-decoded (below the hybrid threshold) image"""
    t = lowlevel.BatchTranscoder(device=0, num_threads=4, gpu_huffman=True)
    try:
        t.set_hybrid_huffman_threshold(100 * 100)
        whole = _img(64, 48, "444", 40)
        sources, orientations = [], []
        for k in range(1, 9):
            sources += [_img(160 + 16 * k, 128, "420", 20 + k), _img(64, 48, "444", 30 + k)]  # GPU-decoded, host-decoded dense
            orientations += [k, 9 - k]
        sources += [_img(129, 70, "411", 7), whole[: len(whole) * 2 // 3], _img(33, 47, "420", 4)]
        orientations += [5, 6, 3]  # refused (4x1 transposed), truncated, refused (perfect mode)
        want = [_host(s, optimized_huffman=True, orientation=o) for s, o in zip(sources, orientations)]
        assert [st for st, _ in want][-3:] == [T.UNSUPPORTED, T.TRUNCATED, T.UNSUPPORTED] and all(st == T.SUCCESS for st, _ in want[:-3])
        for gpu in (True, False):
            statuses, files = t.transcode(sources, optimized_huffman=True, orientation=orientations, gpu_huffman=gpu)
            assert statuses == [st for st, _ in want], gpu
            assert files == [f for _, f in want], gpu
            if gpu:
                assert t.stats()["gpu_decoded_images"] == 8
        # identity images give today's bytes
        identity = [i for i, o in enumerate(orientations) if o == 1]
        assert len(identity) == 2 and all(files[i] == lowlevel.transcode_host(sources[i], optimized_huffman=True) for i in identity)
    finally:
        t.close()


def test_multiscan_restart_and_progressive_sources(transcoder):
    base = _img(40, 48, "420", 9)
    multiscan = S.recode(base, [[0], [1], [2]])
    restart = _img(48, 32, "420", 10, restart_interval=2)
    progressive = next(d for _, d in _DECODE if lowlevel.get_image_info(d)["sof_marker"] == 0xC2 and M.expected(d, 6, True)["status"] == T.SUCCESS)
    sources = [multiscan, restart, progressive]
    for target in ("optimized", "progressive", "annexk_rst3"):
        kw = dict(T.TARGETS[target], orientation=6, trim=True)
        want = [lowlevel.transcode_host(s, **kw) for s in sources]
        assert want[0] == lowlevel.transcode_host(base, **kw)
        for gpu in (True, False):
            statuses, files = transcoder.transcode(sources, gpu_huffman=gpu, **kw)
            assert statuses == [0, 0, 0] and files == want, (target, gpu)


@pytest.mark.parametrize("orientation", [2, 3, 4])
def test_pixels_on_the_device(transcoder, orientation):
    """Decoding the mirrored file = decoding the source with the geometry pass mirroring the pixels.  Exact for the vertical mirror of
    gray and 4:4:4 sources; a horizontal mirror leaves the IDCT's first pass up to 2 levels off (tests/test_transcode_orient_host.py
    measured it on the host, where the claim of exactness for 2 and 3 met its counter-example), so 2 and 3 get that file's bound."""
    from test_transcode_orient_host import PIXEL_BOUND
    picked = []
    for _, d in _DECODE:
        info = oracle.read_info(d)
        if (info["ncomp"] == 1 or (info["hmax"], info["vmax"]) == (1, 1)) and M.kept_size(info, orientation, False) is not None:
            picked.append(d)
    assert len(picked) >= 10
    statuses, files = transcoder.transcode(picked, optimized_huffman=True, orientation=orientation)
    assert statuses == [0] * len(picked)
    dec = lowlevel.BatchDecoder(device=0, num_threads=8)
    try:
        a, sa = dec.decode(files, fmt="rgb", gpu_huffman=True)
        a = [x.cpu().numpy() for x in a]
        b, sb = dec.decode(picked, fmt="rgb", gpu_huffman=True, transforms=[(None, orientation)] * len(picked))
        b = [x.cpu().numpy() for x in b]
    finally:
        dec.close()
    assert list(sa) == [0] * len(picked) and list(sb) == [0] * len(picked)
    for x, y in zip(a, b):
        assert x.shape == y.shape
        d = int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max())
        assert d <= (0 if orientation == 4 else PIXEL_BOUND)


def test_hipimtrans_orientation_from_exif(tmp_path):
    assert os.path.exists(TOOL), "build the tool: make -C nvimagecodec_amd/csrc"
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    picked = [(n, d) for n, d in _DECODE if oracle.read_info(d)["hmax"] <= 2 and min(oracle.read_info(d)["width"], oracle.read_info(d)["height"]) >= 16][::7][:10]
    assert len(picked) == 10
    tagged = {}
    for k, (name, data) in enumerate(picked):
        tagged[name] = M.with_segment(data, M.exif_segment(k % 8 + 1, k % 2 == 0))
        (src / (name + ".jpg")).write_bytes(tagged[name])
    p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst), "-b", "4", "-w", "1", "--lossless", "--orientation", "exif", "--trim",
                        "--optimized_huffman", "true"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Total images: 10 (failed: 0, unsupported: 0)" in p.stdout
    for k, (name, data) in enumerate(picked):
        want = lowlevel.transcode_host(data, optimized_huffman=True, orientation=k % 8 + 1, trim=True)
        assert want == lowlevel.transcode_host(tagged[name], optimized_huffman=True, from_exif=True, trim=True)
        assert (dst / (name + ".jpg")).read_bytes() == want, name
    for extra in (["--orientation", "6"], ["--trim"]):
        p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst)] + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "--lossless" in p.stderr
    p = subprocess.run([TOOL, "-i", str(src), "-o", str(dst), "--lossless", "--orientation", "9"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
