"""The encode path at the edges of the 8-bit range and of the quality scale, on the CPU: saturated pictures (helpers/extreme_images.py) at
qualities 1, 75 and 100 against libjpeg-turbo's own files (tests/golden/encode_extreme, written by make_golden_encode_extreme.py), the
quantization tables of every quality, and the host entropy coders -- the plain one and the GPU coders' algorithms run on the host -- on
the coefficients those pictures give: DC differences of category 11, AC magnitudes near 1023, blocks without a single zero.  The GPU side
of the same content is tests/test_gpu_encode_extremes.py; this file pins the reference it compares with."""
import functools
import hashlib
import io
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers.extreme_images import PATTERNS, dqt_tables, extreme_image, extremes_reached
from nvimagecodec_amd import lowlevel

with open(os.path.join(GOLDEN, "manifest_encode_extreme.json")) as _f:
    _ME = json.load(_f)["encode_extreme"]
with open(os.path.join(GOLDEN, "quant_tables_q1_100.json")) as _f:
    _QT = json.load(_f)["tables"]

SIZES = ((8, 8), (17, 13), (40, 24))
QUALITIES = (1, 75, 100)
_FACTORS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2), "411": (4, 1), "410": (4, 2), "gray": (1, 1)}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _entries(pattern):
    return [e for e in _ME if e["pattern"] == pattern]


@functools.lru_cache(maxsize=None)
def _image(pattern, w, h, seed):
    im = extreme_image(pattern, w, h, seed)
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def _forward(pattern, w, h, seed, sub, q):
    return oracle.forward(_image(pattern, w, h, seed), sub, q)[0]


def _golden(e):
    with open(os.path.join(GOLDEN, "encode_extreme", e["name"] + ".jpg"), "rb") as f:
        return f.read()


def real_blocks(w, h, sub):
    """(width_in_blocks, height_in_blocks) per component: the blocks that carry samples of the picture"""
    hs, vs = _FACTORS[sub]
    luma = ((w + 7) // 8, (h + 7) // 8)
    if sub == "gray":
        return [luma]
    chroma = (((w + hs - 1) // hs + 7) // 8, ((h + vs - 1) // vs + 7) // 8)
    return [luma, chroma, chroma]


def assert_decodes_to(jpeg, coefs, w, h, sub, what):
    got, _ = oracle.decode_coefficients(jpeg)
    assert len(got) == len(coefs), what
    for c, ((rw, rh), g, r) in enumerate(zip(real_blocks(w, h, sub), got, coefs)):
        assert np.array_equal(g[:rh, :rw], r[:rh, :rw]), (what, c)


def _all_cases(pattern):
    """the manifest's cases of one pattern plus the samplings Pillow cannot write, from oracle.forward alone"""
    cases = [(e["width"], e["height"], e["seed"], e["sub"], e["quality"]) for e in _entries(pattern)]
    seeds = {(e["width"], e["height"]): e["seed"] for e in _entries(pattern)}
    for (w, h) in SIZES:
        for sub in ("440", "411", "410"):
            for q in QUALITIES:
                cases.append((w, h, seeds[(w, h)], sub, q))
    return cases


def test_manifest_is_complete_and_inputs_reproduce():
    assert len(_ME) == len(PATTERNS) * len(SIZES) * 4 * len(QUALITIES)
    assert {e["quality"] for e in _ME} == set(QUALITIES) and {e["sub"] for e in _ME} == {"444", "422", "420", "gray"}
    for e in _ME:
        with open(os.path.join(GOLDEN, "encode_extreme", e["input"]), "rb") as f:
            raw = f.read()
        assert _sha(raw) == e["rgb_sha256"], e["input"]
        assert _image(e["pattern"], e["width"], e["height"], e["seed"]).tobytes() == raw, e["input"]
        assert _sha(_golden(e)) == e["jpeg_sha256"], e["name"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_oracle_encode_matches_libjpeg_turbo_at_the_extremes(pattern):
    """as test_oracle_golden.py::test_oracle_encode_matches_libjpeg_turbo_bitstream: tables, coefficients and scan bytes"""
    for e in _entries(pattern):
        rgb = _image(pattern, e["width"], e["height"], e["seed"])
        jpeg = _golden(e)
        mine = oracle.encode(rgb, e["sub"], e["quality"])
        c_ref, q_ref = oracle.decode_coefficients(jpeg)
        c_mine, q_mine = oracle.decode_coefficients(mine)
        assert len(q_ref) == len(q_mine) == (1 if e["sub"] == "gray" else 3)
        for a, b in zip(q_ref, q_mine):
            assert np.array_equal(a, b), e["name"]
        for a, b in zip(c_ref, c_mine):
            assert np.array_equal(a, b), e["name"]
        assert oracle.scan_bytes(mine) == oracle.scan_bytes(jpeg), e["name"]
        # and oracle.forward, which the GPU tests compare coefficients with, is what went into that file
        assert_decodes_to(jpeg, _forward(pattern, e["width"], e["height"], e["seed"], e["sub"], e["quality"]), e["width"], e["height"], e["sub"],
                          e["name"])


def test_quality_tables_equal_libjpeg_turbos_for_every_quality():
    assert sorted(_QT, key=int) == [str(q) for q in range(1, 101)]
    for q in range(1, 101):
        luma, chroma = oracle.quality_tables(q)
        assert luma.tolist() == _QT[str(q)]["luma"], q
        assert chroma.tolist() == _QT[str(q)]["chroma"], q
        assert dqt_tables(oracle.encode(_image("noise", 8, 8, 1), "444", q)) == {0: _QT[str(q)]["luma"], 1: _QT[str(q)]["chroma"]}, q
    assert max(_QT["1"]["luma"]) == 255 and set(_QT["100"]["luma"]) == {1} and set(_QT["100"]["chroma"]) == {1}


@pytest.mark.parametrize("pattern", PATTERNS)
def test_host_coders_write_the_oracles_file(pattern):
    """the host coder and the GPU coder's baseline algorithm on the host, restart intervals 0, 1 and 3: whole files, byte for byte"""
    for (w, h, seed, sub, q) in _all_cases(pattern):
        rgb = _image(pattern, w, h, seed)
        coefs = _forward(pattern, w, h, seed, sub, q)
        for r in (0, 1, 3):
            want = oracle.encode(rgb, sub, q, restart_interval=r)
            assert lowlevel.encode_from_coefficients_host(w, h, coefs, sub, q, restart_interval=r) == want, (w, h, sub, q, r)
            assert lowlevel.encode_from_coefficients_baseline_gpu_algorithm_host(w, h, coefs, sub, q, restart_interval=r) == want, (w, h, sub, q, r)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_progressive_coders_agree_and_keep_the_coefficients(pattern):
    for (w, h, seed, sub, q) in _all_cases(pattern):
        coefs = _forward(pattern, w, h, seed, sub, q)
        want = lowlevel.encode_from_coefficients_host(w, h, coefs, sub, q, progressive=True)
        got = lowlevel.encode_from_coefficients_gpu_algorithm_host(w, h, coefs, sub, q, progressive=True)
        assert got == want, (w, h, sub, q)
        assert oracle.read_info(want)["sof"] == 0xC2
        assert_decodes_to(want, coefs, w, h, sub, (w, h, sub, q))


def test_the_inputs_reach_what_they_are_for():
    """so that the set cannot quietly lose its edge: a DC difference of category 11, AC magnitudes of category 10, Cb and Cr at both ends
    of their range (where forward_pair_kernel's unmasked chroma packing is tight), a flat 0 block (the 16-bit column pass's bound)"""
    cases = []
    for e in _ME:
        if e["sub"] == "444" and e["quality"] == 100:
            cases.append((_image(e["pattern"], e["width"], e["height"], e["seed"]),
                          _forward(e["pattern"], e["width"], e["height"], e["seed"], "444", 100)))
    dc, ac, cbs, crs = extremes_reached(cases)
    assert dc >= 1024, dc
    assert ac >= 512, ac
    assert {0, 255} <= cbs and {0, 255} <= crs
    black = _forward("black", 8, 8, next(e["seed"] for e in _ME if e["input"] == "black_8x8.rgb"), "444", 100)
    assert black[0][0, 0, 0] == -1024 and not black[0][0, 0, 1:].any()
    # 65535 >> 16 and 16777215 >> 16: the two sums the packing argument names
    assert (-11059 * 255 - 21709 * 255 + (128 << 16) + 32767, 32768 * 255 + (128 << 16) + 32767) == (65535, 16777215)


def test_live_sweep_of_every_quality_against_pillow():
    """every pattern at one ragged size, every quality from 1 to 100, the four samplings Pillow writes: scan bytes and tables"""
    try:
        from PIL import Image, features
    except ImportError:
        pytest.skip("Pillow is not installed")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow is not built against libjpeg-turbo")
    w, h = 17, 13
    for pattern in PATTERNS:
        rgb = _image(pattern, w, h, 7)
        im = Image.fromarray(rgb)
        gray = im.convert("L")
        for sub, code in (("444", 0), ("422", 1), ("420", 2), ("gray", None)):
            for q in range(1, 101):
                b = io.BytesIO()
                if sub == "gray":
                    gray.save(b, "JPEG", quality=q)
                else:
                    im.save(b, "JPEG", quality=q, subsampling=code)
                ref = b.getvalue()
                mine = oracle.encode(rgb, sub, q)
                assert oracle.scan_bytes(mine) == oracle.scan_bytes(ref), (pattern, sub, q)
                assert dqt_tables(mine) == dqt_tables(ref), (pattern, sub, q)
