"""The sampling-layout goldens: every legal JPEG sampling layout beyond the seven a stock encoder writes, as files written from chosen
coefficients (helpers/jpeg_from_coefficients.py) and libjpeg-turbo's hashes of their pixels (tests/golden/manifest_sampling.json, made by
tests/golden/make_golden_sampling.py).  The files are rebuilt here, byte for byte: the manifest pins their sha256 too.

  * stock ratios with larger factors (Y 2x1 + C 2x1 is "444", Y 2x2 + C 1x2 "422", ...) and 410V (Y 2x4, C 1x1);
  * layouts only replication reaches: factor 3, factor 4 vertically, luma below the maximum, Cb != Cr;
  * one-component frames with factors above 1 (non-interleaved scans over the real blocks of an MCU-padded grid);
  * four-component frames (CMYK / YCCK / no Adobe segment) that need the h2v2, h1v2 and h2v1 triangle filters or ratio 3;
  * progressive files (libjpeg's default script), restart intervals, Adobe transform 0 (RGB) on three components;
  * layouts libjpeg refuses (more than 10 blocks per MCU, a fractional ratio).
Sizes put MCU padding and ragged edges everywhere; 264 px wide files reach the tile paths of the pixel kernels, 4 px wide ones the
"downsampled_width > 2" rule of jdsample.c."""
import functools
import hashlib
import json
import os

import numpy as np

from helpers import jpeg_from_coefficients as jc

MANIFEST_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "manifest_sampling.json")

THREE = {
    "y21c21": [(2, 1), (2, 1), (2, 1)], "y12c12": [(1, 2), (1, 2), (1, 2)], "y22c12": [(2, 2), (1, 2), (1, 2)],
    "y22c21": [(2, 2), (2, 1), (2, 1)], "y24c11": [(2, 4), (1, 1), (1, 1)],
    "y31c11": [(3, 1), (1, 1), (1, 1)], "y32c11": [(3, 2), (1, 1), (1, 1)], "y13c11": [(1, 3), (1, 1), (1, 1)],
    "y14c11": [(1, 4), (1, 1), (1, 1)], "y11c22": [(1, 1), (2, 2), (2, 2)],
    "y22cb11cr21": [(2, 2), (1, 1), (2, 1)], "y21cb11cr21": [(2, 1), (1, 1), (2, 1)], "y41cb21cr11": [(4, 1), (2, 1), (1, 1)],
}
GRAY = {"gray22": [(2, 2)], "gray12": [(1, 2)], "gray21": [(2, 1)], "gray44": [(4, 4)], "gray31": [(3, 1)]}
FOUR = {"k22111122": [(2, 2), (1, 1), (1, 1), (2, 2)], "k12111112": [(1, 2), (1, 1), (1, 1), (1, 2)],
        "k22211211": [(2, 2), (2, 1), (1, 2), (1, 1)], "k11111122": [(1, 1), (1, 1), (1, 1), (2, 2)],
        "k31111131": [(3, 1), (1, 1), (1, 1), (3, 1)]}
REFUSED_LAYOUTS = {"y42c21": [(4, 2), (2, 1), (2, 1)], "y24c12": [(2, 4), (1, 2), (1, 2)], "y31cb21cr11": [(3, 1), (2, 1), (1, 1)]}
WIDE = {"y21c21", "y12c12", "y22c12", "y22c21", "y24c11", "y31c11", "y11c22", "gray22"}    # + 264 x 16: the tile paths
NARROW = {"y21cb11cr21", "y22cb11cr21", "y41cb21cr11", "y11c22", "k22111122", "k22211211", "k11111122"}  # + 4 x 6: downsampled width <= 2
# libjpeg's default progressive script (jcparam.c jpeg_simple_progression)
PROG3 = [("dc", [0, 1, 2], 0, 1), ("ac", 0, 1, 5, 0, 2), ("ac", 2, 1, 63, 0, 1), ("ac", 1, 1, 63, 0, 1), ("ac", 0, 6, 63, 0, 2),
         ("ac", 0, 1, 63, 2, 1), ("dc", [0, 1, 2], 1, 0), ("ac", 2, 1, 63, 1, 0), ("ac", 1, 1, 63, 1, 0), ("ac", 0, 1, 63, 1, 0)]
PROG1 = [("dc", [0], 0, 1), ("ac", 0, 1, 5, 0, 2), ("ac", 0, 6, 63, 0, 2), ("ac", 0, 1, 63, 2, 1), ("dc", [0], 1, 0), ("ac", 0, 1, 63, 1, 0)]


def _case(name, layout, samp, w, h, kind, adobe=None, progressive=False, restart_interval=0):
    return dict(name=name, layout=layout, sampling=[list(s) for s in samp], width=w, height=h, kind=kind, adobe=adobe,
                progressive=progressive, restart_interval=restart_interval)


def _cases():
    cases = []
    for layout, samp in list(THREE.items()) + list(GRAY.items()):
        sizes = [(83, 61), (17, 9), (8, 8)] + ([(264, 16)] if layout in WIDE else []) + ([(4, 6)] if layout in NARROW else [])
        cases += [_case("%s_%dx%d" % (layout, w, h), layout, samp, w, h, "ycc" if len(samp) == 3 else "gray") for w, h in sizes]
    for layout, samp in FOUR.items():
        kinds = [(83, 61, "adobe0"), (83, 61, "adobe2"), (17, 9, "plain"), (8, 8, "adobe2")] + ([(4, 6, "adobe0")] if layout in NARROW else [])
        cases += [_case("%s_%dx%d_%s" % (layout, w, h, k), layout, samp, w, h, k, {"adobe0": 0, "adobe2": 2, "plain": None}[k]) for w, h, k in kinds]
    for layout, w, h in (("y21c21", 17, 9), ("y31c11", 83, 61)):
        cases.append(_case("%s_%dx%d_rgb" % (layout, w, h), layout, THREE[layout], w, h, "rgb", adobe=0))
    for layout in ("gray22", "y21c21", "y24c11", "y31c11"):
        samp = GRAY.get(layout) or THREE[layout]
        cases.append(_case(layout + "_83x61_prog", layout, samp, 83, 61, "gray" if len(samp) == 1 else "ycc", progressive=True))
    cases.append(_case("y22c12_83x61_rst2", "y22c12", THREE["y22c12"], 83, 61, "ycc", restart_interval=2))
    cases.append(_case("gray22_83x61_rst3", "gray22", GRAY["gray22"], 83, 61, "gray", restart_interval=3))
    return cases


def coefficients(name, w, h, sampling):
    """In-gamut blocks (the SIMD and the C IDCT of libjpeg-turbo agree on them); a one-component frame's padding blocks stay zero
    (they are not coded, decoders give zeros back)"""
    rng = np.random.default_rng(sum(map(ord, "%s_%dx%d" % (name, w, h))))
    coefs = jc.random_coefficients(rng, w, h, sampling, 6, dense=6, small=2, dc=40)
    if len(sampling) == 1:
        coefs[0][-(-h // 8):] = 0
        coefs[0][:, -(-w // 8):] = 0
    return coefs


def build(case):
    """The file of a case, as bytes"""
    samp, w, h = [tuple(s) for s in case["sampling"]], case["width"], case["height"]
    coefs = coefficients(case["name"], w, h, samp)
    qt = [np.full(64, 5 + c, dtype=np.int32) for c in range(len(samp))]
    if case["progressive"]:
        return jc.write_progressive(w, h, samp, coefs, qt, PROG1 if len(samp) == 1 else PROG3)
    return jc.write_baseline(w, h, samp, coefs, qt, adobe=case["adobe"], restart_interval=case["restart_interval"])


CASES = _cases()
REFUSED_CASES = [_case(layout + "_83x61", layout, samp, 83, 61, "ycc") for layout, samp in REFUSED_LAYOUTS.items()]

if os.path.exists(MANIFEST_PATH):
    with open(MANIFEST_PATH) as _f:
        MANIFEST = json.load(_f)
    _H = {e["name"]: e for e in MANIFEST["sampling"] + MANIFEST["refused"]}
    ENTRIES = [dict(c, **_H[c["name"]]) for c in CASES]
    REFUSED = [dict(c, **_H[c["name"]]) for c in REFUSED_CASES]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _jpeg(name):
    case = next(c for c in CASES + REFUSED_CASES if c["name"] == name)
    return build(case)


def jpeg(entry):
    """the file of a manifest entry; its bytes are the ones libjpeg-turbo's hashes were taken from"""
    data = _jpeg(entry["name"])
    assert hashlib.sha256(data).hexdigest() == entry["jpeg_sha256"], ("the writer no longer writes this golden", entry["name"])
    return data


def ratios(sampling):
    """per component (hmax / h, vmax / v)"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    return [(hmax // h, vmax // v) for h, v in sampling]


def replicate(plane, fx, fy, width, height):
    return np.repeat(np.repeat(plane.astype(np.int64), fy, axis=0), fx, axis=1)[:height, :width]


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert (int arrays in, H x W x 3 uint8 out)"""
    r = y + ((cr * 91881 + 32768 - 128 * 91881) >> 16)
    g = y + ((cb * -22554 + cr * -46802 + 32768 + 128 * 22554 + 128 * 46802) >> 16)
    b = y + ((cb * 116130 + 32768 - 128 * 116130) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def libjpeg_upsampler(h, v, hmax, vmax, dw, fancy):
    """The method libjpeg-turbo's jinit_upsampler (jdsample.c) picks for a component of factors h x v and downsampled width dw"""
    if h == hmax and v == vmax:
        return "fullsize"
    if h * 2 == hmax and v == vmax:
        return "h2v1_fancy" if fancy and dw > 2 else "h2v1"
    if h == hmax and v * 2 == vmax and fancy:
        return "h1v2_fancy"
    if h * 2 == hmax and v * 2 == vmax:
        return "h2v2_fancy" if fancy and dw > 2 else "h2v2"
    if hmax % h == 0 and vmax % v == 0:
        return "int"
    return "refused"


def luma_kernel_layout(sampling):
    """The luma kernels (luma_color_kernel<HS, VS>) take a full-size luma with both chroma components at one ratio of at most 2 each
    way; they carry the triangle filters.  Every other three-component layout is replicated (generic_color_kernel)."""
    (fx1, fy1), (fx2, fy2) = ratios(sampling)[1:3]
    return ratios(sampling)[0] == (1, 1) and (fx1, fy1) == (fx2, fy2) and fx1 <= 2 and fy1 <= 2


def expected_unsupported(entry, fmt, fancy):
    """Whether the decoder is to decline this file in this output format: four components have no raw planes; `y` is the luma plane,
    so it needs a full-size luma of a Y'CbCr frame; a replicated layout declines when libjpeg would filter a component instead."""
    samp, W = entry["sampling"], entry["width"]
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    if any(libjpeg_upsampler(h, v, hmax, vmax, 1, fancy) == "refused" for h, v in samp):
        return True
    if len(samp) == 4:
        return fmt == "yuv_planar"
    if fmt == "yuv_planar" or len(samp) == 1:
        return False
    if fmt == "y":
        return entry["kind"] == "rgb" or ratios(samp)[0] != (1, 1)
    if luma_kernel_layout(samp):
        return False
    return any(libjpeg_upsampler(h, v, hmax, vmax, -(-W * h // hmax), fancy).endswith("_fancy") for h, v in samp)
