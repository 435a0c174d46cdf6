"""Test helper: decode cases steered onto the seams of the pixel stage's STORES (csrc/decode_kernels.hip: K1, K2; csrc/plane_color_kernels.hip: the
kernels that read planes), the way steered_streams.py,
progressive_seams.py and coder_seams.py steer files onto the entropy kernels'.

The store code picks its path from the pointer, the pitch and the width together; a tightly packed output ties the three, so a case
here is a picture PLUS a placement inside a framed arena (helpers/framed_outputs.py).  Every case claims the classes it is meant to
reach (Case.seams); reached(case) restates the host's tile arithmetic (DecodeBatch::build_pixel_units) and the kernels' path conditions
in plain Python and says which classes the case really reaches; tests/test_pixel_seams.py (no GPU) asserts claim <= reached for every
case, the census REQUIRED <= union of the claims, and the restated constants and conditions against the sources as text.
tests/test_gpu_pixel_seams.py decodes the cases.

Families:  A  K2's staged interleaved store      B  K2's planar store          C  K1's stores to the output
           D  generic and CMYK colour kernels    E  geometry pass, regions     F  scaled decode
Pictures are synth_image + oracle.encode unless a case names a golden file; none is larger than 400 x 80 (the sources of the transposing
orientations stand: 16..18 x 262..264, so that the OUTPUT is 255..257 wide).  Plain numpy, the oracle and the goldens' manifests; no GPU."""
import collections
import functools
import json
import os

import numpy as np

import oracle
from helpers import ifast_idct
from helpers import scaled_goldens as S
from helpers.framed_outputs import Hashed
from helpers.geometry import upright
from nvimagecodec_amd.synth import synth_image

# ---------------------------------------------------------------- the sources' constants and conditions, restated
TILE_W = 32             # kLumaTileW: blocks per wide tile row
TILE_H = 4              # kLumaTileH: block rows per wide tile (narrow tiles: 16 x 8 blocks)
UNIT_BLOCKS = 128       # kBlocksPerUnit: blocks per workgroup of K1
XFORM_ROWS = 8          # kTransformRowsPerUnit
SCALED_ROWS = 8         # kScaledRowsPerUnit
THREADS = 256           # kThreads
NARROW_ROW_BYTES = 16 * 24   # kNarrowRowBytes
WIDE_ROW_BYTES = TILE_W * 24  # kBlocksPerWave * 24
# (file under nvimagecodec_amd/csrc, text that must stand in it); tests/test_pixel_seams.py looks every one up
SOURCE_TEXT = {
    "TILE": [("device_layout.h", "constexpr int kLumaTileW = %d, kLumaTileH = %d;" % (TILE_W, TILE_H)),
             ("decode_kernels.hip", "constexpr int kBlocksPerWave = %d;" % TILE_W)],
    "UNIT_BLOCKS": [("device_layout.h", "constexpr int kBlocksPerUnit = %d;" % UNIT_BLOCKS)],
    "XFORM_ROWS": [("device_layout.h", "constexpr int kTransformRowsPerUnit = %d;" % XFORM_ROWS)],
    "SCALED_ROWS": [("device_layout.h", "constexpr int kScaledRowsPerUnit = %d;" % SCALED_ROWS)],
    "THREADS": [("decode_kernel_common.h", "constexpr int kThreads = %d;" % THREADS)],
    "NARROW_ROW_BYTES": [("decode_kernels.hip", "constexpr int kNarrowRowBytes = 16 * 24;")],
    # DecodeBatch::build_pixel_units: luma_tiles() below
    "tiles": [("decoder_core.cpp", "first_row = (uint32_t)im.transform.y0 / 8 / kLumaTileH * kLumaTileH;"),
              ("decoder_core.cpp", "real_rows = std::min(real_rows, (uint32_t)(im.transform.y1 + 7) / 8);"),
              ("decoder_core.cpp", "first_col = (uint32_t)im.transform.x0 / 8 / kLumaTileW * kLumaTileW;"),
              ("decoder_core.cpp", "end_col = std::min(end_col, (uint32_t)(im.transform.x1 + 7) / 8);"),
              ("decoder_core.cpp", "const uint32_t span = end_col - first_col, ragged = span % kLumaTileW;"),
              ("decoder_core.cpp", "const uint32_t wide_end = (ragged != 0 && ragged <= kLumaTileW / 2) ? end_col - ragged : end_col;"),
              ("decoder_core.cpp", "for (uint32_t by = first_row; by < real_rows; by += kLumaTileH)"),
              ("decoder_core.cpp", "for (uint32_t by = first_row; by < real_rows; by += 2 * kLumaTileH) tiles.push_back(WorkUnit{(uint32_t)i, wide_end, by, 1u});"),
              ("decoder_core.cpp", "const uint32_t ipitch = (uint32_t)align_up((size_t)im.pic_w * t.bpp, 16);")],
    # luma_color_body's staged store: staged_waves() below
    "staged": [("decode_kernels.hip", "const int bx0 = u.block_base, by_wave = (int)u.comp + (narrow ? 2 * wave : wave);"),
               ("decode_kernels.hip", "if (!staged || by_wave >= bh || y0w >= H) return;"),
               ("decode_kernels.hip", "const int row_bytes = min((W - bx0 * 8) * 3, tile_row_bytes);"),
               ("decode_kernels.hip", "const int nrows = min(min(narrow ? 16 : 8, H - y0w), (bh - by_wave) * 8);"),
               ("decode_kernels.hip", "if (off + 16 <= row_bytes) {")],
    # luma_color_body's planar store: _reached_b() below
    "planar": [("decode_kernels.hip", "const bool full = x0 + 8 <= W;"),
               ("decode_kernels.hip", "if (full && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 7) == 0) {")],
    # idct_plane_body's store: _reached_c() below
    "k1": [("decode_kernels.hip", "const bool fast = (x0 + 8 <= lim_w) && (((uintptr_t)base | pitch) & 7) == 0;"),
           ("decode_kernels.hip", "const int lim_w = to_out ? cd.samp_w : bw * 8;")],
    # scaled_color_kernel: scaled_paths() below
    "scaled": [("plane_color_kernels.hip", "const int wide_groups = (direct && aligned16) ? (W >> 4) : 0;"),
               ("plane_color_kernels.hip", "for (int g = wide_groups * 4 + lane; g < groups; g += 64) {"),
               ("plane_color_kernels.hip", "const bool whole = aligned && n == 4;"),
               ("plane_color_kernels.hip", "const int x = g * 4, n = min(4, W - x);"),
               ("plane_color_kernels.hip", "const bool direct = k0.fx == 1 && k0.fy == 1 && (gray || (k1.fx == 1 && k1.fy == 1 && k2.fx == 1 && k2.fy == 1));")],
}

SAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2), "gray": (1, 1), "411": (4, 1), "410": (4, 2)}
FUSED = ("444", "422", "420", "440", "gray")  # what K2 (luma_color_kernel) takes
GOLDEN = S.GOLDEN

# name: unique; seams: the classes the case claims; source: ("synth", W, H, sub) | ("golden", set, name) | ("scaled", manifest name);
# fmt / fancy: the decode call's; place: keyword arguments of framed_outputs.Layout.add; roi / orientation: the transform or None / 1;
# scale: the denominator (1: full size)
Case = collections.namedtuple("Case", "name family seams source fmt fancy place roi orientation scale")


# ---------------------------------------------------------------- sources and geometry
@functools.lru_cache(maxsize=None)
def jpeg(source):
    if source[0] == "synth":
        _, w, h, sub = source
        img = synth_image(w, h, seed=w * 131 + h * 7 + len(sub))
        return oracle.encode(img[:, :, 1].copy() if sub == "gray" else img, sub, 88)
    if source[0] == "golden":
        with open(os.path.join(GOLDEN, source[1], source[2] + ".jpg"), "rb") as f:
            return f.read()
    return S.jpeg(S.by_name(source[1]))


@functools.lru_cache(maxsize=None)
def info(source):
    return oracle.read_info(jpeg(source))


def sub_of(source):
    """the sampling's name (SAMPLING's key) of a three- or one-component source"""
    i = info(source)
    if i["ncomp"] == 1:
        return "gray"
    hv = (i["hmax"] // i["h"][1], i["vmax"] // i["v"][1])
    return next(k for k, v in SAMPLING.items() if v == hv and k != "gray")


def picture_size(case):
    """(W, H) of the picture the pixel kernels produce: the file's, or the scaled one"""
    if case.scale != 1:
        sc = S.by_name(case.source[1])["scales"][str(case.scale)]
        return sc["width"], sc["height"]
    i = info(case.source)
    return i["width"], i["height"]


def output_shape(case):
    w, h = picture_size(case)
    if case.roi is not None:
        w, h = case.roi[2] - case.roi[0], case.roi[3] - case.roi[1]
    if case.orientation >= 5:
        w, h = h, w
    if case.fmt in ("rgb", "bgr"):
        return (h, w, 3)
    if case.fmt in ("rgb_planar", "bgr_planar"):
        return (3, h, w)
    if case.fmt == "y":
        return (h, w)
    i = info(case.source)
    return [(i["dh"][c], i["dw"][c]) for c in range(min(i["ncomp"], 3))]


def has_transform(case):
    w, h = picture_size(case)
    return case.orientation != 1 or (case.roi is not None and tuple(case.roi) != (0, 0, w, h))


def luma_grid(W, H, sub):
    """(blocks_w, blocks_h) of component 0: the MCU-padded grid"""
    hs, vs = SAMPLING[sub]
    return -(-W // (8 * hs)) * hs, -(-H // (8 * vs)) * vs


def luma_tiles(W, H, sub, roi=None):
    """DecodeBatch::build_pixel_units: the K2 tiles of a picture, (first block column, first block row, narrow)"""
    bw, _ = luma_grid(W, H, sub)
    real_rows, first_row, first_col, end_col = (H + 7) // 8, 0, 0, bw
    if roi is not None:
        x0, y0, x1, y1 = roi
        first_row = y0 // 8 // TILE_H * TILE_H
        real_rows = min(real_rows, (y1 + 7) // 8)
        first_col = x0 // 8 // TILE_W * TILE_W
        end_col = min(end_col, (x1 + 7) // 8)
    span = end_col - first_col
    ragged = span % TILE_W
    wide_end = end_col - ragged if (ragged != 0 and ragged <= TILE_W // 2) else end_col
    tiles = [(bx, by, False) for by in range(first_row, real_rows, TILE_H) for bx in range(first_col, wide_end, TILE_W)]
    if wide_end < end_col:
        tiles += [(wide_end, by, True) for by in range(first_row, real_rows, 2 * TILE_H)]
    return tiles


def tile_plan(W, H, sub, roi=None):
    """what luma_tiles derives on the way, for the predicates of the region cases"""
    bw, _ = luma_grid(W, H, sub)
    x0, y0, x1, y1 = roi
    first_col, end_col = x0 // 8 // TILE_W * TILE_W, min(bw, (x1 + 7) // 8)
    return dict(first_col=first_col, end_col=end_col, blocks_w=bw, ragged=(end_col - first_col) % TILE_W, first_row=y0 // 8 // TILE_H * TILE_H)


def staged_waves(W, H, sub, roi=None):
    """luma_color_body's staged store: one record per wave that stores -- (narrow, bx0, by_wave, row_bytes, nrows)"""
    _, bh = luma_grid(W, H, sub)
    out = []
    for bx0, by0, narrow in luma_tiles(W, H, sub, roi):
        for wave in range(4):
            by_wave = by0 + (2 * wave if narrow else wave)
            y0w = by_wave * 8
            if by_wave >= bh or y0w >= H:
                continue
            row_bytes = min((W - bx0 * 8) * 3, NARROW_ROW_BYTES if narrow else WIDE_ROW_BYTES)
            nrows = min(min(16 if narrow else 8, H - y0w), (bh - by_wave) * 8)
            assert row_bytes > 0 and nrows > 0
            out.append((narrow, bx0, by_wave, row_bytes, nrows))
    return out


def luma_layout(case):
    """the kernel flavour (LumaLayout) K2 runs a case's tiles with, or None where K2 does not run"""
    if case.scale != 1 or case.fmt in ("y", "yuv_planar") or case.source[0] == "golden" and case.source[1] == "cmyk":
        return None
    sub = sub_of(case.source)
    if sub not in FUSED:
        return None
    if sub == "gray" or not case.fancy:
        return 0
    return 1 if case.fmt in ("rgb", "bgr") else 2


def luma_units(cases):
    """[units of layout 0, 1, 2] that a batch of these cases gives K2 (hipjpegTestKernelFlavours' second array)"""
    n = [0, 0, 0]
    for c in cases:
        lay = luma_layout(c)
        if lay is not None:
            i = info(c.source)
            n[lay] += len(luma_tiles(i["width"], i["height"], sub_of(c.source), c.roi if has_transform(c) else None))
    return n


def plane_offsets(case):
    """(offsets modulo 256 of the output's planes, their pitches) as framed_outputs.Layout.add will place them"""
    shape, place = output_shape(case), case.place
    res = place.get("residue", 0)
    if case.fmt in ("rgb", "bgr", "y"):
        return [res], [place.get("pitch") or shape[1] * (1 if case.fmt == "y" else 3)]
    if case.fmt == "yuv_planar":
        return [r for _, r in place["planes"]], [p or s[1] for (p, _), s in zip(place["planes"], shape)]
    return [(res + k * place["plane_stride"]) % 256 for k in range(3)], [place.get("pitch") or shape[2]] * 3


# ---------------------------------------------------------------- reached(): the classes a case sits on, from the restated arithmetic
def _reached_a(case):
    w, h = picture_size(case)
    sub = sub_of(case.source)
    _, bh = luma_grid(w, h, sub)
    got = set()
    tiles = luma_tiles(w, h, sub)
    wide_cols = sorted({bx for bx, _, n in tiles if not n})
    for narrow, bx0, by_wave, row_bytes, nrows in staged_waves(w, h, sub):
        if narrow:
            where = "narrow0" if bx0 == 0 else "narrow32" if bx0 == 32 and wide_cols == [0] else None
        else:
            where = "wide_last" if bx0 == wide_cols[-1] and not any(n for _, _, n in tiles) else "wide_inner"
        if where:
            got.add("A.%s.r%d" % (where, row_bytes % 16))
        if row_bytes == (NARROW_ROW_BYTES if narrow else WIDE_ROW_BYTES):
            got.add("A.full_narrow" if narrow else "A.full_wide")
        got.add("A.%s.%s" % (sub, "narrow" if narrow else "wide"))
        if not narrow and h - by_wave * 8 < 8:
            got.add("A.rows_lt8")
        if narrow and nrows <= 8:
            got.add("A.narrow_first_only")
        if narrow and nrows == 9:
            got.add("A.narrow_second_one_row")
    if sub == "420" and (h + 7) // 8 < bh:
        got.add("A.padding_row")
    if h in (64, 65):
        got.add("A.h%d" % h)
    (off,), (pitch,) = plane_offsets(case)
    got.add("A.off%d" % (off % 16))
    got.add("A.pitch16" if pitch % 16 == 0 else "A.pitch_odd" if pitch % 2 else "A.pitch_other")
    got.add("A.%s" % ("plain" if not case.fancy else case.fmt))
    return got


def _reached_b(case):
    w, h = picture_size(case)
    sub = sub_of(case.source)
    offs, (pitch, _, _) = plane_offsets(case)
    shape = "narrow" if any(n for _, _, n in luma_tiles(w, h, sub)) else "wide"
    rows_fast = [all((o + y * pitch) % 8 == 0 for o in offs) for y in range(h)]  # (x0 is a multiple of 8)
    got = {"B.%s.%s" % (case.fmt, "fancy" if case.fancy else "plain")}
    if w % 8:
        if all(rows_fast):
            got.add("B.aligned_ragged." + shape)
        if any(rows_fast) and not all(rows_fast) and pitch % 2:
            got.add("B.odd_pitch." + shape)
        if pitch % 8 == 0 and sum(1 for o in offs if o % 8) == 1:
            got.add("B.one_misaligned." + shape)
    return got


def _reached_c(case):
    i = info(case.source)
    sub = sub_of(case.source)
    offs, pitches = plane_offsets(case)
    got = {"C.y_gray" if sub == "gray" else "C.y_colour"} if case.fmt == "y" else {"C.yuv" + sub}
    for c, (off, pitch) in enumerate(zip(offs, pitches)):
        samp_w, nblocks = i["dw"][c], i["bw"][c] * i["bh"][c]
        # idct_plane_body: base = dst + y0 * pitch + x0 with y0, x0 multiples of 8, so base & 7 == dst & 7
        aligned = off % 8 == 0 and pitch % 8 == 0
        if aligned and samp_w % 8 and samp_w > 8:
            got.add("C.aligned_ragged")
            if c > 0 and sub == "420":
                got.add("C.chroma_ragged")
        if off % 8 and pitch % 8 == 0:
            got.add("C.misaligned_base")
        if pitch % 8 and off % 8 == 0:
            got.add("C.pitch_not8")
        if nblocks > UNIT_BLOCKS and nblocks % UNIT_BLOCKS:
            got.add("C.multi_unit")
    return got


def _reached_d(case):
    if case.source[0] == "golden":
        return {"D.ycck" if info(case.source)["colorspace"] == 4 else "D.cmyk"}
    (_, pitch) = plane_offsets(case)
    w, _ = picture_size(case)
    return {"D.%s.w%d" % (sub_of(case.source), w)} if pitch[0] % 2 and pitch[0] > w * 3 else set()


def _reached_e(case):
    w, h = picture_size(case)
    shape = output_shape(case)
    oh, ow = (shape[1], shape[2]) if case.fmt.endswith("_planar") else (shape[0], shape[1])
    _, pitches = plane_offsets(case)
    if pitches[0] <= ow * (3 if case.fmt in ("rgb", "bgr") else 1):
        return set()
    got = {"E.o%d" % case.orientation, "E.w%d" % ow, "E.h%d" % oh, "E.fmt." + case.fmt, "E.o%d.%s" % (case.orientation, case.fmt)}
    if case.roi is not None:
        sub = sub_of(case.source)
        p = tile_plan(w, h, sub, case.roi)
        if p["first_col"] == TILE_W and 1 <= p["ragged"] <= TILE_W // 2 and p["end_col"] < p["blocks_w"] and p["first_row"] % 8 == 4:
            got.add("E.region." + ("gray" if sub == "gray" else "plain" if not case.fancy else case.fmt))
    return got


def scaled_paths(W, offs, pitches, direct):
    """scaled_color_kernel's choices for one output: (wide_groups, tail groups as (x, n), aligned, aligned16)"""
    aligned = all(v % 4 == 0 for v in list(offs) + list(pitches))
    aligned16 = all(v % 16 == 0 for v in list(offs) + list(pitches))
    wide_groups = W >> 4 if direct and aligned16 else 0
    tail = [(g * 4, min(4, W - g * 4)) for g in range(wide_groups * 4, (W + 3) >> 2)]
    return wide_groups, tail, aligned, aligned16


def _reached_f(case):
    w, h = picture_size(case)
    sub = sub_of(case.source)
    direct = sub in ("444", "420", "gray") or case.fmt == "y"
    got = {"F.fmt." + case.fmt, "F.direct" if direct else "F.upsampled", "F.w%d" % w, "F.denom%d" % case.scale}
    shape = output_shape(case)
    oh = shape[1] if case.fmt.endswith("_planar") else shape[0]  # (rows of the scaled kernel's workgroups, or of the geometry pass's)
    if SCALED_ROWS - 2 <= oh <= SCALED_ROWS + 1:
        got.add("F.h%d" % oh)
    if has_transform(case):
        return got | {"F.region"}
    offs, pitches = plane_offsets(case)
    wide_groups, tail, aligned, aligned16 = scaled_paths(w, offs, pitches, direct)
    ragged = any(n < 4 for _, n in tail)
    if wide_groups and tail:
        got.add("F.a16_tail")
        if ragged:
            got.add("F.a16_tail_ragged")
    if aligned and not aligned16 and ragged:
        got.add("F.a4_ragged")
    if not aligned:
        got.add("F.unaligned")
    if case.fmt.endswith("_planar") and sum(1 for o in offs if o % 4) == 1:
        got.add("F.one_plane_misaligned")
    return got


def reached(case):
    return {"A": _reached_a, "B": _reached_b, "C": _reached_c, "D": _reached_d, "E": _reached_e, "F": _reached_f}[case.family](case)


# ---------------------------------------------------------------- the census
REQUIRED = (
    ["A.%s.r%d" % (s, r) for s in ("narrow0", "wide_last", "narrow32") for r in range(16)] + ["A.full_wide", "A.full_narrow"] +
    ["A.rows_lt8", "A.narrow_first_only", "A.narrow_second_one_row", "A.padding_row", "A.h64", "A.h65"] +
    ["A.%s.%s" % (s, t) for s in FUSED for t in ("narrow", "wide")] + ["A.rgb", "A.bgr", "A.plain"] +
    ["A.off%d" % r for r in range(16)] + ["A.pitch16", "A.pitch_odd"] +
    ["B.%s.%s" % (c, t) for c in ("aligned_ragged", "odd_pitch", "one_misaligned") for t in ("wide", "narrow")] +
    ["B.%s.%s" % (f, t) for f in ("rgb_planar", "bgr_planar") for t in ("fancy", "plain")] +
    ["C.aligned_ragged", "C.misaligned_base", "C.pitch_not8", "C.multi_unit", "C.chroma_ragged", "C.y_colour", "C.y_gray", "C.yuv420", "C.yuv422", "C.yuv444"] +
    ["D.%s.w%d" % (s, w) for s in ("411", "410") for w in (255, 256, 257)] + ["D.cmyk", "D.ycck"] +
    ["E.o%d" % o for o in range(1, 9)] + ["E.w%d" % w for w in (255, 256, 257)] + ["E.h%d" % h for h in (7, 8, 9)] +
    ["E.fmt." + f for f in ("rgb", "rgb_planar", "y")] + ["E.o%d.%s" % (o, f) for o in range(1, 9) for f in ("rgb", "rgb_planar", "y")] +
    ["E.region." + k for k in ("rgb", "bgr", "rgb_planar", "plain", "gray")] +
    ["F.a16_tail", "F.a16_tail_ragged", "F.a4_ragged", "F.unaligned", "F.one_plane_misaligned", "F.direct", "F.upsampled", "F.region"] +
    ["F.fmt." + f for f in ("rgb", "bgr", "rgb_planar", "y")] + ["F.w%d" % w for w in (65, 33, 17, 25, 32, 40, 1, 4)] +
    ["F.denom%d" % d for d in (2, 4, 8)] + ["F.h7", "F.h8", "F.h9"])


def _padded(row_bytes, k):
    """a pitch with at least 16 guard bytes behind the row: a multiple of 16 for even k, odd for odd k"""
    if k % 2 == 0:
        return -(-(row_bytes + 16) // 16) * 16
    p = row_bytes + 17
    return p if p % 2 else p + 1


def _family_a():
    heights = (7, 8, 9, 25, 64, 65)
    widths = list(range(113, 129)) + list(range(241, 257)) + list(range(257, 273)) + [384]
    cases = []
    for i, w in enumerate(widths):
        sub, h = FUSED[i % 5], heights[i % 6]
        where = "narrow0" if w <= 128 else "wide_last" if w <= 256 else "narrow32" if w <= 272 else None
        res = (w - (256 if where == "narrow32" else 0)) * 3 % 16
        seams = ["A.%s.r%d" % (where, res)] if where else ["A.full_wide", "A.full_narrow"]
        seams.append("A.%s.%s" % (sub, "wide" if where == "wide_last" else "narrow"))
        if w == 256:
            seams.append("A.full_wide")
        if h == 7 and where == "wide_last":
            seams.append("A.rows_lt8")
        if h in (7, 8) and where != "wide_last":
            seams.append("A.narrow_first_only")
        if h in (9, 25, 65) and where != "wide_last":
            seams.append("A.narrow_second_one_row" if h != 65 else "A.narrow_first_only")
        if sub == "420" and (h + 7) // 8 % 2:
            seams.append("A.padding_row")
        if h in (64, 65):
            seams.append("A.h%d" % h)
        for k, (mode, fmt, fancy) in enumerate((("rgb", "rgb", True), ("bgr", "bgr", True), ("plain", "rgb", False))):
            n = 3 * i + k
            pitch = _padded(w * 3, n)
            extra = ["A." + mode, "A.off%d" % (n % 16), "A.pitch16" if pitch % 16 == 0 else "A.pitch_odd"]
            cases.append(Case("A.%dx%d.%s.%s" % (w, h, sub, mode), "A", tuple(seams + extra), ("synth", w, h, sub), fmt, fancy,
                              dict(pitch=pitch, residue=n % 16 + 16 * (n % 5)), None, 1, 1))
    return cases


def _family_b():
    cases = []
    n = 0
    for w, shape in ((250, "wide"), (117, "narrow")):
        for fmt, fancy in (("rgb_planar", True), ("bgr_planar", True), ("rgb_planar", False), ("bgr_planar", False)):
            for cls in ("aligned_ragged", "odd_pitch", "one_misaligned"):
                sub, h = ("420", "444", "422", "440")[n % 4], (19, 9, 17)[n % 3]
                extent = lambda pitch: (h - 1) * pitch + w
                if cls == "aligned_ragged":
                    pitch = -(-(w + 16) // 8) * 8
                    place = dict(pitch=pitch, residue=8 * (n % 4), plane_stride=-(-(extent(pitch) + 128) // 8) * 8)
                elif cls == "odd_pitch":
                    pitch = _padded(w, 1)
                    place = dict(pitch=pitch, residue=8 * (n % 4), plane_stride=-(-(extent(pitch) + 128) // 8) * 8)
                else:  # plane 1 alone is misaligned: the stride is 4 modulo 8, twice the stride 0
                    pitch = -(-(w + 16) // 8) * 8
                    place = dict(pitch=pitch, residue=8 * (n % 4), plane_stride=-(-(extent(pitch) + 128) // 8) * 8 + 4)
                seams = ("B.%s.%s" % (cls, shape), "B.%s.%s" % (fmt, "fancy" if fancy else "plain"))
                cases.append(Case("B.%dx%d.%s.%s.%s.%s" % (w, h, sub, fmt, "fancy" if fancy else "plain", cls), "B", seams, ("synth", w, h, sub), fmt,
                                  fancy, place, None, 1, 1))
                n += 1
    return cases


def _family_c():
    cases = []

    def y(name, source, seams, pitch, residue):
        cases.append(Case("C.y." + name, "C", tuple(seams), source, "y", True, dict(pitch=pitch, residue=residue), None, 1, 1))

    def yuv(name, source, seams, planes):
        cases.append(Case("C.yuv." + name, "C", tuple(seams), source, "yuv_planar", True, dict(planes=planes), None, 1, 1))

    y("colour_aligned", ("synth", 50, 37, "420"), ["C.y_colour", "C.aligned_ragged"], 72, 8)
    y("colour_misaligned", ("synth", 50, 37, "422"), ["C.y_colour", "C.misaligned_base"], 72, 3)
    y("colour_pitch", ("synth", 50, 37, "444"), ["C.y_colour", "C.pitch_not8"], 67, 16)
    y("gray_aligned", ("synth", 45, 21, "gray"), ["C.y_gray", "C.aligned_ragged"], 64, 0)
    y("gray_misaligned", ("synth", 45, 21, "gray"), ["C.y_gray", "C.misaligned_base"], 64, 5)
    y("gray_pitch", ("synth", 45, 21, "gray"), ["C.y_gray", "C.pitch_not8"], 61, 8)
    y("multi_unit", ("synth", 133, 70, "444"), ["C.y_colour", "C.multi_unit", "C.aligned_ragged"], 152, 0)   # 17 x 9 blocks
    y("multi_unit_whole", ("synth", 136, 72, "gray"), ["C.y_gray", "C.multi_unit"], 152, 8)
    # 50 x 37 at 4:2:0: chroma planes 25 x 19 (ragged on their own), luma 50 wide; 4:2:2: 25 x 37; 4:4:4: all 50 wide
    yuv("420_aligned", ("synth", 50, 37, "420"), ["C.yuv420", "C.aligned_ragged", "C.chroma_ragged"], [(72, 0), (48, 8), (48, 16)])
    yuv("420_mixed", ("synth", 50, 37, "420"), ["C.yuv420", "C.misaligned_base", "C.pitch_not8", "C.chroma_ragged"], [(72, 1), (45, 8), (48, 0)])
    yuv("422_mixed", ("synth", 50, 37, "422"), ["C.yuv422", "C.aligned_ragged", "C.misaligned_base", "C.pitch_not8"], [(67, 0), (48, 4), (48, 8)])
    yuv("444_mixed", ("synth", 50, 37, "444"), ["C.yuv444", "C.aligned_ragged", "C.misaligned_base", "C.pitch_not8"], [(72, 8), (72, 7), (69, 0)])
    yuv("420_multi_unit", ("synth", 270, 70, "420"), ["C.yuv420", "C.multi_unit", "C.aligned_ragged", "C.chroma_ragged"], [(288, 0), (152, 8), (157, 0)])
    return cases


def _family_d():
    cases = []
    n = 0
    for sub in ("411", "410"):
        for w in (255, 256, 257):
            cases.append(Case("D.%s.w%d" % (sub, w), "D", ("D.%s.w%d" % (sub, w),), ("synth", w, 19 + n, sub), "rgb", True,
                              dict(pitch=_padded(w * 3, 1), residue=n * 5 + 1), None, 1, 1))
            n += 1
    cases.append(Case("D.cmyk", "D", ("D.cmyk",), ("golden", "cmyk", "k50x37_s211_base_adobe0"), "rgb", True, dict(pitch=_padded(150, 1), residue=7), None, 1, 1))
    cases.append(Case("D.ycck", "D", ("D.ycck",), ("golden", "cmyk", "k50x37_s211_base_adobe2"), "rgb", True, dict(pitch=_padded(150, 0), residue=2), None, 1, 1))
    return cases


REGION_PICTURE = (400, 80)
# x0 >= 256: first_col = 32; the right edge leaves 1..16 block columns behind the last whole tile and stops short of the picture's edge;
# y0 in 32..63: first_row = 4, so a narrow tile (which spans 8 block rows) starts in the middle of a narrow tile of the whole picture
REGIONS = ((260, 37, 371, 75, 1), (257, 33, 264, 41, 6), (300, 63, 383, 80, 3))


def _family_e():
    cases = []
    n = 0
    sizes = ((255, 7), (256, 8), (257, 9))
    for o in range(1, 9):
        for k, fmt in enumerate(("rgb", "rgb_planar", "y")):
            for j in range(3):
                ow, oh = sizes[j][0], sizes[(j + o + k) % 3][1]
                rw, rh = (ow, oh) if o < 5 else (oh, ow)
                # a picture a little larger than the region, stored lying or standing as the orientation needs it
                source = ("synth", rw + 9, rh + 7, ("420", "444", "422")[n % 3])
                roi = (5, 3, 5 + rw, 3 + rh)
                bpp = 3 if fmt == "rgb" else 1
                place = dict(pitch=_padded(ow * bpp, n), residue=(n * 7) % 32)
                if fmt == "rgb_planar":
                    place["plane_stride"] = -(-((oh - 1) * place["pitch"] + ow + 128) // 4) * 4 + (n % 4)
                seams = ("E.o%d" % o, "E.w%d" % ow, "E.h%d" % oh, "E.fmt." + fmt, "E.o%d.%s" % (o, fmt))
                cases.append(Case("E.o%d.%dx%d.%s" % (o, ow, oh, fmt), "E", seams, source, fmt, True, place, roi, o, 1))
                n += 1
    w, h = REGION_PICTURE
    for x0, y0, x1, y1, o in REGIONS:
        for kind, fmt, fancy, sub in (("rgb", "rgb", True, "420"), ("bgr", "bgr", True, "422"), ("rgb_planar", "rgb_planar", True, "444"),
                                      ("plain", "rgb", False, "420"), ("gray", "rgb", True, "gray")):
            rw, rh = x1 - x0, y1 - y0
            ow, oh = (rw, rh) if o < 5 else (rh, rw)
            bpp = 1 if fmt == "rgb_planar" else 3
            place = dict(pitch=_padded(ow * bpp, n), residue=(n * 3) % 16)
            if fmt == "rgb_planar":
                place["plane_stride"] = (oh - 1) * place["pitch"] + ow + 128 + n % 8
            seams = ("E.region." + kind, "E.o%d" % o)
            cases.append(Case("E.region.%d_%d_%d_%d.o%d.%s" % (x0, y0, x1, y1, o, kind), "E", seams, ("synth", w, h, sub), fmt, fancy, place,
                              (x0, y0, x1, y1), o, 1))
            n += 1
    return cases


def _family_f():
    cases = []

    def add(name, denom, fmt, seams, pitch_pad, residue, stride_mod=0, roi=None, orientation=1):
        c = Case("F.%s.d%d.%s.p%d.r%d%s" % (name, denom, fmt, pitch_pad, residue, ".s%d" % stride_mod if stride_mod else ""), "F", tuple(seams),
                 ("scaled", name), fmt, True, {}, roi, orientation, denom)
        shape = output_shape(c)
        oh, ow = (shape[1], shape[2]) if fmt.endswith("_planar") else (shape[0], shape[1])
        row = ow * (3 if fmt in ("rgb", "bgr") else 1)
        place = dict(pitch=row + pitch_pad, residue=residue)
        if fmt.endswith("_planar"):
            place["plane_stride"] = -(-((oh - 1) * place["pitch"] + ow + 128) // 16) * 16 + stride_mod
        cases.append(c._replace(place=place))

    def pad16(name, denom, fmt):
        """the least pad >= 16 that makes the pitch a multiple of 16"""
        sc = S.by_name(name)["scales"][str(denom)]
        row = sc["width"] * (3 if fmt in ("rgb", "bgr") else 1)
        return -(-(row + 16) // 16) * 16 - row

    # aligned16 with W % 16 != 0: the wide loop runs AND the tail behind it has work; 65, 33, 17 end in a group of one pixel
    for name in ("h130x70_444_opt_q75", "h130x70_420_opt_q75", "h130x70_gray_opt_q75"):
        for denom, w in ((2, 65), (4, 33), (8, 17)):
            for fmt in ("rgb", "rgb_planar") if "gray" not in name else ("rgb", "y"):
                seams = ["F.a16_tail", "F.a16_tail_ragged", "F.direct", "F.w%d" % w, "F.denom%d" % denom, "F.fmt." + fmt] + (["F.h9"] if denom == 8 else [])
                add(name, denom, fmt, seams, pad16(name, denom, fmt), 16 * denom)
    add("s50x37_444_base_q90", 2, "bgr", ["F.a16_tail", "F.a16_tail_ragged", "F.w25", "F.fmt.bgr"], pad16("s50x37_444_base_q90", 2, "bgr"), 0)
    add("h320x200_420_opt_q75", 8, "rgb", ["F.a16_tail", "F.w40", "F.denom8"], pad16("h320x200_420_opt_q75", 8, "rgb"), 32)   # 40 = 2 x 16 + 2 x 4
    add("s64x48_444_base_q90", 2, "rgb", ["F.w32", "F.direct"], pad16("s64x48_444_base_q90", 2, "rgb"), 0)                   # whole wide groups only
    add("s64x48_420_base_q90", 8, "rgb", ["F.h6"], 20, 4)     # 8 x 6: one workgroup, two of its rows idle
    # 4-byte aligned only, with a ragged last group
    add("h130x70_444_opt_q75", 2, "rgb", ["F.a4_ragged", "F.w65"], 17, 4)        # 195 + 17 = 212
    add("s50x37_420_base_q90", 2, "rgb_planar", ["F.a4_ragged", "F.w25"], 19, 8, stride_mod=4)   # 25 + 19 = 44
    add("s33x65_gray_base_q90", 2, "y", ["F.a4_ragged", "F.w17", "F.fmt.y"], 19, 12)             # 17 + 19 = 36
    # unaligned: odd pitch or odd base
    add("h130x70_420_opt_q75", 4, "bgr", ["F.unaligned", "F.w33", "F.fmt.bgr"], 18, 3)
    add("h130x70_gray_opt_q75", 2, "y", ["F.unaligned", "F.w65"], 16, 0)          # pitch 81
    add("s64x48_444_base_q90", 2, "rgb_planar", ["F.unaligned", "F.w32"], 17, 16)
    # one plane misaligned: a plane stride of 2 modulo 4 puts plane 1 at +2 and plane 2 at +4
    add("h130x70_444_opt_q75", 4, "rgb_planar", ["F.one_plane_misaligned", "F.w33"], pad16("h130x70_444_opt_q75", 4, "rgb_planar"), 0, stride_mod=2)
    # pictures that are not `direct`: 4:2:2 and 4:4:0 are upsampled per pixel at a scale
    add("s50x37_422_base_q90", 2, "rgb", ["F.upsampled", "F.w25"], pad16("s50x37_422_base_q90", 2, "rgb"), 0)
    add("o50x37_440_base_q90", 2, "rgb", ["F.upsampled", "F.w25", "F.a4_ragged"], 17, 4)   # 75 + 17 = 92
    add("s33x65_422_base_q90", 2, "bgr", ["F.upsampled", "F.w17", "F.unaligned"], 16, 1)
    add("t33x17_440_base", 2, "rgb_planar", ["F.upsampled", "F.w17", "F.h9"], 16 + 15, 0)  # 17 x 9
    # y of colour files (the scaled/ set records the library's own grayscale decode), 1 x 1 and 7 x 5
    add("t33x17_420_base", 2, "y", ["F.fmt.y", "F.w17", "F.h9", "F.a16_tail"], 31, 16)      # 17 + 31 = 48
    add("t7x5_444_base", 2, "rgb", ["F.w4"], 20, 0)
    add("t7x5_422_prog", 2, "y", ["F.w4", "F.unaligned"], 17, 5)
    add("t1x1_420_base", 2, "rgb", ["F.w1"], 29, 0)
    add("t1x1_gray_base", 8, "y", ["F.w1"], 16, 3)
    add("t17x9_444_base", 2, "rgb", ["F.direct"], 16, 0)                                      # 9 x 5
    # heights around the 8 rows of a workgroup, by a region of a scaled picture, turned: 35 rows cut to 7 and to 8
    add("h130x70_420_opt_q75", 2, "rgb", ["F.region", "F.h7"], 17, 5, roi=(3, 9, 60, 16), orientation=3)
    add("h130x70_444_opt_q75", 2, "rgb_planar", ["F.region", "F.h8"], 16, 8, roi=(1, 20, 65, 28), orientation=4)
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    out = _family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def family(letter):
    return [c for c in cases() if c.family == letter]


def neighbours(letter, fmt, fancy, per_family=2):
    """a few cases of the OTHER families that can share a decode call (same format, same upsampling) with a batch of family `letter`"""
    out = []
    for other in "ABCDEF":
        if other != letter:
            out += [c for c in family(other) if c.fmt == fmt and c.fancy == fancy][:per_family]
    return out


def groups(case_list):
    """cases by what one decode call fixes for its whole batch: {(fmt, fancy): [cases]}, in order of first appearance"""
    g = collections.OrderedDict()
    for c in case_list:
        g.setdefault((c.fmt, c.fancy), []).append(c)
    return g


# ---------------------------------------------------------------- expectations
def h1v2_fancy(plane, height):
    """jdsample.c h1v2_fancy_upsample: 3/4 of the nearer row, 1/4 of the further, bias 1 for the upper and 2 for the lower output row"""
    p = plane.astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]])
    down = np.concatenate([p[1:], p[-1:]])
    out = np.zeros((2 * p.shape[0], p.shape[1]), dtype=np.int64)
    out[0::2] = (3 * p + up + 1) >> 2
    out[1::2] = (3 * p + down + 2) >> 2
    return out[:height]


def pixels_from_planes(planes, i, fancy=True, bgr=False):
    """libjpeg-turbo's upsampling and colour conversion on component planes (cropped to the components' sizes: oracle.decode_planes for
    the default IDCT, ifast_idct.planes for the fast one) -> H x W x 3.  tests/test_pixel_seams.py pins it to oracle.decode on the default
    IDCT's planes for every sampling of family A; the fast-IDCT run of family A takes its expectations from it."""
    W, H = i["width"], i["height"]
    if i["ncomp"] == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    full = []
    for c, pl in enumerate(planes):
        fx, fy = i["hmax"] // i["h"][c], i["vmax"] // i["v"][c]
        if fancy and (fx, fy) == (1, 2):
            full.append(h1v2_fancy(pl, H)[:, :W])
        elif fancy:
            full.append(ifast_idct.upsample(pl, fx, fy, W, H))
        else:
            full.append(np.repeat(np.repeat(pl.astype(np.int64), fy, axis=0), fx, axis=1)[:H, :W])
    y, cb, cr = full
    r = np.clip(y + ((cr * 91881 + 32768 - 128 * 91881) >> 16), 0, 255)
    g = np.clip(y + ((cb * -22554 + cr * -46802 + 32768 + 128 * 22554 + 128 * 46802) >> 16), 0, 255)
    b = np.clip(y + ((cb * 116130 + 32768 - 128 * 116130) >> 16), 0, 255)
    return np.stack([b, g, r] if bgr else [r, g, b], axis=2).astype(np.uint8)


def _cmyk_rgb(cmyk, adobe):
    """extensions/libjpeg_turbo/jpeg_mem.cpp:303-313 (as tests/test_cmyk.py)"""
    c, m, y, k = [cmyk[:, :, i].astype(np.int32) for i in range(4)]
    if adobe:
        return np.stack([(k * c) // 255, (k * m) // 255, (k * y) // 255], axis=2).astype(np.uint8)
    return np.stack([(255 - k) * (255 - c) // 255, (255 - k) * (255 - m) // 255, (255 - k) * (255 - y) // 255], axis=2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _full(source, kind, fancy, fast_idct):
    """the whole picture at full size: kind rgb / bgr (H x W x 3), y (H x W) or yuv (planes)"""
    j = jpeg(source)
    if source[:2] == ("golden", "cmyk"):
        with open(os.path.join(GOLDEN, "manifest_cmyk.json")) as f:
            entry = next(e for e in json.load(f)["cmyk"] if e["name"] == source[2])
        assert kind == "rgb" and not fast_idct
        return _cmyk_rgb(oracle.decode_cmyk(j), entry["kind"] != "plain")
    if fast_idct:
        assert kind in ("rgb", "bgr")
        return pixels_from_planes(ifast_idct.planes(j), info(source), fancy, kind == "bgr")
    if kind == "yuv":
        return oracle.decode_planes(j)[:3]
    return oracle.decode(j, {"rgb": oracle.FMT_RGB, "bgr": oracle.FMT_BGR, "y": oracle.FMT_GRAY}[kind], fancy=fancy)


def expected(case, fast_idct=False, scaled_full=None):
    """What the case's output must hold: an array (a list of planes for yuv_planar), or a Hashed for a scaled picture.
    scaled_full: for a region of a scaled picture, the whole scaled picture as H x W x 3 RGB (the caller decodes it tightly and
    checks it against the manifest's hash: the goldens pin hashes, not pixels)."""
    if case.scale != 1:
        entry = S.by_name(case.source[1])
        if has_transform(case):
            x0, y0, x1, y1 = case.roi
            want = upright(scaled_full[y0:y1, x0:x1], case.orientation)
            if case.fmt.startswith("bgr"):
                want = want[:, :, ::-1]
            return np.ascontiguousarray(want.transpose(2, 0, 1) if case.fmt.endswith("_planar") else want)
        sc = entry["scales"][str(case.scale)]
        if case.fmt == "y" and "y_sha256" in sc:
            return Hashed(sc["y_sha256"], lambda a: a)
        status, sha = S.expected(entry, case.scale)
        assert status == S.SUCCESS
        canon = {"rgb": lambda a: a, "bgr": lambda a: a[:, :, ::-1], "rgb_planar": lambda a: a.transpose(1, 2, 0),
                 "bgr_planar": lambda a: a[::-1].transpose(1, 2, 0),
                 # a gray file: the library's RGB is the luma three times
                 "y": lambda a: np.repeat(a[:, :, None], 3, axis=2)}[case.fmt]
        assert case.fmt != "y" or sub_of(case.source) == "gray"
        return Hashed(sha, canon)
    kind = "yuv" if case.fmt == "yuv_planar" else "y" if case.fmt == "y" else "bgr" if case.fmt.startswith("bgr") else "rgb"
    full = _full(case.source, kind, case.fancy, fast_idct)
    if kind == "yuv":
        return full
    if has_transform(case):
        x0, y0, x1, y1 = case.roi or (0, 0) + picture_size(case)
        full = upright(full[y0:y1, x0:x1], case.orientation)
    return np.ascontiguousarray(full.transpose(2, 0, 1) if case.fmt.endswith("_planar") else full)
