"""Drop chroma -> crop -> turn of a lossless transcode, modelled in numpy from the oracle's coefficients -- no call of the library's
transcode: which requests succeed (the eligibility rules of include/hipjpeg.h, with the chroma-only ones waived for GRAYSCALE), and the
picture that must come out: size, luma factors, per component the blocks source[c][oy:oy+rh, ox:ox+rw] turned by
transform_model.turn_blocks, tables, block count.  Also a collector of the APPn / COM segments a COPY_MARKERS output must carry and the
EXIF orientation patch, both written here from the JPEG and TIFF layouts alone."""
import struct

import numpy as np

import oracle
from helpers import transcode_cases as T
from helpers import transform_model as M
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

INVALID_ARGUMENT = 1
JFIF_APP0 = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"  # the writer's own


def gray_eligible(data, qts):
    """What remains of the header rules under GRAYSCALE for a three-component source: frame type, colour model YCbCr, a luma component at
    the frame's full resolution, luma quantizers in 1..255."""
    try:
        info = lowlevel.get_image_info(data)
    except N.HipJpegError:
        return False
    if info["sof_marker"] not in (0xC0, 0xC1, 0xC2) or info["num_components"] != 3 or info["color_model"] != 1:
        return False
    if info["h"][0] != max(info["h"][:3]) or info["v"][0] != max(info["v"][:3]):
        return False
    return 1 <= int(qts[0].min()) and int(qts[0].max()) <= 255


def mcu_size(data, grayscale=False):
    """(width, height) of the iMCU of the picture the crop applies to"""
    info = oracle.read_info(data)
    hs, vs = (1, 1) if grayscale else M.luma_factors(info)
    return 8 * hs, 8 * vs


def recipe_region(data, grayscale=False):
    """The test recipe: origin one iMCU in from the left and top, x1 = min(W, x0 + 2 mcu_w + 5), y1 = min(H, y0 + mcu_h + 11); None when
    the picture is too small for it (W < x0 + 9 or H < y0 + 9)."""
    info = oracle.read_info(data)
    mw, mh = mcu_size(data, grayscale)
    w, h = info["width"], info["height"]
    if w < mw + 9 or h < mh + 9:
        return None
    return mw, mh, min(w, mw + 2 * mw + 5), min(h, mh + mh + 11)


def expected(data, orientation=1, trim=False, region=None, grayscale=False, expand=False):
    """-> dict(status=...) and for SUCCESS: width, height, hs, vs, coefs (per component, over the real area), qts, blocks, origin"""
    info = oracle.read_info(data)
    coefs, qts = oracle.decode_coefficients(data)
    gray = grayscale and info["ncomp"] == 3
    if not (gray_eligible(data, qts) if gray else T.header_eligible(data)):
        return dict(status=T.UNSUPPORTED)
    ncomp = 1 if gray else info["ncomp"]
    hs, vs = (1, 1) if ncomp == 1 else (info["h"][0], info["v"][0])
    x0, y0, x1, y1 = 0, 0, info["width"], info["height"]
    if region is not None and any(region):
        x0, y0, x1, y1 = region
        if not (0 <= x0 < x1 <= info["width"] and 0 <= y0 < y1 <= info["height"]):
            return dict(status=INVALID_ARGUMENT)
        if x0 % (8 * hs) or y0 % (8 * vs):
            if not expand:
                return dict(status=T.UNSUPPORTED)
            x0, y0 = x0 - x0 % (8 * hs), y0 - y0 % (8 * vs)
    if orientation in M.TRANSPOSES and hs == 4:
        return dict(status=T.UNSUPPORTED)
    kept = M.kept_size(dict(width=x1 - x0, height=y1 - y0, ncomp=ncomp, h=[hs], v=[vs]), orientation, trim)
    if kept is None:
        return dict(status=T.UNSUPPORTED)
    w, h = kept
    out, origin = [], []
    for c, (rh, rw) in enumerate(M.real_area(w, h, hs, vs, ncomp)):
        oy, ox = (y0 // 8, x0 // 8) if c == 0 else (y0 // (8 * vs), x0 // (8 * hs))
        blk = coefs[c][oy:oy + rh, ox:ox + rw]
        assert blk.shape[:2] == (rh, rw)  # the source's grid holds them
        wide = blk.astype(np.int32)
        if wide[:, :, 0].min() < -1024 or wide[:, :, 0].max() > 1023 or wide[:, :, 1:].min() < -1023 or wide[:, :, 1:].max() > 1023:
            return dict(status=T.UNSUPPORTED)
        out.append(M.turn_blocks(blk, orientation))
        origin.append((ox, oy))
    qts = list(qts[:ncomp])
    if orientation in M.TRANSPOSES:
        w, h, hs, vs = h, w, vs, hs
        qts = [q.reshape(8, 8).T.reshape(64).copy() for q in qts]
    return dict(status=T.SUCCESS, width=w, height=h, hs=hs, vs=vs, coefs=out, qts=qts, blocks=sum(c.shape[0] * c.shape[1] for c in out),
                origin=origin, region=(x0, y0, x1, y1))


# ---------------------------------------------------------------------------------------------- marker segments
def header_segments(jpeg):
    """[(marker byte, whole segment: FF, marker, length, payload)] between SOI and the first SOS, fill bytes passed over"""
    b, out, pos = bytes(jpeg), [], 2
    while True:
        while pos < len(b) and b[pos] != 0xFF:
            pos += 1
        while pos < len(b) and b[pos] == 0xFF:
            pos += 1
        if pos >= len(b) or b[pos] in (0xDA, 0xD9):
            return out
        m = b[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if pos + 2 > len(b):
            return out
        length = struct.unpack(">H", b[pos:pos + 2])[0]
        if length < 2 or pos + length > len(b):
            return out
        out.append((m, b"\xff" + bytes([m]) + b[pos:pos + length]))
        pos += length


def _is_app_or_com(m):
    return 0xE0 <= m <= 0xEF or m == 0xFE


def _exif_value_offset(segment):
    """(offset of the orientation entry's two value bytes inside the whole segment, struct byte-order character) or None"""
    body = segment[4:]
    if body[:6] != b"Exif\0\0":
        return None
    tiff = body[6:]
    e = {b"II": "<", b"MM": ">"}.get(tiff[:2])
    if e is None or len(tiff) < 8 or struct.unpack(e + "H", tiff[2:4])[0] != 42:
        return None
    ifd = struct.unpack(e + "I", tiff[4:8])[0]
    if ifd + 2 > len(tiff):
        return None
    for i in range(struct.unpack(e + "H", tiff[ifd:ifd + 2])[0]):
        at = ifd + 2 + 12 * i
        if at + 12 > len(tiff):
            return None
        if struct.unpack(e + "H", tiff[at:at + 2])[0] == 0x0112:
            return 4 + 6 + at + 8, e
    return None


def copied_segments(source, turned):
    """The segments a COPY_MARKERS output carries behind its own APP0: every APPn / COM of the source in order, the JFIF APP0 left out,
    and -- when the picture is turned -- the orientation of the first APP1/Exif segment set to 1."""
    out, seen_exif = [], False
    for m, seg in header_segments(source):
        if not _is_app_or_com(m) or (m == 0xE0 and seg[4:9] == b"JFIF\0"):
            continue
        if m == 0xE1 and seg[4:10] == b"Exif\0\0" and not seen_exif:
            seen_exif = True
            found = _exif_value_offset(seg)
            if turned and found is not None:
                at, e = found
                seg = seg[:at] + struct.pack(e + "H", 1) + seg[at + 2:]
        out.append(seg)
    return out


def app_and_com_segments(jpeg):
    return [seg for m, seg in header_segments(jpeg) if _is_app_or_com(m)]
