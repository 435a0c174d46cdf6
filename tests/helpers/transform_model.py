"""The lossless turns of a transcode (hipjpegTranscodeParams_t::orientation), modelled in numpy from the DCT identities alone -- no call
of the library: which sources may be turned, and the picture that must come out (size, luma factors, coefficients over the real block
area, quantization tables).  Also an EXIF orientation reader of its own and the bytes of an APP1/Exif segment to try it on.

With u the horizontal and v the vertical frequency of natural position v * 8 + u:
  horizontal mirror   block columns reversed, coefficients with odd u negated
  vertical mirror     block rows reversed, coefficients with odd v negated
  transpose           block (by, bx) -> (bx, by), coefficient (u, v) -> (v, u); luma factors, width and height swap, tables transposed
  6 = transpose then horizontal mirror, 8 = transpose then vertical mirror, 3 = both mirrors, 7 = transpose then both mirrors."""
import struct

import numpy as np

import oracle
from helpers import transcode_cases as T

MIRRORS_SOURCE_X = {2, 3, 7, 8}
MIRRORS_SOURCE_Y = {3, 4, 6, 7}
TRANSPOSES = {5, 6, 7, 8}


def _hmirror(c):
    sign = np.where(np.arange(64) % 2 == 1, -1, 1).astype(np.int16)  # odd u
    return c[:, ::-1] * sign


def _vmirror(c):
    sign = np.where((np.arange(64) // 8) % 2 == 1, -1, 1).astype(np.int16)  # odd v
    return c[::-1] * sign


def _transpose(c):
    rh, rw = c.shape[:2]
    return c.swapaxes(0, 1).reshape(rw, rh, 8, 8).swapaxes(2, 3).reshape(rw, rh, 64)


_STEPS = {1: (), 2: (_hmirror,), 3: (_hmirror, _vmirror), 4: (_vmirror,), 5: (_transpose,), 6: (_transpose, _hmirror),
          7: (_transpose, _hmirror, _vmirror), 8: (_transpose, _vmirror)}


def turn_blocks(c, orientation):
    """[rows, columns, 64] natural-order blocks of one component -> the blocks of the upright picture"""
    for step in _STEPS[orientation]:
        c = step(c)
    return np.ascontiguousarray(c)


def luma_factors(info):
    return (1, 1) if info["ncomp"] == 1 else (info["h"][0], info["v"][0])


def kept_size(info, orientation, trim):
    """(width, height) of the source that travels, or None where the iMCU rule refuses the turn"""
    hs, vs = luma_factors(info)
    w, h = info["width"], info["height"]
    if orientation in MIRRORS_SOURCE_X and w % (8 * hs):
        if not trim or w < 8 * hs:
            return None
        w -= w % (8 * hs)
    if orientation in MIRRORS_SOURCE_Y and h % (8 * vs):
        if not trim or h < 8 * vs:
            return None
        h -= h % (8 * vs)
    return w, h


def real_area(w, h, hs, vs, ncomp):
    """per component (rows, columns) of blocks that carry samples of a w x h picture"""
    out = [((h + 7) // 8, (w + 7) // 8)]
    for _ in range(1, ncomp):
        out.append((((h + vs - 1) // vs + 7) // 8, ((w + hs - 1) // hs + 7) // 8))
    return out


def expected(data, orientation, trim):
    """-> dict(status=...) and for SUCCESS: width, height, hs, vs, coefs (per component, over the real area), qts, blocks"""
    if not T.header_eligible(data):
        return dict(status=T.UNSUPPORTED)
    info = oracle.read_info(data)
    hs, vs = luma_factors(info)
    if orientation in TRANSPOSES and hs == 4:
        return dict(status=T.UNSUPPORTED)
    kept = kept_size(info, orientation, trim)
    if kept is None:
        return dict(status=T.UNSUPPORTED)
    w, h = kept
    coefs, qts = oracle.decode_coefficients(data)
    out = []
    for c, (rh, rw) in zip(coefs, real_area(w, h, hs, vs, info["ncomp"])):
        blk = c[:rh, :rw]
        wide = blk.astype(np.int32)
        if wide[:, :, 0].min() < -1024 or wide[:, :, 0].max() > 1023 or wide[:, :, 1:].min() < -1023 or wide[:, :, 1:].max() > 1023:
            return dict(status=T.UNSUPPORTED)
        out.append(turn_blocks(blk, orientation))
    if orientation in TRANSPOSES:
        w, h, hs, vs = h, w, vs, hs
        qts = [q.reshape(8, 8).T.reshape(64).copy() for q in qts]
    return dict(status=T.SUCCESS, width=w, height=h, hs=hs, vs=vs, coefs=out, qts=qts, blocks=sum(c.shape[0] * c.shape[1] for c in out))


def check_file(out, want):
    """the file `out` holds the picture `want` (of expected())"""
    info = oracle.read_info(out)
    assert (info["width"], info["height"]) == (want["width"], want["height"])
    assert luma_factors(info) == (want["hs"], want["vs"]) and info["ncomp"] == len(want["coefs"])
    coefs, qts = oracle.decode_coefficients(out)
    for got, c, qa, qb in zip(coefs, want["coefs"], qts, want["qts"]):
        assert np.array_equal(got[:c.shape[0], :c.shape[1]], c) and np.array_equal(qa, qb)


# ---------------------------------------------------------------------------------------------- EXIF
def exif_segment(value, little_endian, tag=0x0112):
    """APP1 marker segment with one IFD0 entry: the orientation tag (SHORT, count 1) holding `value`"""
    e = "<" if little_endian else ">"
    tiff = (b"II" if little_endian else b"MM") + struct.pack(e + "HI", 42, 8)
    tiff += struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", tag, 3, 1, value, 0) + struct.pack(e + "I", 0)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def with_segment(jpeg, segment):
    """the file with `segment` right behind SOI"""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + segment + jpeg[2:]


def read_exif_orientation(jpeg):
    """Tag 0x0112 of IFD0 of the first APP1/Exif segment before the first scan; 1 when missing or outside 1..8."""
    b = bytes(jpeg)
    pos = 2
    while pos + 4 <= len(b) and b[pos] == 0xFF and b[pos + 1] not in (0xDA, 0xD9):
        length = struct.unpack(">H", b[pos + 2:pos + 4])[0]
        body = b[pos + 4:pos + 2 + length]
        if b[pos + 1] == 0xE1 and body[:6] == b"Exif\0\0":
            tiff = body[6:]
            e = {b"II": "<", b"MM": ">"}.get(tiff[:2])
            if e is None or len(tiff) < 8 or struct.unpack(e + "H", tiff[2:4])[0] != 42:
                return 1
            ifd = struct.unpack(e + "I", tiff[4:8])[0]
            if ifd + 2 > len(tiff):
                return 1
            for i in range(struct.unpack(e + "H", tiff[ifd:ifd + 2])[0]):
                entry = tiff[ifd + 2 + 12 * i:ifd + 14 + 12 * i]
                if len(entry) < 12:
                    break
                if struct.unpack(e + "H", entry[:2])[0] == 0x0112:
                    value = struct.unpack(e + "H", entry[8:10])[0]
                    return value if 1 <= value <= 8 else 1
            return 1
        pos += 2 + length
    return 1
