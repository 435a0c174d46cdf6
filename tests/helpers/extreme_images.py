"""Deterministic RGB test pictures that sit on the edges of the 8-bit range: saturated flats, 1-pixel and 8-pixel checkerboards, the
colour-conversion extremes next to each other, {0,255} random and full-range noise.  nvimagecodec_amd.synth.synth_image squeezes its
pixels into 24..232; the encode device stage's arithmetic (chroma packing without a mask, the 16-bit FDCT column pass, the multiply-high
quantizer) is tight only at 0 and 255.  Random patterns are drawn from synth._hash_u32 (a counter hash), so the bytes do not depend on a
numpy generator's stream."""
import numpy as np

from nvimagecodec_amd.synth import _hash_u32

PATTERNS = ("black", "white", "blue", "checker1", "redblue", "stripes4", "random01", "noise", "block_checker", "primaries", "boundary")

_PRIMARIES = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)],
                      dtype=np.uint8)


def _hash_bytes(n, seed, salt):
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) + (np.uint64(seed) + np.uint64(salt)) * np.uint64(0x100000001B3)
        return _hash_u32(ctr)


_KCC = (128 << 16) + 32767  # jccolor.c CBCR_OFFSET + ONE_HALF - 1
_boundary = None


def boundary_colours():
    """Every colour that sits on a rounding boundary of jccolor.c's fixed-point conversion: the low 16 bits of the sum that is shifted
    down for Y, Cb or Cr are 0x0000 or 0xFFFF, so one unit more or less in a weight or in a rounding constant moves the sample.
    -> uint8 [n, 3], in a fixed order"""
    global _boundary
    if _boundary is None:
        a, b = [v.ravel().astype(np.int64) for v in np.mgrid[0:256, 0:256]]
        found = []
        for odd in (0, 1):  # 32768 * x: only the parity of x reaches the low 16 bits
            others = np.array([odd, 128 + odd, 254 + odd], dtype=np.int64)
            low = (-11059 * a - 21709 * b + 32768 * odd + _KCC) & 0xFFFF  # Cb: a = R, b = G, the free channel is B
            k = np.flatnonzero((low == 0) | (low == 0xFFFF))
            found += [np.stack([a[k], b[k], np.full(k.size, o)], axis=1) for o in others]
            low = (32768 * odd - 27439 * a - 5329 * b + _KCC) & 0xFFFF  # Cr: a = G, b = B, the free channel is R
            k = np.flatnonzero((low == 0) | (low == 0xFFFF))
            found += [np.stack([np.full(k.size, o), a[k], b[k]], axis=1) for o in others]
        inv = pow(7471, -1, 65536)
        for target in (0, 0xFFFF):  # Y: a = R, b = G; the B that completes the sum, where there is one
            blue = ((target - (19595 * a + 38470 * b + 32768)) * inv) & 0xFFFF
            k = np.flatnonzero(blue < 256)
            found.append(np.stack([a[k], b[k], blue[k]], axis=1))
        _boundary = np.concatenate(found).astype(np.uint8)
    return _boundary


def extreme_image(pattern, width, height, seed=0):
    """-> uint8 array [height, width, 3] (RGB)"""
    y, x = np.mgrid[0:height, 0:width]
    img = np.zeros((height, width, 3), dtype=np.uint8)
    if pattern == "black":
        pass
    elif pattern == "white":
        img[:] = 255
    elif pattern == "blue":
        img[:, :, 2] = 255
    elif pattern == "checker1":  # 1-pixel black / white checkerboard
        img[:] = (((x + y) & 1) * 255).astype(np.uint8)[:, :, None]
    elif pattern == "redblue":  # 1-pixel red / blue checkerboard: Cb and Cr swing end to end, chroma downsampling averages opposites
        odd = ((x + y) & 1).astype(bool)
        img[~odd] = (255, 0, 0)
        img[odd] = (0, 0, 255)
    elif pattern == "stripes4":  # vertical 4-pixel black / white stripes: an edge in the middle of every block
        img[:] = (((x >> 2) & 1) * 255).astype(np.uint8)[:, :, None]
    elif pattern == "random01":  # every channel of every pixel 0 or 255
        img = (((_hash_bytes(width * height * 3, seed, 11) >> np.uint32(13)) & np.uint32(1)) * np.uint32(255)).astype(np.uint8)
        img = img.reshape(height, width, 3)
    elif pattern == "noise":  # full-range noise
        img = (_hash_bytes(width * height * 3, seed, 12) >> np.uint32(24)).astype(np.uint8).reshape(height, width, 3)
    elif pattern == "block_checker":  # 8x8 blocks alternating 0 and 255: DC differences of category 11 at quality 100
        img[:] = ((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)[:, :, None]
    elif pattern == "primaries":  # 8-pixel bars, one row of blocks lower the bars move on by one: every extreme next to its opposite
        img = _PRIMARIES[((x >> 3) + (y >> 3)) & 7]
    elif pattern == "boundary":  # colours on the rounding boundaries of the colour conversion, drawn at random
        colours = boundary_colours()
        img = colours[_hash_bytes(width * height, seed, 13) % np.uint32(len(colours))].reshape(height, width, 3)
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(img)


_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
           49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def dqt_tables(jpeg):
    """The DQT segments in front of a file's first scan -> {table id: list of 64 in natural (row-major) order}"""
    b = bytes(jpeg)
    tables = {}
    i = 2
    while b[i + 1] != 0xDA:
        assert b[i] == 0xFF
        length = (b[i + 2] << 8) | b[i + 3]
        if b[i + 1] == 0xDB:
            k = i + 4
            while k < i + 2 + length:
                precision, ident = b[k] >> 4, b[k] & 15
                k += 1
                nat = [0] * 64
                for z in range(64):
                    nat[_ZIGZAG[z]] = ((b[k] << 8) | b[k + 1]) if precision else b[k]
                    k += 2 if precision else 1
                tables[ident] = nat
        i += 2 + length
    return tables


def ycc(rgb):
    """jccolor.c rgb_ycc_convert, SCALEBITS 16"""
    r, g, b = [rgb[:, :, i].astype(np.int64) for i in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def extremes_reached(cases):
    """cases: (rgb, per-component coefficients of a 4:4:4 or gray encoding) -> largest |DC difference| in scan order, largest |AC|,
    and the set of Cb and of Cr samples of the pictures"""
    dc, ac, cbs, crs = 0, 0, set(), set()
    for rgb, coefs in cases:
        for c in coefs:
            flat = c[:, :, 0].astype(np.int64).ravel()  # one block per component and MCU: scan order is raster order
            dc = max(dc, int(np.abs(np.diff(np.concatenate([[0], flat]))).max()))
            ac = max(ac, int(np.abs(c[:, :, 1:].astype(np.int64)).max()))
        _, cb, cr = ycc(rgb)
        cbs |= set(np.unique(cb).tolist())
        crs |= set(np.unique(cr).tolist())
    return dc, ac, cbs, crs
