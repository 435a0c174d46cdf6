"""numpy restatement of libjpeg-turbo's fast integer IDCT (JDCT_IFAST), from dequantisation to 8-bit samples.

Two routines, both of the 8-bit library that the reference's CPU path links (extensions/libjpeg_turbo/jpeg_mem.cpp:177 selects
JDCT_FASTEST = JDCT_IFAST when the decoder's `fast_idct` option is set):

  * SIMD: jsimd_idct_ifast_sse2 (simd/x86_64/jidctfst-sse2.asm), what x86-64 runs by default and what the GPU kernels restate.
    Every value is an int16 lane: the dequantising product keeps its low 16 bits (pmullw), sums wrap (paddw/psubw), a constant
    multiply is the high half of a 16-bit product on an operand shifted left by 2 (psllw + pmulhw, constants << 6), the result is
    shifted right by 5 and saturated to int8 (psraw + packsswb) before the + 128.  The routine's "AC terms all zero" shortcut gives
    what the full column pass gives on such a block (every output is the dequantised DC), so it needs no statement of its own.
  * C: jidctfst.c as built in a SIMD-enabled library (JSIMD_FORCENONE=1): DCTELEM is a short there, so every assignment to a
    temporary wraps to 16 bits, while the workspace and the final sums are plain ints; a column or row whose AC terms are zero
    takes a shortcut on those ints, and the result is masked with RANGE_MASK (1023) instead of saturated.

Both take the multiplier table jddctmgr.c builds for JDCT_IFAST: (q * aanscales[k] + 2048) >> 12, stored as int16.
Input: oracle.decode_coefficients (natural order, int16 blocks [bh, bw, 64]); output: the component's plane, blocks_h*8 x blocks_w*8."""
import numpy as np

# jddctmgr.c aanscales[] (natural order): 16384 * s[row] * s[col], s[0] = 1, s[k] = cos(k pi / 16) * sqrt(2), rounded
AANSCALES = np.array([
    16384, 22725, 21407, 19266, 16384, 12873, 8867, 4520,
    22725, 31521, 29692, 26722, 22725, 17855, 12299, 6270,
    21407, 29692, 27969, 25172, 21407, 16819, 11585, 5906,
    19266, 26722, 25172, 22654, 19266, 15137, 10426, 5315,
    16384, 22725, 21407, 19266, 16384, 12873, 8867, 4520,
    12873, 17855, 16819, 15137, 12873, 10114, 6967, 3552,
    8867, 12299, 11585, 10426, 8867, 6967, 4799, 2446,
    4520, 6270, 5906, 5315, 4520, 3552, 2446, 1247], dtype=np.int64)

# jidctfst.c, CONST_BITS = 8
FIX_1_082, FIX_1_414, FIX_1_847, FIX_2_613 = 277, 362, 473, 669
# jidctfst-sse2.asm: PRE_MULTIPLY_SCALE_BITS = 2, CONST_SHIFT = 16 - 2 - 8; F_1_613 = F_2_613 - 256
PW_F1414, PW_F1847, PW_MF1613, PW_F1082 = FIX_1_414 << 6, FIX_1_847 << 6, -(FIX_2_613 - 256) << 6, FIX_1_082 << 6


def w16(x):
    """wrap to int16"""
    return ((np.asarray(x, dtype=np.int64) + 32768) & 0xFFFF) - 32768


def multiplier_table(q):
    """jddctmgr.c, JDCT_IFAST: the int16 multiplier table from a quantisation table (natural order, up to 16 bits)."""
    return w16((np.asarray(q, dtype=np.int64) * AANSCALES + 2048) >> 12)


def _pmulhw(a, k):
    return (w16(a) * k) >> 16


def _pass_simd(d):
    """One 1-D pass of jsimd_idct_ifast_sse2 along axis 1 of d (int16 values as int64, any shape [n, 8, ...])."""
    i = [d[:, k] for k in range(8)]
    tmp10, tmp11, tmp13 = w16(i[0] + i[4]), w16(i[0] - i[4]), w16(i[2] + i[6])
    tmp12 = w16(_pmulhw(w16(i[2] - i[6]) << 2, PW_F1414) - tmp13)
    tmp0, tmp3, tmp1, tmp2 = w16(tmp10 + tmp13), w16(tmp10 - tmp13), w16(tmp11 + tmp12), w16(tmp11 - tmp12)
    z13, z10, z11, z12 = w16(i[5] + i[3]), w16(i[5] - i[3]), w16(i[1] + i[7]), w16(i[1] - i[7])
    tmp7 = w16(z11 + z13)
    tmp11 = _pmulhw(w16(z11 - z13) << 2, PW_F1414)
    z10s, z12s = w16(z10 << 2), w16(z12 << 2)
    z5 = _pmulhw(z10s + z12s, PW_F1847)
    tmp12 = w16(_pmulhw(z10s, PW_MF1613) - z10 + z5)
    tmp10 = w16(_pmulhw(z12s, PW_F1082) - z5)
    tmp6 = w16(tmp12 - tmp7)
    tmp5 = w16(tmp11 - tmp6)
    tmp4 = w16(tmp10 + tmp5)
    out = [tmp0 + tmp7, tmp1 + tmp6, tmp2 + tmp5, tmp3 - tmp4, tmp3 + tmp4, tmp2 - tmp5, tmp1 - tmp6, tmp0 - tmp7]
    return np.stack([w16(o) for o in out], axis=1)


def idct_blocks_simd(coef, mult):
    """coef int [n, 64] natural order, mult = multiplier_table(q) -> uint8 [n, 8, 8] (row, column)."""
    c = np.asarray(coef, dtype=np.int64).reshape(-1, 8, 8)
    d = w16(c * np.asarray(mult, dtype=np.int64).reshape(1, 8, 8))
    ws = _pass_simd(d)                                   # columns: along the row index
    rows = _pass_simd(ws.transpose(0, 2, 1))             # rows: [n, column, row]
    return (np.clip(rows >> 5, -128, 127) + 128).astype(np.uint8).transpose(0, 2, 1)


def _mul_c(x, k):
    """MULTIPLY(var, const) of jidctfst.c: DESCALE in JLONG, then the cast to DCTELEM (short)"""
    return w16((np.asarray(x, dtype=np.int64) * k) >> 8)


def _odd_even_c(i):
    """The butterflies of one 1-D pass of jidctfst.c on DCTELEM (short) inputs; returns the eight sums in int (unwrapped)."""
    tmp10, tmp11, tmp13 = w16(i[0] + i[4]), w16(i[0] - i[4]), w16(i[2] + i[6])
    tmp12 = w16(_mul_c(i[2] - i[6], FIX_1_414) - tmp13)
    tmp0, tmp3, tmp1, tmp2 = w16(tmp10 + tmp13), w16(tmp10 - tmp13), w16(tmp11 + tmp12), w16(tmp11 - tmp12)
    z13, z10, z11, z12 = w16(i[5] + i[3]), w16(i[5] - i[3]), w16(i[1] + i[7]), w16(i[1] - i[7])
    tmp7 = w16(z11 + z13)
    tmp11 = _mul_c(z11 - z13, FIX_1_414)
    z5 = _mul_c(z10 + z12, FIX_1_847)
    tmp10 = w16(_mul_c(z12, FIX_1_082) - z5)
    tmp12 = w16(_mul_c(z10, -FIX_2_613) + z5)
    tmp6 = w16(tmp12 - tmp7)
    tmp5 = w16(tmp11 - tmp6)
    tmp4 = w16(tmp10 + tmp5)
    return [tmp0 + tmp7, tmp1 + tmp6, tmp2 + tmp5, tmp3 - tmp4, tmp3 + tmp4, tmp2 - tmp5, tmp1 - tmp6, tmp0 - tmp7]


def _range_limit(x):
    """range_limit[IDESCALE(x, 5) & RANGE_MASK] of the 8-bit library (jdmaster.c prepare_range_limit_table)"""
    v = ((np.asarray(x, dtype=np.int64) >> 5) + 512 & 1023) - 512
    return np.clip(v + 128, 0, 255)


def idct_blocks_c(coef, mult):
    """jidctfst.c (DCTELEM = short): coef int [n, 64] natural order -> uint8 [n, 8, 8]."""
    c = np.asarray(coef, dtype=np.int64).reshape(-1, 8, 8)
    m = np.asarray(mult, dtype=np.int64).reshape(1, 8, 8)
    dq = c * m                                            # DEQUANTIZE: (short) coef * (short) mult, in int
    # pass 1 (columns) into the int workspace
    full = _odd_even_c([w16(dq[:, k]) for k in range(8)])
    ws = np.stack(full, axis=1)
    zero_ac = np.all(c[:, 1:, :] == 0, axis=1)           # [n, column]
    ws = np.where(zero_ac[:, None, :], dq[:, 0:1, :], ws)
    # pass 2 (rows)
    w = ws.transpose(0, 2, 1)                             # [n, column, row] -> index 1 walks along a row
    outs = np.stack(_odd_even_c([w16(w[:, k]) for k in range(8)]), axis=1)
    zero_row = np.all(w[:, 1:, :] == 0, axis=1)           # [n, row]
    outs = np.where(zero_row[:, None, :], w[:, 0:1, :], outs)
    return _range_limit(outs).astype(np.uint8).transpose(0, 2, 1)


def component_plane(coef, q, c_routine=False):
    """One component: coef int16 [bh, bw, 64] (oracle.decode_coefficients), q its quantisation table -> uint8 [bh*8, bw*8]."""
    bh, bw = coef.shape[:2]
    f = idct_blocks_c if c_routine else idct_blocks_simd
    blocks = f(coef.reshape(-1, 64), multiplier_table(q))
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def planes(jpeg, c_routine=False):
    """Every component's IFAST samples at its own resolution, cropped to the component's size (what P_YUV returns)."""
    import oracle
    info = oracle.read_info(jpeg)
    coefs, qts = oracle.decode_coefficients(jpeg)
    return [component_plane(co, q, c_routine)[:info["dh"][c], :info["dw"][c]] for c, (co, q) in enumerate(zip(coefs, qts))]


def _fancy_h2(cs, plus_left, plus_right, shift, edge_mul, edge_left, edge_right, width):
    """the horizontal triangle filter of jdsample.c on column sums cs [rows, dw] -> [rows, width]"""
    rows, dw = cs.shape
    out = np.zeros((rows, 2 * dw), dtype=np.int64)
    left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
    right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    out[:, 0::2] = (3 * cs + left + plus_left) >> shift
    out[:, 1::2] = (3 * cs + right + plus_right) >> shift
    out[:, 0] = (cs[:, 0] * edge_mul + edge_left) >> shift
    out[:, 2 * dw - 1] = (cs[:, dw - 1] * edge_mul + edge_right) >> shift
    return out[:, :width]


def upsample(plane, fx, fy, width, height):
    """One component to full size as libjpeg-turbo does it with fancy upsampling on (h2v1, h2v2 triangle filters; else replication)."""
    p = plane.astype(np.int64)
    dh, dw = p.shape
    if fx == 1 and fy == 1:
        return p[:height, :width]
    if fx == 2 and fy == 1 and dw > 2:
        return _fancy_h2(p, 1, 2, 2, 4, 0, 0, width)[:height]
    if fx == 2 and fy == 2 and dw > 2:
        y = np.arange(height)
        r0 = y >> 1
        r1 = np.clip(np.where(y & 1, r0 + 1, r0 - 1), 0, dh - 1)
        cs = 3 * p[r0] + p[r1]
        return _fancy_h2(cs, 8, 7, 4, 4, 8, 7, width)
    return np.repeat(np.repeat(p, fy, axis=0), fx, axis=1)[:height, :width]


def cmyk_samples(jpeg, c_routine=False):
    """The CMYK samples libjpeg-turbo gives for a four-component file with JDCT_IFAST (fancy upsampling on; YCCK converted as in
    jdcolor.c ycck_cmyk_convert) -> uint8 [H, W, 4]."""
    import oracle
    info = oracle.read_info(jpeg)
    W, H = info["width"], info["height"]
    full = [upsample(pl, info["hmax"] // info["h"][c], info["vmax"] // info["v"][c], W, H) for c, pl in enumerate(planes(jpeg, c_routine))]
    if info["colorspace"] == 4:
        y, cb, cr = full[0], full[1], full[2]
        r = np.clip(y + ((cr * 91881 + 32768 - 128 * 91881) >> 16), 0, 255)
        g = np.clip(y + ((cb * -22554 + cr * -46802 + 32768 + 128 * 22554 + 128 * 46802) >> 16), 0, 255)
        b = np.clip(y + ((cb * 116130 + 32768 - 128 * 116130) >> 16), 0, 255)
        full = [255 - r, 255 - g, 255 - b, full[3]]
    return np.stack(full, axis=2).astype(np.uint8)
