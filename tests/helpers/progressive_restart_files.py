"""Test helper: a progressive (SOF2) file with a CHOSEN scan script AND a restart interval per scan, in the manner of write_progressive
(jpeg_from_coefficients.py), for the layouts libjpeg's writers do not produce: AC bands cut anywhere with intervals of any length, DC
scans whose intervals cut the blocks differently from scan to scan, AC scans of one component with different intervals.
Coding follows jcphuff.c including its end-of-band RUNS (bounded by max_run), so that runs are cut by the markers: before every
marker the pending run and its correction bits are written out (the band is closed), the bits are padded to a byte with 1-bits, RSTn
counts modulo 8, and the DC predictors start over.  Plain Python + numpy; small pictures only."""
from helpers.jpeg_from_coefficients import DC_CHROMA, DC_LUMA, ZIGZAG, _Bits, _codes, _magnitude, block_grid, random_coefficients  # noqa: F401


# An AC table that has what a progressive coder needs and Annex K lacks -- the end-of-band RUN symbols EOB1..EOB14 (run << 4, size 0):
# end of band and its runs, sixteen zeros, then (run, size) by size: the first 100 symbols in 7 bits, 40 in 8 bits, the last 36 (sizes 8 to
# 10) in 10 bits -- nine 8-bit prefixes that continue, the most second-level lookup tables the kernels take
_AC_PROG_VALS = [r << 4 for r in range(15)] + [0xF0] + [(r << 4) | s for s in range(1, 11) for r in range(16)]
AC_PROG = ([0] * 6 + [100, 40, 0, len(_AC_PROG_VALS) - 140] + [0] * 6, _AC_PROG_VALS)


class _AcCoder:
    """jcphuff.c's AC coders for one scan: the end-of-band run and the correction bits buffered behind it."""

    def __init__(self, bw, codes, max_run):
        self.bw, self.codes, self.max_run = bw, codes, max_run
        self.eobrun = 0
        self.pending = []  # correction bits of the blocks inside the run (BE)

    def close_band(self):  # emit_eobrun
        if self.eobrun:
            nbits = self.eobrun.bit_length() - 1
            self.bw.put(*self.codes[nbits << 4])
            if nbits:
                self.bw.put(self.eobrun & ((1 << nbits) - 1), nbits)
            self.eobrun = 0
        for b in self.pending:
            self.bw.put(b, 1)
        self.pending = []

    def first(self, blk, ss, se, al):  # encode_mcu_AC_first
        run = 0
        for k in range(ss, se + 1):
            val = int(blk[ZIGZAG[k]])
            mag = abs(val) >> al
            if mag == 0:
                run += 1
                continue
            self.close_band()
            while run > 15:
                self.bw.put(*self.codes[0xF0])
                run -= 16
            nb, bits = _magnitude(mag if val > 0 else -mag)
            assert nb <= 10
            self.bw.put(*self.codes[(run << 4) | nb])
            self.bw.put(bits, nb)
            run = 0
        if run:
            self.eobrun += 1
            if self.eobrun >= self.max_run:
                self.close_band()

    def refine(self, blk, ss, se, al):  # encode_mcu_AC_refine
        mags = {k: abs(int(blk[ZIGZAG[k]])) >> al for k in range(ss, se + 1)}
        eob = max([k for k in mags if mags[k] == 1], default=0)  # the last coefficient that becomes non-zero in this pass
        run, mine = 0, []  # `mine`: correction bits of this block (BR)
        for k in range(ss, se + 1):
            mag = mags[k]
            if mag == 0:
                run += 1
                continue
            while run > 15 and k <= eob:
                self.close_band()
                self.bw.put(*self.codes[0xF0])
                run -= 16
                for b in mine:
                    self.bw.put(b, 1)
                mine = []
            if mag > 1:  # non-zero before: its next bit, behind the next symbol
                mine.append(mag & 1)
                continue
            self.close_band()
            self.bw.put(*self.codes[(run << 4) | 1])
            self.bw.put(0 if int(blk[ZIGZAG[k]]) < 0 else 1, 1)
            for b in mine:
                self.bw.put(b, 1)
            mine, run = [], 0
        if run > 0 or mine:
            self.eobrun += 1
            self.pending += mine
            if self.eobrun >= self.max_run or len(self.pending) > 900:
                self.close_band()


def write_progressive_restart(width, height, sampling, coefficients, qtables, script, intervals, max_run=0x7FFF):
    """script: as write_progressive -- ("dc", [component, ...], ah, al) and ("ac", component, ss, se, ah, al).  intervals: one restart
    interval per scan of the script (MCUs of an interleaved scan, blocks of a one-component scan; 0 = none for that scan), written as a
    DRI segment in front of the scan's SOS.  max_run: the longest end-of-band run the coder lets grow (1: every block closes its band).
    Other arguments as write_baseline (8-bit tables only); the AC scans use AC_PROG.  Returns the file as bytes."""
    assert len(intervals) == len(script)
    ncomp = len(sampling)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcus_x, mcus_y = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = bytearray(b"\xff\xd8")
    for c in range(ncomp):
        q = [int(qtables[c][ZIGZAG[k]]) for k in range(64)]
        assert all(1 <= x <= 255 for x in q)
        out += b"\xff\xdb" + (67).to_bytes(2, "big") + bytes([c]) + bytes(q)
    out += b"\xff\xc2" + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(sampling):
        out += bytes([c + 1, (h << 4) | v, c])
    tables = [(0x00, DC_LUMA), (0x10, AC_PROG)] + ([(0x01, DC_CHROMA), (0x11, AC_PROG)] if ncomp > 1 else [])
    for ident, (bits, vals) in tables:
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([ident]) + bytes(bits) + bytes(vals)
    dc_codes = [_codes(*DC_LUMA)] + [_codes(*DC_CHROMA)] * (ncomp - 1)
    ac_codes = [_codes(*AC_PROG)] * ncomp

    def real_blocks(c):
        h, v = sampling[c]
        cw, ch = -(-width * h // hmax), -(-height * v // vmax)  # the component's samples
        return -(-cw // 8), -(-ch // 8)

    for entry, interval in zip(script, intervals):
        out += b"\xff\xdd" + (4).to_bytes(2, "big") + int(interval).to_bytes(2, "big")
        bw = _Bits()
        if entry[0] == "dc":
            comps = list(entry[1])
            ah, al = (entry[2], entry[3]) if len(entry) > 2 else (0, 0)
            out += b"\xff\xda" + (6 + 2 * len(comps)).to_bytes(2, "big") + bytes([len(comps)])
            for c in comps:
                out += bytes([c + 1, 0x00 if c == 0 else 0x10])
            out += bytes([0, 0, (ah << 4) | al])
            if len(comps) == 1:
                nbx, nby = real_blocks(comps[0])
                units = [[(comps[0], y, x)] for y in range(nby) for x in range(nbx)]
            else:
                units = [[(c, my * sampling[c][1] + by, mx * sampling[c][0] + bx) for c in comps for by in range(sampling[c][1]) for bx in range(sampling[c][0])]
                         for my in range(mcus_y) for mx in range(mcus_x)]
            coder = None
        else:
            c, ss, se = entry[1], entry[2], entry[3]
            ah, al = (entry[4], entry[5]) if len(entry) > 4 else (0, 0)
            assert 1 <= ss <= se <= 63
            out += b"\xff\xda" + (8).to_bytes(2, "big") + bytes([1, c + 1, 0x00 if c == 0 else 0x11, ss, se, (ah << 4) | al])
            nbx, nby = real_blocks(c)
            units = [[(c, y, x)] for y in range(nby) for x in range(nbx)]
            coder = _AcCoder(bw, ac_codes[c], max_run)
        pred = {}
        for m, unit in enumerate(units):
            if interval and m and m % interval == 0:
                if coder:
                    coder.close_band()
                bw.flush()  # pads with 1-bits
                bw.out += bytes([0xFF, 0xD0 + (m // interval - 1) % 8])
                pred = {}
            for c, y, x in unit:
                blk = coefficients[c][y][x]
                if coder:
                    (coder.refine if ah else coder.first)(blk, ss, se, al)
                elif ah:  # DC refinement: the next bit of the value
                    bw.put((int(blk[0]) >> al) & 1, 1)
                else:
                    v = int(blk[0]) >> al  # arithmetic shift (encode_mcu_DC_first)
                    diff = v - pred.get(c, 0)
                    pred[c] = v
                    nb, bits = _magnitude(diff)
                    assert nb <= 11
                    bw.put(*dc_codes[c][nb])
                    if nb:
                        bw.put(bits, nb)
        if coder:
            coder.close_band()
        bw.flush()
        out += bw.out
    out += b"\xff\xd9"
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
# What tests/test_progressive_intervals.py (host emulation) and tests/test_gpu_progressive_intervals.py (kernels) both decode.
S444 = [(1, 1), (1, 1), (1, 1)]
S420 = [(2, 2), (1, 1), (1, 1)]
GRAY = [(1, 1)]

# name -> (sampling, width, height, script, restart interval per scan, max_run, dense)
HELPER_CASES = {
    # AC bands cut anywhere, refinement passes over parts of a band, DC refined late; 88 blocks per component, 88 MCUs.  Luma has the
    # six AC scans the kernels take at most, all with interval 7; 87 = two intervals, the second of one block
    "bands_cut_anywhere": (S444, 83, 61, [
        ("dc", [0, 1, 2], 0, 2), ("ac", 0, 1, 5, 0, 2), ("ac", 0, 6, 63, 0, 2), ("ac", 1, 1, 63, 0, 1), ("ac", 2, 1, 63, 0, 1),
        ("ac", 0, 1, 5, 2, 1), ("dc", [0, 1, 2], 2, 1), ("ac", 0, 6, 63, 2, 1), ("ac", 0, 1, 20, 1, 0), ("ac", 0, 21, 63, 1, 0),
        ("ac", 1, 1, 9, 1, 0), ("ac", 1, 10, 63, 1, 0), ("dc", [1], 1, 0), ("dc", [0, 2], 1, 0), ("ac", 2, 1, 63, 1, 0)],
        [5, 7, 7, 3, 87, 7, 9, 7, 7, 7, 3, 3, 10, 4, 87], 0x7FFF, 3),
    # three bit planes; 24 MCUs, 88 luma and 24 chroma blocks (24 = no marker at all in that component's scans)
    "three_bit_planes": (S420, 83, 61, [
        ("dc", [0], 0, 0), ("dc", [1, 2], 0, 0), ("ac", 0, 1, 63, 0, 3), ("ac", 1, 1, 63, 0, 3), ("ac", 2, 1, 63, 0, 3),
        ("ac", 0, 1, 63, 3, 2), ("ac", 0, 1, 63, 2, 1), ("ac", 1, 1, 63, 3, 2), ("ac", 2, 1, 63, 3, 2), ("ac", 0, 1, 63, 1, 0),
        ("ac", 1, 1, 63, 2, 1), ("ac", 1, 1, 63, 1, 0), ("ac", 2, 1, 63, 2, 1), ("ac", 2, 1, 63, 1, 0)],
        [6, 5, 13, 1, 24, 13, 13, 1, 24, 13, 1, 1, 24, 24], 3, 2),
    # the interleaved DC scan cuts the blocks into intervals of 5 MCUs, the per-component refinements into 3 / 5 / 1 blocks
    "dc_recut_per_component": (S420, 50, 37, [
        ("dc", [0, 1, 2], 0, 1), ("ac", 0, 1, 63), ("ac", 1, 1, 63), ("ac", 2, 1, 63), ("dc", [0], 1, 0), ("dc", [1], 1, 0), ("dc", [2], 1, 0)],
        [5, 4, 2, 12, 3, 5, 1], 0x7FFF, 2),
    # 500 blocks, 500 intervals per scan: two workgroups of the interval kernels, the second partly filled
    "gray_500_intervals": (GRAY, 200, 160, [("dc", [0], 0, 1), ("ac", 0, 1, 63, 0, 1), ("dc", [0], 1, 0), ("ac", 0, 1, 63, 1, 0)], [1, 1, 1, 1], 0x7FFF, 3),
}
# luma's AC scans have different intervals: interval i does not cover the same blocks in both, the host entropy stage keeps the file
DIFFERENT_INTERVALS = (S444, 33, 17, [("dc", [0, 1, 2]), ("ac", 0, 1, 5), ("ac", 0, 6, 63), ("ac", 1, 1, 63), ("ac", 2, 1, 63)], [2, 3, 4, 3, 3], 0x7FFF, 3)


def helper_file(case):
    """-> (file, chosen coefficients) of HELPER_CASES[name] or of a case tuple."""
    import numpy as np
    samp, w, h, script, intervals, max_run, dense = HELPER_CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng(w * 1000 + h + len(script))
    coefs = random_coefficients(rng, w, h, samp, 300, dense=dense, small=4, dc=40)
    qt = [np.full(64, 3 + c, dtype=np.int32) for c in range(len(samp))]
    return write_progressive_restart(w, h, samp, coefs, qt, script, intervals, max_run), coefs


def real_blocks(case, c):
    """(rows, columns) of component c's real blocks."""
    samp, w, h = (HELPER_CASES[case] if isinstance(case, str) else case)[:3]
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    cw, ch = -(-w * samp[c][0] // hmax), -(-h * samp[c][1] // vmax)
    return -(-ch // 8), -(-cw // 8)


def flat_picture(gray=False):
    """320 x 200, flat but for one textured patch: long end-of-band runs, cut by the restart markers."""
    import numpy as np
    from nvimagecodec_amd.synth import synth_image
    im = np.full((200, 320, 3), 128, dtype=np.uint8)
    im[80:130, 120:200] = synth_image(80, 50, seed=3)
    return im[:, :, 1].copy() if gray else im


def pillow_files():
    """[(id, file)]: libjpeg-turbo's progressive files with restart markers every MCU row / every 1 / every 5 blocks.  Needs Pillow."""
    import io
    from PIL import Image
    res = []
    for sub in ("444", "420", "gray"):
        im = Image.fromarray(flat_picture(sub == "gray"))
        for q in (30, 90, 100):
            for key, kw in (("rows1", {"restart_marker_rows": 1}), ("blocks1", {"restart_marker_blocks": 1}), ("blocks5", {"restart_marker_blocks": 5})):
                b = io.BytesIO()
                extra = {} if sub == "gray" else {"subsampling": {"444": 0, "420": 2}[sub]}
                im.save(b, "JPEG", quality=q, progressive=True, **extra, **kw)
                res.append(("pillow_%s_q%d_%s" % (sub, q, key), b.getvalue()))
    return res


def transcode_products(golden_dir):
    """[(id, file)]: the project's own progressive coder with restart_interval 1, 3, the luma block count - 1 and 1000 (a DRI and no marker)."""
    import os
    from nvimagecodec_amd import lowlevel
    res = []
    for name, blocks in (("s17x13_444_base_q90", 3 * 2), ("s33x65_420_base_q90", 5 * 9), ("s17x13_gray_base_q90", 3 * 2)):
        with open(os.path.join(golden_dir, "decode", name + ".jpg"), "rb") as f:
            base = f.read()
        for r in (1, 3, blocks - 1, 1000):
            res.append(("%s_r%d" % (name, r), lowlevel.transcode_host(base, progressive=True, restart_interval=r)))
    return res
