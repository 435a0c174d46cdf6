"""Test helper: an existing sequential JPEG file re-coded into a CHOSEN list of sequential scans (T.81 allows a sequential frame to
code its components in several scans, in any order inside a scan).  Every segment in front of the first SOS is kept byte for byte
except the Huffman tables (DHT): APPn / Adobe, DQT, SOF, component ids and the colour signalling stay as they were.  The quantized
coefficients are the oracle's (oracle.decode_coefficients), so a re-coded file decodes to exactly the pixels of the original.

Each scan gets Huffman tables built for the symbols it codes (T.81 K.2, the all-ones code kept free), written in a DHT in front of
it; the scan's i-th component uses table slot i % 2, so that one scan uses two tables and the next one redefines both slots.  A DRI
in front of a scan sets its restart interval where it differs from the one in force.  Plain Python + numpy; small pictures are
quick, a 4K picture takes a few seconds."""
import numpy as np

from helpers.jpeg_from_coefficients import ZIGZAG, _Bits, _magnitude


class DcOutOfRange(ValueError):
    """A DC difference in the new block order does not fit category 11 (baseline / 8-bit): the file cannot be re-coded so."""


def _segments(data):
    """-> (list of (marker, whole segment bytes) in front of the first SOS, restart interval in force there)"""
    assert data[:2] == b"\xff\xd8"
    pos, segs, dri = 2, [], 0
    while True:
        while data[pos] == 0xFF and data[pos + 1] == 0xFF:
            pos += 1
        assert data[pos] == 0xFF, "marker expected"
        m = data[pos + 1]
        if m == 0xDA:
            return segs, dri
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos:pos + 2 + n]
        if m == 0xDD:
            dri = int.from_bytes(seg[4:6], "big")
        segs.append((m, seg))
        pos += 2 + n


def _frame(segs):
    for m, seg in segs:
        if m in (0xC0, 0xC1):
            h, w, nc = int.from_bytes(seg[5:7], "big"), int.from_bytes(seg[7:9], "big"), seg[9]
            comps = [(seg[10 + 3 * i], seg[11 + 3 * i] >> 4, seg[11 + 3 * i] & 15) for i in range(nc)]
            return w, h, comps
    raise ValueError("not a sequential (SOF0 / SOF1) file")


def _code_lengths(freq):
    """T.81 K.2: optimal code lengths for the symbols with freq > 0, at most 16 bits; a reserved pseudo-symbol keeps the all-ones
    code free.  -> (bits[16], vals)"""
    freq = list(freq) + [1]  # symbol 256: reserved
    n = len(freq)
    size = [0] * n
    others = [-1] * n
    f = [x if x > 0 else 0 for x in freq]
    while True:
        c1 = c2 = -1
        for i in range(n):  # c1 = least frequent (ties: the larger index), c2 = next
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        for i in range(n):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    bits = [0] * 33
    for i in range(n):
        if size[i]:
            bits[size[i]] += 1
    for i in range(32, 16, -1):  # K.3 adjustment to 16 bits
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved symbol goes
    vals = []
    for length in range(1, 33):
        for s in range(256):
            if size[s] == length:
                vals.append(s)
    return bits[1:17], vals


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def _dht(tc, th, bits, vals):
    body = bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def _scan_blocks(width, height, comps, coefs, scan):
    """Blocks of the scan in coding order: list of (slot, natural-order coefficients); one-component scans cover the real blocks only."""
    hmax, vmax = max(h for _, h, _ in comps), max(v for _, _, v in comps)
    if len(scan) == 1:
        c = scan[0]
        _, h, v = comps[c]
        sw, sh = -(-width * h // hmax), -(-height * v // vmax)
        return [(0, coefs[c][by, bx]) for by in range(-(-sh // 8)) for bx in range(-(-sw // 8))], -(-sw // 8) * -(-sh // 8)
    mx_n, my_n = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = []
    for my in range(my_n):
        for mx in range(mx_n):
            for slot, c in enumerate(scan):
                _, h, v = comps[c]
                for dy in range(v):
                    for dx in range(h):
                        out.append((slot, coefs[c][my * v + dy, mx * h + dx]))
    return out, mx_n * my_n


def _symbols(blocks, bpm, restart):
    """-> per block: (slot, [(table 'dc'/'ac', symbol, extra value, extra bits)]) with DC prediction per slot, reset at restarts."""
    pred = {}
    coded = []
    for b, (slot, blk) in enumerate(blocks):
        if restart and b % (restart * bpm) == 0:
            pred = {}
        zz = [int(blk[ZIGZAG[k]]) for k in range(64)]
        diff = zz[0] - pred.get(slot, 0)
        pred[slot] = zz[0]
        if abs(diff) > 2047:
            raise DcOutOfRange(diff)
        nb, bits = _magnitude(diff)
        syms = [("dc", nb, bits, nb)]
        run = 0
        for k in range(1, 64):
            if zz[k] == 0:
                run += 1
                continue
            while run > 15:
                syms.append(("ac", 0xF0, 0, 0))
                run -= 16
            nb, bits = _magnitude(zz[k])
            syms.append(("ac", (run << 4) | nb, bits, nb))
            run = 0
        if run:
            syms.append(("ac", 0x00, 0, 0))
        coded.append((slot, syms))
    return coded


def recode(data, scans, restarts=None, coefficients=None):
    """data: a sequential JPEG file; scans: list of lists of component indices (frame order numbers), e.g. [[0], [1, 2]];
    restarts: restart interval per scan (0 = none; default none); coefficients: the file's quantized coefficients as
    oracle.decode_coefficients gives them (default: taken from the oracle).  -> the re-coded file.  Raises DcOutOfRange when a DC
    difference of the new block order does not fit category 11."""
    segs, dri_in_force = _segments(data)
    width, height, comps = _frame(segs)
    if coefficients is None:
        import oracle
        coefficients = oracle.decode_coefficients(data)[0]
    coefs = coefficients
    restarts = list(restarts) if restarts is not None else [0] * len(scans)
    out = bytearray(b"\xff\xd8")
    for m, seg in segs:
        if m != 0xC4:
            out += seg
    for scan, restart in zip(scans, restarts):
        blocks, mcus = _scan_blocks(width, height, comps, coefs, scan)
        bpm = len(blocks) // mcus
        coded = _symbols(blocks, bpm, restart)
        # tables: slot i % 2 of each kind, built from the symbols of the components that use it
        nslots = min(2, len(scan))
        freq = {(k, t): [0] * 256 for k in ("dc", "ac") for t in range(nslots)}
        for slot, syms in coded:
            for kind, sym, _, _ in syms:
                freq[(kind, slot % 2)][sym] += 1
        codes = {}
        for (kind, t), fr in sorted(freq.items()):
            if not any(fr):
                fr[0] = 1
            bits, vals = _code_lengths(fr)
            out += _dht(0 if kind == "dc" else 1, t, bits, vals)
            codes[(kind, t)] = _codes(bits, vals)
        if restart != dri_in_force:
            out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
            dri_in_force = restart
        out += b"\xff\xda" + (6 + 2 * len(scan)).to_bytes(2, "big") + bytes([len(scan)])
        for slot, c in enumerate(scan):
            out += bytes([comps[c][0], ((slot % 2) << 4) | (slot % 2)])
        out += bytes([0, 63, 0])
        bw = _Bits()
        rst = 0
        for b, (slot, syms) in enumerate(coded):
            if restart and b and b % (restart * bpm) == 0:
                bw.flush()
                bw.out += bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
            for kind, sym, extra, nb in syms:
                code, length = codes[(kind, slot % 2)][sym]
                bw.put(code, length)
                if nb:
                    bw.put(extra, nb)
        bw.flush()
        out += bw.out
    out += b"\xff\xd9"
    return bytes(out)
