"""Lossless JPEG (SOF3, Huffman) files for the tests, and a numpy model of how they decode.

The rules (checked against libjpeg-turbo by tests/golden/make_golden_lossless.py, which uses this module):

  * one Huffman symbol SSSS per sample from a class-0 table: 0 = difference 0, 1..15 = SSSS extra bits with the usual sign
    extension, 16 = 32768 with no extra bits;
  * state x = (prediction + difference) & 0xFFFF per component and position, predictions from the state in plain integers:
    Ps 1: a, 2: b, 3: c, 4: a + b - c, 5: a + ((b - c) >> 1), 6: b + ((a - c) >> 1), 7: (a + b) >> 1 (a left, b above, c above-left);
  * the first sample of the picture and of every restart interval is predicted as 1 << (P - Pt - 1), the rest of that row from a,
    column 0 of every other row from b; a restart interval is a whole number of rows;
  * the sample is the low 16 bits of x << Pt, or the low 8 bits when P <= 8; nothing is clamped.

Writers: `write_samples` codes a picture so that it decodes to the samples given; `write_differences` codes any differences at all,
which is how states outside 0 .. 2^P - 1 are reached.
"""
import numpy as np

FLAT, OPTIMAL, LONG = "flat", "optimal", "long"


# ------------------------------------------------------------------------------------------------------------- the model
def predict(ps, a, b, c):
    """Works on Python ints and on int64 arrays alike (>> is arithmetic on both)."""
    if ps == 1:
        return a
    if ps == 2:
        return b
    if ps == 3:
        return c
    if ps == 4:
        return a + b - c
    if ps == 5:
        return a + ((b - c) >> 1)
    if ps == 6:
        return b + ((a - c) >> 1)
    if ps == 7:
        return (a + b) >> 1
    raise ValueError(ps)


def interval_rows(height, restart_rows):
    return restart_rows if restart_rows else height


def model_states(diffs, precision, ps, pt=0, restart_rows=0):
    """diffs: H x W x N differences (any integers, taken mod 2^16).  Returns the H x W x N states, sample by sample as the rules say."""
    d = np.asarray(diffs).astype(np.int64) & 0xFFFF
    h, w, n = d.shape
    rows = interval_rows(h, restart_rows)
    init = 1 << (precision - pt - 1)
    x = np.zeros((h, w, n), dtype=np.int64)
    for y in range(h):
        if y % rows == 0:
            # the interval's first row: init, then always the left neighbour -- a running sum
            x[y] = (init + np.cumsum(d[y], axis=0)) & 0xFFFF
            continue
        if ps == 1:
            first = (x[y - 1, 0] + d[y, 0]) & 0xFFFF
            x[y] = (first + np.cumsum(d[y], axis=0) - d[y, 0]) & 0xFFFF
            continue
        if ps in (2, 3):
            above = x[y - 1] if ps == 2 else np.concatenate([x[y - 1, :1], x[y - 1, :-1]], axis=0)  # column 0 is predicted from b
            x[y] = (above + d[y]) & 0xFFFF
            continue
        up = x[y - 1].tolist()
        dy = d[y].tolist()
        line = [[(up[0][k] + dy[0][k]) & 0xFFFF for k in range(n)]]
        for col in range(1, w):
            line.append([(predict(ps, line[col - 1][k], up[col][k], up[col - 1][k]) + dy[col][k]) & 0xFFFF for k in range(n)])
        x[y] = np.array(line, dtype=np.int64).reshape(w, n)
    return x


def samples_of_states(x, precision, pt=0):
    return ((np.asarray(x).astype(np.int64) << pt) & (0xFF if precision <= 8 else 0xFFFF)).astype(np.uint8 if precision <= 8 else np.uint16)


def model_decode(diffs, precision, ps, pt=0, restart_rows=0):
    """What a decoder returns for these differences: uint16 (uint8 when precision <= 8), H x W x N."""
    return samples_of_states(model_states(diffs, precision, ps, pt, restart_rows), precision, pt)


def differences_of_states(x, precision, ps, pt=0, restart_rows=0):
    """The differences (0 .. 65535) that make a decoder arrive at the states x (H x W x N, each 0 .. 65535)."""
    x = np.asarray(x).astype(np.int64)
    h, w, n = x.shape
    rows = interval_rows(h, restart_rows)
    a = np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 1:] = x[:-1, :-1]
    pred = predict(ps, a, b, c)
    pred[:, 0] = b[:, 0]
    first = np.arange(h) % rows == 0
    pred[first] = a[first]
    pred[first, 0] = 1 << (precision - pt - 1)
    return (x - pred) & 0xFFFF


# ------------------------------------------------------------------------------------------------------------- Huffman tables
def flat_table():
    """17 symbols, every code five bits long"""
    bits = [0] * 17
    bits[5] = 17
    return bits, list(range(17))


def long_table(order=None):
    """17 symbols with code lengths 2, 2, 3, 4, ... 15, 16, 16 in the order given (default 0 .. 16): the last two code words are 16 bits"""
    lengths = [2, 2] + list(range(3, 16)) + [16, 16]
    bits = [0] * 17
    for l in lengths:
        bits[l] += 1
    return bits, list(order if order is not None else range(17))


def optimal_table(freq):
    """T.81 K.2: code lengths from the symbol counts, no code of all ones, at most 16 bits.  freq: 17 counts."""
    freq = list(freq) + [1]  # the reserved code point
    nsym = len(freq)
    codesize = [0] * nsym
    others = [-1] * nsym
    while True:
        c1 = -1
        for i in range(nsym):
            if freq[i] and (c1 < 0 or freq[i] <= freq[c1]):
                c1 = i
        c2 = -1
        for i in range(nsym):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= freq[c2]):
                c2 = i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):
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
    bits[i] -= 1  # the reserved code point leaves
    vals = [s for l in range(1, 33) for s in range(nsym - 1) if codesize[s] == l]
    return bits[:17], vals


def _codes(bits, vals):
    code, k, out = 0, 0, {}
    for l in range(1, 17):
        for _ in range(bits[l]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def categories(diffs):
    """SSSS of each difference (taken mod 2^16, read as -32767 .. 32768)"""
    d = np.asarray(diffs).astype(np.int64) & 0xFFFF
    signed = np.where(d > 32768, d - 65536, d)
    mag = np.abs(signed)
    ssss = np.zeros(d.shape, dtype=np.int64)
    for s in range(1, 17):
        ssss[mag >= (1 << (s - 1))] = s
    return ssss, signed


# ------------------------------------------------------------------------------------------------------------- the writer
def _pack(values, lengths):
    """Bit strings (value, length) joined most significant bit first, padded with ones to a whole byte, FF bytes stuffed"""
    values = np.asarray(values, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.int64)
    total = int(lengths.sum())
    starts = np.cumsum(lengths) - lengths
    idx = np.repeat(np.arange(len(lengths)), lengths)
    within = np.arange(total, dtype=np.int64) - np.repeat(starts, lengths)
    bits = ((values[idx] >> (lengths[idx] - 1 - within).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, dtype=np.uint8)])
    raw = np.packbits(bits)
    ff = np.flatnonzero(raw == 0xFF)
    return np.insert(raw, ff + 1, 0).tobytes()


def _marker(m, payload=b""):
    return bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def write_differences(diffs, precision, ps, pt=0, restart_rows=0, comp_ids=None, table=OPTIMAL, tables=None, sampling=None,
                      restart_interval=None, scan_order=None, extra_markers=b"", scan_header=None):
    """diffs: H x W x N.  table: FLAT, OPTIMAL (per file and component), LONG, or tables = [(bits, vals)] per component.
    The remaining arguments bend the file away from what the decoder takes: sampling = [(h, v)] per component, restart_interval = the
    DRI value itself (default restart_rows * W), scan_header = (Ss, Se, Ah, Al) as written."""
    d = np.asarray(diffs).astype(np.int64) & 0xFFFF
    h, w, n = d.shape
    comp_ids = list(comp_ids) if comp_ids is not None else list(range(1, n + 1))
    sampling = sampling or [(1, 1)] * n
    ssss, signed = categories(d)
    if tables is None:
        if table == FLAT:
            tables = [flat_table()] * n
        elif table == LONG:
            tables = [long_table()] * n
        else:
            tables = [optimal_table(np.bincount(ssss[:, :, c].ravel(), minlength=17)) for c in range(n)]
    out = bytearray(b"\xff\xd8") + bytes(extra_markers)
    for c, (bits, vals) in enumerate(tables):
        out += _marker(0xC4, bytes([c]) + bytes(bits[1:17]) + bytes(vals))
    sof = bytes([precision]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([n])
    for c in range(n):
        sof += bytes([comp_ids[c], (sampling[c][0] << 4) | sampling[c][1], 0])
    out += _marker(0xC3, sof)
    rows = interval_rows(h, restart_rows)
    dri = restart_interval if restart_interval is not None else (restart_rows * w if restart_rows else 0)
    if dri:
        out += _marker(0xDD, int(dri).to_bytes(2, "big"))
    order = list(scan_order) if scan_order is not None else list(range(n))
    sos = bytes([n])
    for c in order:
        sos += bytes([comp_ids[c], c << 4])
    ss, se, ah, al = scan_header if scan_header is not None else (ps, 0, 0, pt)
    out += _marker(0xDA, sos + bytes([ss, se, (ah << 4) | al]))
    # code word and extra bits of every sample as one bit string
    code = np.zeros(d.shape, dtype=np.uint64)
    length = np.zeros(d.shape, dtype=np.int64)
    for c in range(n):
        lut = _codes(*tables[c])
        cw = np.array([lut.get(s, (0, 0))[0] for s in range(17)], dtype=np.uint64)
        cl = np.array([lut.get(s, (0, 0))[1] for s in range(17)], dtype=np.int64)
        assert (cl[np.unique(ssss[:, :, c])] > 0).all(), "the table lacks a category the picture uses"
        s = ssss[:, :, c]
        extra_len = np.where(s == 16, 0, s)
        extra = np.where(signed[:, :, c] < 0, signed[:, :, c] - 1, signed[:, :, c]) & ((1 << extra_len) - 1)
        code[:, :, c] = (cw[s] << extra_len.astype(np.uint64)) | extra.astype(np.uint64)
        length[:, :, c] = cl[s] + extra_len
    code, length = code[:, :, order], length[:, :, order]
    for k, y0 in enumerate(range(0, h, rows)):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += _pack(code[y0:y0 + rows].ravel(), length[y0:y0 + rows].ravel())
    out += b"\xff\xd9"
    return bytes(out)


def with_stuffed_byte(diffs, at=(0, 0, 0)):
    """A stuffed FF 00 on demand: the differences with 32767 planted at `at`.  Under the FLAT table that is code 01111 and fifteen
    one-bits, nineteen ones in a row, which cover a whole byte wherever they fall; the writer stuffs a zero behind it."""
    d = np.array(diffs, dtype=np.int64)
    d[at] = 32767
    return d


def has_stuffed_byte(data):
    sos = data.index(b"\xff\xda")
    return b"\xff\x00" in data[sos:]


def write_samples(samples, precision, ps, pt=0, restart_rows=0, **kw):
    """samples: H x W x N (or H x W), each 0 .. 2^P - 1 with the low Pt bits zero; the file decodes to exactly these."""
    s = np.asarray(samples).astype(np.int64)
    if s.ndim == 2:
        s = s[:, :, None]
    assert ((s >> pt) << pt == s).all() and s.min() >= 0 and s.max() < (1 << precision)
    return write_differences(differences_of_states(s >> pt, precision, ps, pt, restart_rows), precision, ps, pt, restart_rows, **kw)


def random_samples(seed, height, width, ncomp, precision, pt=0, smooth=True):
    """A smooth ramp plus noise (small differences, short codes) or plain noise (every category up to P)"""
    rng = np.random.default_rng(seed)
    top = 1 << (precision - pt)
    if smooth and top > 4:
        y, x = np.mgrid[0:height, 0:width]
        base = (x * 3 + y * 5)[:, :, None] + np.arange(ncomp) * 7
        s = (base + rng.integers(-2, 3, size=(height, width, ncomp))) % top
    else:
        s = rng.integers(0, top, size=(height, width, ncomp))
    return (s.astype(np.int64) << pt)
