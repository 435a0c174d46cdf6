"""What the lossless coder must write, modelled in numpy: libjpeg-turbo's headers in lossless mode around the entropy-coded bytes of
tests/helpers/lossless_files.py, coded with ONE optimal table over the category counts of all components (the library forces optimized
coding in lossless mode).  tests/golden/make_golden_lossless_encode.py asserts that this model equals the live library on every golden;
the tests compare the coder with the model where no golden exists.  Also: the inputs of the goldens, rebuilt from the manifest's
seeds and parameters, and input descriptors with odd pitches and base offsets."""
import numpy as np

from helpers import lossless_files as LF

COMPONENT_IDS = {1: (1,), 2: (0, 1), 3: (0x52, 0x47, 0x42), 4: (0x43, 0x4D, 0x59, 0x4B)}
JFIF = LF._marker(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
ADOBE = LF._marker(0xEE, b"Adobe\0\x64\0\0\0\0\0")


def as_hwn(samples):
    s = np.asarray(samples)
    return s[:, :, None] if s.ndim == 2 else s


def differences(samples, precision, ps, pt=0, restart_rows=0):
    s = as_hwn(samples).astype(np.int64)
    return LF.differences_of_states(s >> pt, precision, ps, pt, restart_rows)


def pooled_table(diffs):
    ssss, _ = LF.categories(diffs)
    return LF.optimal_table(np.bincount(ssss.ravel(), minlength=17))


def headers(h, w, n, precision, ps, pt, restart_rows, table):
    """SOI, APPn, SOF3, DHT, [DRI], SOS as jcmarker.c writes them in lossless mode"""
    bits, vals = table
    ids = COMPONENT_IDS[n]
    out = b"\xff\xd8" + (JFIF if n == 1 else ADOBE if n >= 3 else b"")
    sof = bytes([precision]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([n])
    for c in range(n):
        sof += bytes([ids[c], 0x11, 0])
    out += LF._marker(0xC3, sof)
    out += LF._marker(0xC4, bytes([0]) + bytes(bits[1:17]) + bytes(vals))
    if restart_rows:
        out += LF._marker(0xDD, int(restart_rows * w).to_bytes(2, "big"))
    sos = bytes([n])
    for c in range(n):
        sos += bytes([ids[c], 0])
    return out + LF._marker(0xDA, sos + bytes([ps, 0, pt]))


def scan_bytes(data, n):
    """the entropy-coded segment and EOI of a file with one scan of n components"""
    sos = data.index(b"\xff\xda")
    return data[sos + 2 + 6 + 2 * n:]


def model_file(samples, precision, ps, pt=0, restart_rows=0):
    s = as_hwn(samples)
    h, w, n = s.shape
    rr = min(restart_rows, h) if restart_rows else 0  # one interval: no marker in the scan, DRI still names restart_rows
    d = differences(s, precision, ps, pt, rr)
    table = pooled_table(d)
    coded = LF.write_differences(d, precision, ps, pt, rr, tables=[table] * n)
    return headers(h, w, n, precision, ps, pt, restart_rows, table) + scan_bytes(coded, n)


def parse(data):
    """-> dict of what the markers say: precision, height, width, components, ids, predictor, point_transform, dri, order of segments"""
    out = {"order": [], "dri": 0}
    i = 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        length = int.from_bytes(data[i + 2:i + 4], "big")
        body = data[i + 4:i + 2 + length]
        out["order"].append(m)
        if m == 0xC3:
            out.update(precision=body[0], height=int.from_bytes(body[1:3], "big"), width=int.from_bytes(body[3:5], "big"), components=body[5],
                       ids=[body[6 + 3 * c] for c in range(body[5])], sampling=[body[7 + 3 * c] for c in range(body[5])])
        elif m == 0xDD:
            out["dri"] = int.from_bytes(body, "big")
        elif m == 0xC4:
            out.setdefault("dht", []).append(body[0])
        elif m == 0xDA:
            n = body[0]
            out.update(scan_ids=[body[1 + 2 * c] for c in range(n)], scan_tables=[body[2 + 2 * c] for c in range(n)], predictor=body[1 + 2 * n],
                       se=body[2 + 2 * n], point_transform=body[3 + 2 * n] & 15, ah=body[3 + 2 * n] >> 4)
            out["scan_at"] = i + 2 + length
            return out
        i += 2 + length


def case_samples(e):
    """The input of a manifest entry: H x W x N, uint8 for precision <= 8 else uint16"""
    h, w, n, P, pt = e["height"], e["width"], e["components"], e["precision"], e["point_transform"]
    dtype = np.uint8 if P <= 8 else np.uint16
    if e["kind"] == "constant":
        return np.full((h, w, n), e["seed"] % (1 << P), dtype=dtype)
    s = LF.random_samples(e["seed"], h, w, n, P, pt, e["smooth"])
    if pt:  # low bits that the point transform drops
        s = s + np.random.default_rng(e["seed"] + 1000).integers(0, 1 << pt, size=s.shape)
    if e["kind"] == "ssss16":  # a difference of 32768 under predictor 1: 0 then 32768 in one row
        s[h // 2, 0::2] = 0
        s[h // 2, 1::2] = 32768
    assert s.min() >= 0 and s.max() < (1 << P)
    return s.astype(dtype)


def expected(samples, pt):
    s = np.asarray(samples)
    return ((s.astype(np.int64) >> pt) << pt).astype(s.dtype)


def padded_input(N, samples, planar, pad, offset):
    """A hipjpegLosslessEncodeInput_t over a copy of the samples (H x W x N) with `pad` extra bytes per row and `offset` bytes in front of
    every plane.  -> (structure, components, the buffers to keep alive)"""
    s = as_hwn(samples)
    h, w, n = s.shape
    size = s.itemsize
    x = N.LosslessEncodeInput()
    x.sample_bytes, x.planar, x.width, x.height = size, 1 if planar else 0, w, h
    keep = []
    planes = [np.ascontiguousarray(s[:, :, c]) for c in range(n)] if planar else [np.ascontiguousarray(s).reshape(h, w * n)]
    for c, p in enumerate(planes):
        pitch = p.shape[1] * size + pad
        buf = np.full(offset + h * pitch + 16, 0xA5, dtype=np.uint8)
        rows = buf[offset:offset + h * pitch].reshape(h, pitch)
        rows[:, :p.shape[1] * size] = p.view(np.uint8).reshape(h, -1)
        x.plane[c] = buf.ctypes.data + offset
        x.pitch[c] = pitch
        keep.append(buf)
    return x, n, keep


def encode_raw_host(entry, x, n, precision, predictor=1, point_transform=0, restart_rows=0):
    """hipjpegEncodeLosslessHost / hipjpegEncodeLosslessGpuAlgorithmHost (`entry`) over a ready descriptor -> (status, file or None)"""
    import ctypes
    from nvimagecodec_amd import _native as N
    fn = getattr(N.load(), entry)
    p = N.LosslessEncodeParams(precision, predictor, point_transform, restart_rows, n)
    need = ctypes.c_size_t(0)
    st = fn(ctypes.byref(x), ctypes.byref(p), None, 0, ctypes.byref(need))
    if st != 9:
        return st, None
    out = np.empty(need.value, dtype=np.uint8)
    st = fn(ctypes.byref(x), ctypes.byref(p), out.ctypes.data, out.size, ctypes.byref(need))
    return st, out[:need.value].tobytes()


def encode_raw_batch(encoder, raws, precision, predictor, point_transform, restart_rows):
    """hipjpegEncodeLosslessBatch on a lowlevel.BatchLosslessEncoder's handle over ready descriptors [(structure, components)], one
    parameter list each -> (statuses, files)"""
    from nvimagecodec_amd import _native as N
    n = len(raws)
    X = (N.LosslessEncodeInput * max(n, 1))()
    P = (N.LosslessEncodeParams * max(n, 1))()
    for i, (x, comps) in enumerate(raws):
        X[i] = x
        P[i] = N.LosslessEncodeParams(precision[i], predictor[i], point_transform[i], restart_rows[i], comps)
    return encoder._encode(X, P, n)
