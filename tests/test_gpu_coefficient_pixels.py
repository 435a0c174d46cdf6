"""Coefficient tensors to pixels and pixels to coefficient tensors, on the device and with no entropy stage:
hipjpegCoefficientsToPixelsBatch (the caller's tensors -> coef_to_decoder_kernel -> the decoder's pixel kernels) and
hipjpegPixelsToCoefficientsBatch (the forward kernels -> coef_from_coder_kernel -> the caller's tensors).  The first is pinned to the
file decode (same pixels as hipjpegDecodeBatch for a file with those coefficients) and to the oracle, the second to the file route
(hipjpegDecodeCoefficientsHost of the file hipjpegEncodeBatch writes).

One mixed batch serves the pixel tests -- the smallest pictures at which the unit-to-image map and the grids can go wrong: one block;
real areas narrower than the MCU-padded grid on both axes; units that end inside a component (320x200 4:2:0: 1000 luma blocks);
several units and rounds (640x480); a component of exactly 256 blocks and one of 257; 4:1:1 / 4:1:0 / 4:4:0 and replicated layouts."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as J
from helpers import sampling_goldens as SG
from helpers import transcode_cases as T
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 3
SENTINEL = -21846  # 0xAAAA
PIXEL_SENTINEL = 0x5A
_GOLDENS = ["s1x1_gray_base_q90", "s8x8_420_base_q90", "s8x8_444_base_q50", "s17x13_420_base_q90", "s17x13_420_prog_q50", "s50x37_420_base_q50",
            "s50x37_gray_prog_q50", "s33x65_422_base_q90", "s3x5_420_base_q90", "s3x5_gray_base_q90", "s3x5_444_base_q90", "h320x200_420_opt_q75",
            "c1_640x480_444_base_q90", "s64x48_420_base_q90"]
_SAMPLING = ["y22cb11cr21_83x61", "y31c11_83x61_prog", "gray22_83x61_rst3"]


def _img(w, h, sub, seed, q=88):
    return oracle.encode(synth_image(w, h, seed=seed), sub, q)


@functools.lru_cache(maxsize=None)
def _batch():
    """[(name, file)]"""
    decode = dict(T.golden_files("decode"))
    files = [(n, decode[n]) for n in _GOLDENS]
    files += [("gray_128x128", _img(128, 128, "gray", 21)), ("gray_2056x8", _img(2056, 8, "gray", 22)),  # 256 and 257 blocks
              ("411_129x70", _img(129, 70, "411", 23)), ("410_70x45", _img(70, 45, "410", 24)), ("440_33x47", _img(33, 47, "440", 25))]
    by_name = {e["name"]: e for e in SG.ENTRIES}
    files += [("sampling_" + n, SG.jpeg(by_name[n])) for n in _SAMPLING]
    assert len(files) == 14 + 5 + 3
    return tuple(files)


@functools.lru_cache(maxsize=None)
def _host():
    """decode_coefficients_host of the batch: the tensors' source, computed once and left alone"""
    return tuple(lowlevel.decode_coefficients_host(d) for _, d in _batch())


@functools.lru_cache(maxsize=None)
def _file_decode(fmt, fancy, fast_idct=False):
    """BatchDecoder.decode of the batch's files: (statuses, outputs as numpy), computed once per configuration"""
    dec = lowlevel.BatchDecoder(device=0, num_threads=8)
    try:
        outs, statuses = dec.decode([d for _, d in _batch()], fmt=fmt, fancy=fancy, fast_idct=fast_idct, check=False)
        return tuple(statuses), tuple(_numpy(o) for o in outs)
    finally:
        dec.close()


def _numpy(o):
    if o is None:
        return None
    return [t.cpu().numpy() for t in o] if isinstance(o, (list, tuple)) else o.cpu().numpy()


def _same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def _upload(coefs, extra=0, fill=SENTINEL):
    import torch
    out = []
    for c in coefs:
        c = np.ascontiguousarray(c, dtype=np.int16).reshape(c.shape[0], c.shape[1], 8, 8)
        t = torch.full((c.shape[0], c.shape[1] + extra, 8, 8), fill, dtype=torch.int16, device="cuda:0")
        t[:, : c.shape[1]] = torch.from_numpy(c).to("cuda:0")
        out.append(t)
    return out


@pytest.fixture(scope="module")
def handle():
    h = lowlevel.BatchCoefficients(device=0, num_threads=8)
    yield h
    h.close()


def _real_blocks(indices):
    return sum(c.shape[0] * c.shape[1] for i in indices for c in _host()[i][1])


# ---------------------------------------------------------------- 1. parity with the file decode
@pytest.mark.parametrize("fmt,fancy,fast_idct", [(f, fancy, False) for f in ("rgb", "bgr_planar", "y", "yuv_planar") for fancy in (True, False)] +
                         [("rgb", True, True)])
def test_parity_with_file_decode(handle, fmt, fancy, fast_idct):
    """one call over the whole batch, every picture twice: pitch = blocks_w, and pitch = blocks_w + 3 with a sentinel in the extra blocks"""
    import torch
    want_statuses, want = _file_decode(fmt, fancy, fast_idct)
    if fmt == "rgb" and not fancy:
        assert want_statuses == (0,) * len(_batch())  # every image decodes (a replicated layout is declined where libjpeg would filter)
    assert sum(s == 0 for s in want_statuses) >= 19 and set(want_statuses) <= {0, UNSUPPORTED}
    images = [(info, _upload(coefs, extra)) for extra in (0, 3) for info, coefs in _host()]
    statuses, outs = handle.to_pixels(images, fmt=fmt, fancy=fancy, fast_idct=fast_idct)
    torch.cuda.synchronize()
    assert tuple(statuses) == want_statuses * 2
    names = [n for n, _ in _batch()] * 2
    wrong = [(n, k) for k, (n, st, a, b) in enumerate(zip(names, statuses, outs, want * 2)) if st == 0 and not _same(_numpy(a), b)]
    assert not wrong, wrong
    assert handle.stats()["moved_blocks"] == 2 * _real_blocks([i for i, st in enumerate(want_statuses) if st == 0])
    # the tensors are read only
    for (info, coefs), (_, tensors) in zip(_host() * 2, images):
        for ref, t in zip(coefs, tensors):
            got = t.cpu().numpy()
            assert np.array_equal(got[:, : ref.shape[1]], ref) and (got[:, ref.shape[1]:] == SENTINEL).all()


# ---------------------------------------------------------------- 2. against the oracle
def test_against_the_oracle(handle):
    import torch
    rng = np.random.default_rng(20260)
    ql, qc = oracle.quality_tables(50)
    cases = [(24, 24, [(2, 2), (1, 1), (1, 1)], [ql, qc, qc], 1023, 1), (16, 8, [(1, 1), (1, 1), (1, 1)], [ql, qc, qc], 1023, 1),
             (40, 8, [(1, 1)], [ql], 40, 2)]
    images, want = [], []
    for w, h, sampling, tables, extreme, scale in cases:
        coefs = J.random_coefficients(rng, w, h, sampling, extreme)
        written = J.write_baseline(w, h, sampling, coefs, tables)
        used = [np.asarray(t, dtype=np.uint16) * scale for t in tables]  # (gray: every quantizer doubled, in place of the file's)
        want.append(oracle.decode(J.write_baseline(w, h, sampling, coefs, used)))
        info = lowlevel.coefficient_info(written)
        assert [list(q) for q in info["qtables"]] == [list(np.asarray(t)) for t in tables]
        info["qtables"] = used
        real = [c[:bh, :bw] for c, bh, bw in zip(coefs, info["blocks_h"], info["blocks_w"])]
        images.append((info, _upload(real, extra=1)))
    statuses, outs = handle.to_pixels(images, fmt="rgb")
    torch.cuda.synchronize()
    assert statuses == [0, 0, 0]
    for k, (o, ref) in enumerate(zip(outs, want)):
        assert np.array_equal(o.cpu().numpy(), ref), k


# ---------------------------------------------------------------- 3. an edit on the stream
def test_edit_on_the_stream(handle):
    import torch
    names = [n for n, _ in _batch()]
    picked = [names.index(n) for n in ("s17x13_420_base_q90", "h320x200_420_opt_q75", "s50x37_gray_prog_q50")]
    want = []
    for i in picked:
        info, coefs = _host()[i]
        edited = [c.copy() for c in coefs]
        for c in edited:
            c.reshape(c.shape[0], c.shape[1], 64)[:, :, 1:] = 0
        want.append(oracle.decode(lowlevel.encode_coefficients_host(info, edited)))
    stream = torch.cuda.Stream(device=0)
    staged = [[torch.from_numpy(c).pin_memory() for c in _host()[i][1]] for i in picked]
    with torch.cuda.stream(stream):
        images = []
        for i, host in zip(picked, staged):
            tensors = [t.to("cuda:0", non_blocking=True) for t in host]
            for t in tensors:
                t.view(t.shape[0], t.shape[1], 64)[:, :, 1:] = 0
            images.append(lowlevel.CoefficientImage(_host()[i][0], tensors))
        statuses, outs = handle.to_pixels(images, fmt="rgb", stream=stream)
    stream.synchronize()
    assert statuses == [0, 0, 0]
    for i, o, ref in zip(picked, outs, want):
        assert np.array_equal(o.cpu().numpy(), ref), names[i]


# ---------------------------------------------------------------- 4. what an earlier batch left in the arena
def test_stale_arena():
    import torch
    names = [n for n, _ in _batch()]
    big = names.index("c1_640x480_444_base_q90")
    small = [names.index(n) for n in ("s17x13_420_base_q90", "s3x5_420_base_q90")]
    want_statuses, want = _file_decode("rgb", True)
    h = lowlevel.BatchCoefficients(device=0, num_threads=2)
    try:
        info = _host()[big][0]
        full = [torch.full((bh, bw, 8, 8), 1023, dtype=torch.int16, device="cuda:0") for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
        statuses, _ = h.to_pixels([(info, full)])
        assert statuses == [0]
        for fancy in (True, False):
            statuses, outs = h.to_pixels([(_host()[i][0], _upload(_host()[i][1])) for i in small], fancy=fancy)
            torch.cuda.synchronize()
            assert statuses == [0, 0]
            ref = _file_decode("rgb", fancy)[1]
            for i, o in zip(small, outs):
                assert np.array_equal(o.cpu().numpy(), ref[i]), (names[i], fancy)
    finally:
        h.close()


# ---------------------------------------------------------------- 5. geometry
def test_geometry(handle):
    import torch
    files = dict(_batch())
    names = [n for n, _ in _batch()]
    picked = ["h320x200_420_opt_q75", "s50x37_420_base_q50"]
    transforms = [((16, 8, 200, 150), 6), (None, 3)]
    dec = lowlevel.BatchDecoder(device=0, num_threads=2)
    try:
        want, st = dec.decode([files[n] for n in picked], transforms=transforms)
        want = [o.cpu().numpy() for o in want]
        assert list(st) == [0, 0] and want[0].shape == (184, 142, 3) and want[1].shape == (37, 50, 3)
        _, want_yuv = dec.decode([files[n] for n in picked], fmt="yuv_planar", transforms=transforms, check=False)
        assert list(want_yuv) == [UNSUPPORTED, UNSUPPORTED]
    finally:
        dec.close()
    images = [(_host()[names.index(n)][0], _upload(_host()[names.index(n)][1])) for n in picked]
    statuses, outs = handle.to_pixels(images, transforms=transforms)
    torch.cuda.synchronize()
    assert statuses == [0, 0]
    for n, o, ref in zip(picked, outs, want):
        assert np.array_equal(o.cpu().numpy(), ref), n
    # the transforms were consumed by that batch
    statuses, outs = handle.to_pixels(images)
    torch.cuda.synchronize()
    assert statuses == [0, 0] and all(np.array_equal(o.cpu().numpy(), _file_decode("rgb", True)[1][names.index(n)]) for n, o in zip(picked, outs))
    statuses, _ = handle.to_pixels(images, fmt="yuv_planar", transforms=transforms)
    assert statuses == [UNSUPPORTED, UNSUPPORTED]


# ---------------------------------------------------------------- 6. refusals
def _raw_to_pixels(h, entries, stream=None):
    """entries: [(CoefficientInfo, CoefficientPlanes, output tensor [H, W, 3], pitch)] -> (return code, statuses)"""
    import torch
    n = len(entries)
    I, P, O = (N.CoefficientInfo * n)(), (N.CoefficientPlanes * n)(), (N.Output * n)()
    for i, (ci, cp, out, pitch) in enumerate(entries):
        I[i], P[i] = ci, cp
        O[i].plane[0], O[i].pitch[0] = out.data_ptr(), pitch
    statuses = (ctypes.c_int * n)(*([-1] * n))
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    rc = N.load().hipjpegCoefficientsToPixelsBatch(h, I, P, n, O, N.OUTPUT_RGBI, N.FLAG_FANCY_UPSAMPLING, statuses, s)
    return rc, list(statuses)


def _entry(info, tensors, pitch_delta=0):
    import torch
    ci, cp = lowlevel._info_struct(info), N.CoefficientPlanes()
    for c, t in enumerate(tensors):
        cp.coef[c], cp.pitch_blocks[c] = t.data_ptr(), t.shape[1]
    out = torch.full((info["height"], info["width"], 3), PIXEL_SENTINEL, dtype=torch.uint8, device="cuda:0")
    return [ci, cp, out, out.stride(0) + pitch_delta]


def test_refusals(handle):
    import torch
    names = [n for n, _ in _batch()]
    good_a, good_b, victim = names.index("s17x13_420_base_q90"), names.index("h320x200_420_opt_q75"), names.index("s64x48_420_base_q90")
    want = _file_decode("rgb", True)[1]
    keep = []

    def fresh(i):
        t = _upload(_host()[i][1])
        keep.append(t)
        return _entry(_host()[i][0], t)

    cmyk_info, cmyk_coefs = lowlevel.decode_coefficients_host(T.golden_files("cmyk")[0][1])
    assert cmyk_info["num_components"] == 4
    cmyk = _upload(cmyk_coefs)
    entries = [fresh(good_a), _entry(cmyk_info, cmyk)]
    e = fresh(victim)
    e[0].blocks_w[0] += 1  # not what the geometry gives
    entries.append(e)
    e = fresh(victim)
    e[1].coef[1] += 2  # not 16-byte aligned
    entries.append(e)
    e = fresh(victim)
    e[1].pitch_blocks[2] = e[0].blocks_w[2] - 1
    entries.append(e)
    e = fresh(victim)
    e[0].h[1] = 5
    entries.append(e)
    e = fresh(victim)
    e[3] = 64 * 3 - 1  # a row does not fit
    entries.append(e)
    e = fresh(victim)
    e[1].coef[0] = None
    entries.append(e)
    e = fresh(victim)
    e[0].width = 65536
    entries.append(e)
    entries.append(fresh(good_b))
    rc, statuses = _raw_to_pixels(handle._h, entries)
    torch.cuda.synchronize()
    assert rc == 0
    assert statuses == [0, UNSUPPORTED] + [INVALID_ARGUMENT] * 7 + [0]
    for e, st in zip(entries, statuses):
        if st != 0:
            assert bool((e[2] == PIXEL_SENTINEL).all())  # a failing image writes nothing to its output
    assert np.array_equal(entries[0][2].cpu().numpy(), want[good_a]) and np.array_equal(entries[-1][2].cpu().numpy(), want[good_b])


def test_refused_while_a_submit_is_in_flight_on_the_handle():
    import torch
    names = [n for n, _ in _batch()]
    i = names.index("s64x48_420_base_q90")
    src = _batch()[i][1]
    tensors = _upload(_host()[i][1])
    entry = _entry(_host()[i][0], tensors)
    pixels = torch.zeros((64, 48, 3), dtype=torch.uint8, device="cuda:0")
    info = lowlevel.encode_coefficient_info(48, 64, "420", 90)
    planes = [torch.full((bh, bw, 8, 8), SENTINEL, dtype=torch.int16, device="cuda:0") for bh, bw in zip(info["blocks_h"], info["blocks_w"])]

    def from_pixels(h):
        I, E, P = (N.EncodeInput * 1)(), (N.EncodeParams * 1)(N.EncodeParams(90, N.CSS["420"], N.OUTPUT_RGBI, 0, 0, 0)), (N.CoefficientPlanes * 1)()
        I[0].plane[0], I[0].pitch[0], I[0].width, I[0].height = pixels.data_ptr(), pixels.stride(0), 48, 64
        for c, t in enumerate(planes):
            P[0].coef[c], P[0].pitch_blocks[c] = t.data_ptr(), t.shape[1]
        st = (ctypes.c_int * 1)(-1)
        return N.load().hipjpegPixelsToCoefficientsBatch(h, I, E, 1, P, st, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)), st[0]

    def check(h, in_flight, settle):
        in_flight()
        assert _raw_to_pixels(h, [entry])[0] == INVALID_ARGUMENT and from_pixels(h)[0] == INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert bool((entry[2] == PIXEL_SENTINEL).all()) and all(bool((t == SENTINEL).all()) for t in planes)
        settle()
        assert _raw_to_pixels(h, [entry]) == (0, [0]) and from_pixels(h) == (0, 0)
        torch.cuda.synchronize()
        assert np.array_equal(entry[2].cpu().numpy(), oracle.decode(src))
        assert not any(bool((t == SENTINEL).any()) for t in planes)
        entry[2].fill_(PIXEL_SENTINEL)
        for t in planes:
            t.fill_(SENTINEL)

    enc = lowlevel.BatchEncoder(device=0, num_threads=2, gpu_huffman=True)
    try:
        check(enc._h, lambda: enc.submit([torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda:0")], "420", 90), enc.wait)
    finally:
        enc.close()
    dec = lowlevel.BatchDecoder(device=0, num_threads=2)
    try:
        outs = dec.allocate_outputs([src])
        check(dec._h, lambda: dec.submit([src], outs), dec.wait)
    finally:
        dec.close()


# ---------------------------------------------------------------- 7. pixels to tensors
_PICTURES = [(1, 1, "444", 88), (17, 13, "420", 88), (50, 37, "gray", 88), (320, 200, "420", 88), (128, 128, "gray", 88), (2056, 8, "gray", 88),
             (129, 70, "411", 88), (70, 45, "410", 88), (33, 47, "440", 88), (64, 48, "422", 88),
             (17, 13, "420", 1), (17, 13, "420", 100), (320, 200, "420", 1), (320, 200, "420", 100)]


def _inputs(input_format):
    """(tensors, subsamplings, qualities) of the batch in one input format of the encoder"""
    import torch
    pictures = _PICTURES
    if input_format == "gray":
        pictures = [p for p in _PICTURES if p[2] == "gray"]
    if input_format == "yuv_planar":
        pictures = [(64, 48, "420", 88)]
    tensors = []
    for k, (w, h, sub, q) in enumerate(pictures):
        rgb = synth_image(w, h, seed=40 + k)
        if input_format == "rgb":
            a = rgb
        elif input_format == "bgr":
            a = rgb[:, :, ::-1]
        elif input_format == "rgb_planar":
            a = rgb.transpose(2, 0, 1)
        elif input_format == "bgr_planar":
            a = rgb[:, :, ::-1].transpose(2, 0, 1)
        elif input_format == "gray":
            a = rgb[:, :, 1]
        else:
            tensors.append([torch.from_numpy(np.ascontiguousarray(p)).to("cuda:0") for p in (rgb[:, :, 0], rgb[::2, ::2, 1], rgb[::2, ::2, 2])])
            continue
        tensors.append(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"))
    return tensors, [p[2] for p in pictures], [p[3] for p in pictures]


@pytest.mark.parametrize("input_format", ["rgb", "bgr", "rgb_planar", "bgr_planar", "gray", "yuv_planar"])
def test_pixels_to_tensors(handle, input_format):
    import torch
    tensors, subs, quals = _inputs(input_format)
    enc = lowlevel.BatchEncoder(device=0, num_threads=4)
    try:
        files = enc.encode(tensors, subs, quals, input_format)
    finally:
        enc.close()
    want = [lowlevel.decode_coefficients_host(f) for f in files]
    outs = [[torch.full((bh, bw + 3, 8, 8), SENTINEL, dtype=torch.int16, device="cuda:0") for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
            for info, _ in want]
    statuses, images = handle.from_pixels(tensors, subs, quals, input_format, outs=outs)
    torch.cuda.synchronize()
    assert statuses == [0] * len(tensors)
    assert handle.stats()["moved_blocks"] == sum(c.shape[0] * c.shape[1] for _, coefs in want for c in coefs)
    for k, (im, (info, coefs)) in enumerate(zip(images, want)):
        assert {a: v for a, v in im.info.items() if a != "qtables"} == {a: v for a, v in info.items() if a != "qtables"}, k
        assert all(np.array_equal(a, b) for a, b in zip(im.info["qtables"], info["qtables"])), k
        assert len(im.coefs) == len(coefs)
        for c, (t, ref) in enumerate(zip(im.coefs, coefs)):
            got = t.cpu().numpy()
            assert np.array_equal(got[:, : ref.shape[1]], ref), (k, c)
            assert (got[:, ref.shape[1]:] == SENTINEL).all(), (k, c)  # the padding keeps the sentinel
    # allocated by the call: the same tensors
    if input_format == "rgb":
        statuses, images = handle.from_pixels(tensors, subs, quals, input_format)
        torch.cuda.synchronize()
        assert statuses == [0] * len(tensors)
        assert all(np.array_equal(t.cpu().numpy(), ref) for im, (_, coefs) in zip(images, want) for t, ref in zip(im.coefs, coefs))


def test_pixels_to_tensors_failures_stay_alone(handle):
    import torch
    pixels = [torch.from_numpy(synth_image(17, 13, seed=60 + k)).to("cuda:0") for k in range(5)]
    enc = lowlevel.BatchEncoder(device=0, num_threads=2)
    try:
        files = enc.encode(pixels, "420", 88)
    finally:
        enc.close()
    info = lowlevel.encode_coefficient_info(17, 13, "420", 88)
    outs = [[torch.full((bh, bw, 8, 8), SENTINEL, dtype=torch.int16, device="cuda:0") for bh, bw in zip(info["blocks_h"], info["blocks_w"])] for _ in pixels]
    null_plane = list(outs[1])
    outs[1] = [null_plane[0], null_plane[1], None]
    # views two bytes into larger tensors: every stride is right, no pointer is 16-byte aligned
    big = [torch.full((bh * bw * 64 + 8,), SENTINEL, dtype=torch.int16, device="cuda:0") for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
    outs[3] = [b[1: 1 + bh * bw * 64].view(bh, bw, 8, 8) for b, bh, bw in zip(big, info["blocks_h"], info["blocks_w"])]
    statuses, images = handle.from_pixels(pixels, ["420", "420", "no_such", "420", "420"], 88, outs=outs)
    torch.cuda.synchronize()
    assert statuses == [0, INVALID_ARGUMENT, UNSUPPORTED, INVALID_ARGUMENT, 0]
    assert images[1] is None and images[2] is None and images[3] is None
    assert all(bool((t == SENTINEL).all()) for t in null_plane + outs[2] + big)  # a failing image writes nothing into its planes
    for k in (0, 4):
        assert all(np.array_equal(t.cpu().numpy(), ref) for t, ref in zip(images[k].coefs, lowlevel.decode_coefficients_host(files[k])[1]))


# ---------------------------------------------------------------- 8. round trip, nothing in between
def test_round_trip_on_one_stream(handle):
    import torch
    cases = [(320, 200, "420", 71), (50, 37, "gray", 72)]
    rgb = [synth_image(w, h, seed=s) for w, h, _, s in cases]
    want = [oracle.decode(oracle.encode(a, sub, 90)) for a, (_, _, sub, _) in zip(rgb, cases)]
    staged = [torch.from_numpy(a).pin_memory() for a in rgb]
    stream = torch.cuda.Stream(device=0)
    with torch.cuda.stream(stream):
        pixels = [t.to("cuda:0", non_blocking=True) for t in staged]
        statuses, images = handle.from_pixels(pixels, [c[2] for c in cases], 90, stream=stream)
        assert statuses == [0, 0]
        statuses, outs = handle.to_pixels(images, stream=stream)
        assert statuses == [0, 0]
    stream.synchronize()
    for o, ref, c in zip(outs, want, cases):
        assert np.array_equal(o.cpu().numpy(), ref), c
