"""Coefficient tensors on the device: hipjpegDecodeCoefficientsBatch (entropy decode, GPU or host pool -> coef_export_kernel -> the
caller's tensors) and hipjpegEncodeCoefficientsBatch (the caller's tensors -> coef_import_kernel -> entropy coder, GPU or host pool).
Whatever route an image takes, its tensors are the ones hipjpegDecodeCoefficientsHost fills and its file the one
hipjpegEncodeCoefficientsHost writes (tests/test_coefficients_host.py pins those against the oracle and the lossless transcode).

One mixed batch serves every test -- the unit-to-image map of both kernels is exercised by it: one block; real areas narrower than the
MCU-padded grid on both axes; units that end inside a component (320x200 4:2:0: luma has 1000 blocks, the fourth unit is part full);
several units and rounds (640x480); a component of exactly 256 blocks and one of 257; four components, 4:1:1 / 4:1:0 / 4:4:0 and
replicated layouts for the export; progressive and multi-scan sequential sources."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from helpers import sampling_goldens as SG
from helpers import sequential_scans as S
from helpers import transcode_cases as T
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 1
SENTINEL = -21846  # 0xAAAA
_GOLDENS = ["s1x1_gray_base_q90", "s8x8_420_base_q90", "s8x8_gray_prog_q50", "s8x8_444_base_q50", "s17x13_420_base_q90", "s50x37_420_base_q50",
            "s33x65_422_base_q90", "s3x5_420_base_q90", "s3x5_gray_base_q90", "s3x5_444_base_q90", "h320x200_420_opt_q75", "c1_640x480_444_base_q90",
            "s17x13_420_prog_q50", "s64x48_420_base_q90", "s50x37_gray_prog_q50"]


def _img(w, h, sub, seed, q=88, **kw):
    return oracle.encode(synth_image(w, h, seed=seed), sub, q, **kw)


@functools.lru_cache(maxsize=None)
def _batch():
    """[(name, file)]: every image decodes"""
    decode = dict(T.golden_files("decode"))
    files = [(n, decode[n]) for n in _GOLDENS]
    files += [("gray_128x128", _img(128, 128, "gray", 21)), ("gray_2056x8", _img(2056, 8, "gray", 22)),   # 256 and 257 blocks
              ("411_129x70", _img(129, 70, "411", 23)), ("410_70x45", _img(70, 45, "410", 24)), ("440_33x47", _img(33, 47, "440", 25)),
              ("rst2_40x40", _img(40, 40, "420", 26, restart_interval=2))]
    files.append(("multiscan_40x40", S.recode(_img(40, 40, "420", 27), [[0], [1], [2]])))
    files.append(("cmyk", T.golden_files("cmyk")[0][1]))
    files += [("sampling_" + e["name"], SG.jpeg(e)) for e in SG.ENTRIES
              if e["name"] in ("k22111122_83x61_adobe2", "y22cb11cr21_83x61", "y31c11_83x61_prog", "gray22_83x61_rst3")]
    assert len(files) == len(_GOLDENS) + 12
    return tuple(files)


@functools.lru_cache(maxsize=None)
def _host():
    """decode_coefficients_host of the batch: the reference, computed once and left alone"""
    return tuple(lowlevel.decode_coefficients_host(d) for _, d in _batch())


@functools.lru_cache(maxsize=None)
def _eligible():
    return tuple(i for i, (_, d) in enumerate(_batch()) if T.expected_eligible(d) == (True, True))


@functools.lru_cache(maxsize=None)
def _host_files(target):
    """encode_coefficients_host of every eligible image of the batch"""
    return {i: lowlevel.encode_coefficients_host(*_host()[i], **T.TARGETS[target]) for i in _eligible()}


def _make(gpu_huffman, gpu_restart=False):
    return lowlevel.BatchCoefficients(device=0, num_threads=8, gpu_huffman=gpu_huffman, gpu_restart=gpu_restart)


@pytest.fixture(scope="module")
def handles():
    """name -> handle: the host pool, the GPU entropy stages, and the GPU coder taking restart intervals as well"""
    h = {"host": _make(False), "gpu": _make(True), "gpu_restart": _make(True, True)}
    yield h
    for v in h.values():
        v.close()


def _filled(info, extra=0):
    import torch
    return [torch.full((bh, bw + extra, 8, 8), SENTINEL, dtype=torch.int16, device="cuda:0") for bh, bw in zip(info["blocks_h"], info["blocks_w"])]


def _upload(coefs, extra=0, fill=0):
    import torch
    out = []
    for c in coefs:
        t = torch.full((c.shape[0], c.shape[1] + extra, 8, 8), fill, dtype=torch.int16, device="cuda:0")
        t[:, : c.shape[1]] = torch.from_numpy(c).to("cuda:0")
        out.append(t)
    return out


# ---------------------------------------------------------------- 7. export
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("route", ["host", "gpu"])
def test_export(handles, route, extra):
    import torch
    whole = dict(_batch())["s64x48_420_base_q90"]
    truncated = whole[: len(whole) * 2 // 3]
    arithmetic = whole.replace(b"\xff\xc0", b"\xff\xc9", 1)  # SOF9: a frame type the decoder does not decode
    assert lowlevel.coefficient_info(truncated)["blocks_w"] == [8, 4, 4]
    bad_status = {}
    for name, data in (("truncated", truncated), ("arithmetic", arithmetic)):
        with pytest.raises(N.HipJpegError) as e:
            lowlevel.decode_coefficients_host(data)
        bad_status[name] = e.value.status
    assert bad_status == {"truncated": T.TRUNCATED, "arithmetic": T.UNSUPPORTED}
    sources = [d for _, d in _batch()]
    sources.insert(3, truncated)
    sources.insert(9, arithmetic)
    sources.append(truncated)
    bad = {3: T.TRUNCATED, 9: T.UNSUPPORTED, len(sources) - 1: T.TRUNCATED}
    outs = [None if bad.get(i) == T.UNSUPPORTED else _filled(lowlevel.coefficient_info(s), extra) for i, s in enumerate(sources)]
    statuses, images = handles[route].decode(sources, outs=outs)
    torch.cuda.synchronize()
    want = iter(_host())
    for i, (st, im) in enumerate(zip(statuses, images)):
        if i in bad:
            assert st == bad[i] and im is None, i
            if outs[i] is not None:
                assert all(bool((t == SENTINEL).all()) for t in outs[i]), i  # a failing image writes nothing into its planes
            continue
        info, coefs = next(want)
        assert st == 0, (i, st)
        assert {k: v for k, v in im.info.items() if k != "qtables"} == {k: v for k, v in info.items() if k != "qtables"}
        assert all(np.array_equal(a, b) for a, b in zip(im.info["qtables"], info["qtables"]))
        assert len(im.coefs) == len(coefs)
        for c, (t, ref) in enumerate(zip(im.coefs, coefs)):
            got = t.cpu().numpy()
            assert np.array_equal(got[:, : ref.shape[1]], ref), (i, c)
            assert (got[:, ref.shape[1]:] == SENTINEL).all(), (i, c)  # the padding keeps the sentinel
    stats = handles[route].stats()
    assert stats["moved_blocks"] == sum(c.shape[0] * c.shape[1] for _, coefs in _host() for c in coefs)
    if route == "gpu":
        assert stats["gpu_decoded_images"] > 0  # DC values from the compact plane
    else:
        assert stats["gpu_decoded_images"] == 0


def test_export_honours_the_hybrid_threshold():
    h = _make(True)
    try:
        h.set_hybrid_huffman_threshold(100 * 100)
        picked = [i for i, (n, _) in enumerate(_batch()) if n in ("s64x48_420_base_q90", "c1_640x480_444_base_q90", "s17x13_420_prog_q50")]
        statuses, images = h.decode([_batch()[i][1] for i in picked])
        assert statuses == [0, 0, 0] and h.stats()["gpu_decoded_images"] == 1
        for i, im in zip(picked, images):
            assert all(np.array_equal(t.cpu().numpy(), ref) for t, ref in zip(im.coefs, _host()[i][1]))
    finally:
        h.close()


# ---------------------------------------------------------------- 8. import
# (the restart flag concerns restart intervals only)
@pytest.mark.parametrize("route,target", [(r, t) for r in ("host", "gpu") for t in T.TARGETS] + [("gpu_restart", "annexk_rst3")])
def test_import(handles, route, target):
    picked = list(_eligible())
    assert len(picked) >= 20
    images = [(_host()[i][0], _upload(_host()[i][1])) for i in picked]
    statuses, files = handles[route].encode(images, **T.TARGETS[target])
    assert statuses == [0] * len(picked)
    wrong = [_batch()[i][0] for i, f in zip(picked, files) if f != _host_files(target)[i]]
    assert not wrong, wrong
    stats = handles[route].stats()
    assert stats["moved_blocks"] == sum(c.shape[0] * c.shape[1] for i in picked for c in _host()[i][1])
    if route == "host" or (route == "gpu" and target == "annexk_rst3"):
        assert stats["gpu_coded_images"] == 0
    else:
        assert stats["gpu_coded_images"] > 0


@pytest.mark.parametrize("route", ["host", "gpu"])
def test_import_range_guard(handles, route):
    picked = list(_eligible())
    names = [_batch()[i][0] for i in picked]
    ac, dc = names.index("h320x200_420_opt_q75"), names.index("c1_640x480_444_base_q90")
    coefs = [[c.copy() for c in _host()[i][1]] for i in picked]
    coefs[ac][0][-1, -1, 7, 7] = 1024   # an AC value in the last real block of the luma: the part-full unit
    coefs[dc][2][0, 0, 0, 0] = -1025    # a DC value in the first block of a chroma component
    images = [(_host()[i][0], _upload(c)) for i, c in zip(picked, coefs)]
    statuses, files = handles[route].encode(images, **T.TARGETS["optimized"])
    assert [k for k, s in enumerate(statuses) if s != 0] == sorted((ac, dc))
    assert statuses[ac] == T.UNSUPPORTED and statuses[dc] == T.UNSUPPORTED and files[ac] is None and files[dc] is None
    for k, i in enumerate(picked):
        if k not in (ac, dc):
            assert files[k] == _host_files("optimized")[i], names[k]
    # the same values where nobody reads: in the pitch padding
    padded = []
    for i in picked:
        t = _upload(_host()[i][1], extra=2)
        for x in t:
            x[:, -2:, 7, 7] = 1024
            x[:, -2:, 0, 0] = -1025
        padded.append((_host()[i][0], t))
    statuses, files = handles[route].encode(padded, **T.TARGETS["optimized"])
    assert statuses == [0] * len(picked)
    assert all(f == _host_files("optimized")[i] for f, i in zip(files, picked))


def test_python_surface_validates_tensors(handles):
    import torch
    info, coefs = _host()[_eligible()[0]]
    good = _upload(coefs)
    h = handles["host"]
    for bad in ([t.cpu() for t in good], [t.to(torch.int32) for t in good], [t.transpose(2, 3) for t in good], [t[:, :, :, :4] for t in good], good[:-1] if len(good) > 1 else []):
        with pytest.raises(TypeError):
            h.encode([(info, bad)])
    with pytest.raises(TypeError):
        h.decode([_batch()[_eligible()[0]][1]], outs=[[t.cpu() for t in good]])


# ---------------------------------------------------------------- 9. round trip on the device
@pytest.mark.parametrize("target", list(T.TARGETS))
def test_round_trip_on_the_device(handles, target):
    sources = [d for _, d in _batch()]
    t = lowlevel.BatchTranscoder(device=0, num_threads=8, gpu_huffman=True, gpu_restart=True)
    try:
        want_statuses, want = t.transcode(sources, **T.TARGETS[target])
    finally:
        t.close()
    h = handles["gpu_restart"]
    statuses, images = h.decode(sources)
    assert statuses == [0] * len(sources)
    statuses, files = h.encode(images, **T.TARGETS[target])  # the tensors never leave the device
    assert statuses == want_statuses
    assert sum(s == 0 for s in statuses) == len(_eligible()) and {s for s in statuses} == {0, T.UNSUPPORTED}
    wrong = [n for (n, _), a, b in zip(_batch(), files, want) if a != b]
    assert not wrong, wrong


# ---------------------------------------------------------------- 10. an edit on the device
def test_an_edit_on_the_device(handles):
    import torch
    picked = [i for i in _eligible() if _batch()[i][0] in ("s64x48_420_base_q90", "s50x37_gray_prog_q50", "h320x200_420_opt_q75")]
    assert len(picked) == 3
    stream = torch.cuda.Stream(device=0)
    h = handles["gpu"]
    statuses, images = h.decode([_batch()[i][1] for i in picked], stream=stream)
    assert statuses == [0, 0, 0]
    with torch.cuda.stream(stream):
        for im in images:
            im.coefs[0][..., 0, 0] += 1
    statuses, files = h.encode(images, optimized_huffman=True, stream=stream)
    assert statuses == [0, 0, 0]
    for i, f in zip(picked, files):
        got, tables = oracle.decode_coefficients(f)
        for c, ref in enumerate(_host()[i][1]):
            rh, rw = ref.shape[:2]
            edited = ref.reshape(rh, rw, 64).copy()
            if c == 0:
                edited[:, :, 0] += 1
            assert np.array_equal(got[c][:rh, :rw], edited), (i, c)
            assert np.array_equal(tables[c], _host()[i][0]["qtables"][c])


# ---------------------------------------------------------------- 11. busy handle
def test_refused_while_a_submit_is_in_flight_on_the_handle():
    """each call takes a decode page or the encode batch for itself"""
    import torch
    src = dict(_batch())["s64x48_420_base_q90"]
    info, coefs = lowlevel.decode_coefficients_host(src)
    a = np.frombuffer(src, dtype=np.uint8)
    ptrs, lens = (ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_size_t * 1)(a.size)
    tensors = _filled(info)
    P, I = (N.CoefficientPlanes * 1)(), (N.CoefficientInfo * 1)(lowlevel._info_struct(info))
    for c, t in enumerate(tensors):
        P[0].coef[c], P[0].pitch_blocks[c] = t.data_ptr(), t.shape[1]
    params, statuses = (N.TranscodeParams * 1)(), (ctypes.c_int * 1)()
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    want_pixels = oracle.decode(src)

    def check(handle, in_flight, settle):
        decode = lambda: N.load().hipjpegDecodeCoefficientsBatch(handle, ptrs, lens, 1, P, N.FLAG_GPU_HUFFMAN, statuses, stream)
        encode = lambda: N.load().hipjpegEncodeCoefficientsBatch(handle, I, P, params, 1, N.FLAG_GPU_HUFFMAN, statuses, stream)
        in_flight()
        assert decode() == INVALID_ARGUMENT and encode() == INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in tensors)
        settle()
        assert decode() == 0 and statuses[0] == 0
        torch.cuda.synchronize()
        assert all(np.array_equal(t.cpu().numpy(), ref) for t, ref in zip(tensors, coefs))
        assert encode() == 0 and statuses[0] == 0
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        assert N.load().hipjpegEncodeGetBitstream(handle, 0, ctypes.byref(p), ctypes.byref(n)) == 0
        assert ctypes.string_at(p, n.value) == lowlevel.transcode_host(src)
        for t in tensors:
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
        assert np.array_equal(outs[0].cpu().numpy(), want_pixels)
        # afterwards the handle still decodes pixels correctly
        again, st = dec.decode([src], gpu_huffman=True)
        assert list(st) == [0] and np.array_equal(again[0].cpu().numpy(), want_pixels)
    finally:
        dec.close()
