"""WHEN the device work of a stream-taking call runs: every call of nvimagecodec_amd.lowlevel with a `stream`, and the plugin's decoder and
encoder with a user stream, on a fresh non-blocking stream that a finite busy-wait keeps occupied (tests/helpers/stalled_stream.py).
The current stream stays the default one, so a call that ignored its `stream` argument is seen too.

  (P) producer        the input holds a decoy; the real input is copied over it on the stream, behind the stall; the result must be the
                      reference's for the real input (and differ from the reference's for the decoy)
  (W) no early write  a clone of the sentinel-filled output queued on the stream in front of the call must still be all sentinel
  (C) consumer        a clone of the output queued on the stream right behind the call, with only the stream waited for, must be the
                      reference's result

Expected values are the oracle's, the numpy models' and the goldens', never an unstalled run of the same call.  The table of calls
against checks is tests/helpers/stream_order_cases.py; tests/test_stream_order_census.py holds it against lowlevel.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import lossless_encode_model as M
from helpers import lossless_files as LF
from helpers import scaled_goldens as SG
from helpers import stalled_stream as SS
from helpers.geometry import upright
from helpers.stream_order_cases import CASES, EXEMPT, PLUGIN_CASES  # noqa: F401  (the table of this module)
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel as LL
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

BASE, PROG, RST, GRAY = "s64x48_420_base_q90", "s33x65_422_prog_q50", "r130x70_420_base_rst7", "s50x37_gray_base_q90"
LOSSLESS = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "manifest_lossless.json")))["lossless"]}
STALL_ENDED = "the stall ended before the point that relies on it: raise STALL_MS (tests/helpers/stalled_stream.py)"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    SS.calibrate()
    return torch


# ---------------------------------------------------------------------------------------------------------------- files and references
@functools.lru_cache(maxsize=None)
def _golden(name):
    with open(os.path.join(GOLDEN, "decode", name + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _picture(w, h, seed):
    return synth_image(w, h, seed=seed)


@functools.lru_cache(maxsize=None)
def _coded(w, h, seed, sub="420", quality=90, restart_interval=0):
    """the oracle's file of a synthetic picture"""
    return oracle.encode(_picture(w, h, seed), sub, quality, restart_interval)


@functools.lru_cache(maxsize=None)
def _rgb(jpeg):
    """oracle.decode, once per file, left unchanged"""
    a = oracle.decode(jpeg)
    a.setflags(write=False)
    return a


def _batches():
    """four small batches for the pipelined decoder; the second is all progressive (a per-page entropy stream)"""
    return ([_golden(BASE), _golden(RST), _golden(GRAY)], [_golden(PROG), _golden("s64x48_420_prog_q90")],
            [_coded(70, 45, 31, "444", 85), _golden("s64x48_444_base_q90")], [_coded(96, 80, 32, "420", 75), _golden(GRAY)])


def _lossless_golden(name):
    with open(os.path.join(GOLDEN, "lossless", name + ".jpg"), "rb") as f:
        return f.read()


def _up(torch, a):
    """a numpy array on the device (uint16 through its bits: torch.from_numpy has no uint16)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _sentinel_outputs(dec, jpegs, **kw):
    return SS.sentinel_like(dec.allocate_outputs(jpegs, "rgb", kw.get("transforms"), kw.get("scales")))


def _assert_pixels(snaps, jpegs, what):
    for k, (t, j) in enumerate(zip(snaps, jpegs)):
        assert np.array_equal(SS.host(t), _rgb(j)), (what, k)


def _overwrite(torch, stream, dst, src):
    """dst.copy_(src) queued on `stream` (tensors or lists of tensors)"""
    with torch.cuda.stream(stream):
        for d, s in zip(dst if isinstance(dst, (list, tuple)) else [dst], src if isinstance(src, (list, tuple)) else [src]):
            d.copy_(s)


# ---------------------------------------------------------------------------------------------------------------- BatchDecoder.decode
@pytest.mark.parametrize("route", ["plain", "transforms", "half"])
@pytest.mark.parametrize("gpu_huffman", [False, True])
def test_decode_writes_behind_the_stream_and_is_seen_by_it(torch_mod, gpu_huffman, route):
    torch = torch_mod
    names = [BASE, PROG, RST, GRAY]
    jpegs = [_golden(n) for n in names]
    kw, want = {}, [_rgb(j) for j in jpegs]
    if route == "transforms":  # a region and orientation 6: the geometry pass
        regions = [(3, 5, r.shape[1] - 2, r.shape[0] - 1) for r in want]
        kw["transforms"] = [(r, 6) for r in regions]
        want = [upright(a[r[1]:r[3], r[0]:r[2]], 6) for a, r in zip(want, regions)]
    elif route == "half":  # scale denominator 2: the scaled kernels, against libjpeg-turbo's hashes
        kw["scales"] = [2] * len(jpegs)
        assert [SG.jpeg(SG.by_name(n)) for n in names] == jpegs
        want = [SG.expected(SG.by_name(n), 2) for n in names]
        assert all(st == SG.SUCCESS for st, _ in want)
    dec = LL.BatchDecoder(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        outs = _sentinel_outputs(dec, jpegs, **kw)
        SS.ready()
        st = SS.stall(S)
        before = SS.snapshot(S, outs)
        assert st.still_running(), STALL_ENDED
        _, statuses = dec.decode(jpegs, outs=outs, stream=S, gpu_huffman=gpu_huffman, **kw)
        if not gpu_huffman:  # (with the GPU entropy stage the call waits for its verdicts, and so for the stall in front of them)
            assert st.still_running(), STALL_ENDED
        after = SS.snapshot(S, outs)
        S.synchronize()
        assert statuses == [0] * len(jpegs)
        assert (dec.stats()["gpu_entropy_images"] > 0) == gpu_huffman
        assert SS.all_sentinel(before), "(W) the outputs were written ahead of the caller's stream"
        for k, (t, w) in enumerate(zip(after, want)):
            if route == "half":
                assert SG.sha(SS.host(t)) == w[1], ("(C)", names[k])
            else:
                assert np.array_equal(SS.host(t), w), ("(C)", names[k])
    finally:
        dec.close()


def test_decode_twice_on_one_handle_behind_a_stall(torch_mod):
    """The second call rewrites the handle's one staging page: it must wait until the first call's copy and kernels, which sit behind the
    stall, have used it (DecodeBatch::reserve waits for done_event_)."""
    torch = torch_mod
    a, b = [_coded(160, 128, 33)], [_golden(BASE)]
    dec = LL.BatchDecoder(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        outs_a, outs_b = _sentinel_outputs(dec, a), _sentinel_outputs(dec, b)
        SS.ready()
        st = SS.stall(S)
        _, sa = dec.decode(a, outs=outs_a, stream=S)
        assert st.still_running(), STALL_ENDED  # the first call returned while nothing of it had run
        _, sb = dec.decode(b, outs=outs_b, stream=S)
        after = SS.snapshot(S, outs_a + outs_b)
        S.synchronize()
        assert sa == [0] and sb == [0]
        _assert_pixels(after, a + b, "two calls")
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------------------- BatchDecoder.submit
def test_submit_three_batches_behind_one_stall_then_reuse_a_page(torch_mod):
    torch = torch_mod
    batches = _batches()
    dec = LL.BatchDecoder(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        outs = [_sentinel_outputs(dec, b) for b in batches]
        SS.ready()
        st = SS.stall(S)
        before = SS.snapshot(S, outs[0] + outs[1] + outs[2])
        for b, o in zip(batches[:3], outs[:3]):
            dec.submit(b, o, stream=S)
        assert st.still_running(), "hipjpegDecodeBatchSubmit waited for the device (or: " + STALL_ENDED + ")"
        snaps = []
        for b, o in zip(batches[:3], outs[:3]):
            assert dec.wait() == [0] * len(b)  # final statuses
            snaps.append(SS.snapshot(S, o))
        # page 0 again, with another batch: the first batch's pixels are in their outputs (and snapshotted) and stay right
        dec.submit(batches[3], outs[3], stream=S)
        assert dec.wait() == [0] * len(batches[3])
        snaps.append(SS.snapshot(S, outs[3]))
        S.synchronize()
        assert SS.all_sentinel(before), "(W) outputs written ahead of the caller's stream"
        for k, (snap, b) in enumerate(zip(snaps, batches)):
            _assert_pixels(snap, b, "(C) batch %d" % k)
        _assert_pixels(outs[0], batches[0], "batch 0 after its page was reused")
    finally:
        dec.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_submit_on_two_user_streams(torch_mod, pinned):
    """Batch 1 on a stalled stream, batch 2 on an idle one: wait() settles the oldest first, and both are right.  pinned: the bitstreams
    lie in page-locked tensors, and the copy engine reads them where they lie (zero-copy input)."""
    torch = torch_mod
    batches = _batches()
    b1, b2 = batches[0], batches[2]  # three and two baseline files: every one takes the GPU entropy stage
    dec = LL.BatchDecoder(device=0, num_threads=2)
    try:
        S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1, o2 = _sentinel_outputs(dec, b1), _sentinel_outputs(dec, b2)
        in1, in2 = b1, b2
        if pinned:
            in1, in2 = [[torch.frombuffer(bytearray(j), dtype=torch.uint8).pin_memory() for j in b] for b in (b1, b2)]
        SS.ready()
        st = SS.stall(S1)
        before = SS.snapshot(S1, o1)
        dec.submit(in1, o1, stream=S1)
        zero1 = dec.stats()["zero_copy_images"]
        dec.submit(in2, o2, stream=S2)
        zero2 = dec.stats()["zero_copy_images"]
        assert st.still_running(), STALL_ENDED
        assert dec.wait() == [0] * len(b1)  # (a Wait for batch 2 would be refused: its size is another)
        a1 = SS.snapshot(S1, o1)
        assert dec.wait() == [0] * len(b2)
        a2 = SS.snapshot(S2, o2)
        S1.synchronize()
        S2.synchronize()
        assert (zero1, zero2) == ((len(b1), len(b2)) if pinned else (0, 0))
        assert SS.all_sentinel(before), "(W)"
        _assert_pixels(a1, b1, "(C) stalled stream")
        _assert_pixels(a2, b2, "(C) idle stream")
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------------------- BatchLosslessDecoder
_LOSSLESS_A = ("p16_ps1_pt0_c3", "p16_ps7_pt0_c1", "p8_ps1_pt0_c3")  # two 16-bit files and one 8-bit file
_LOSSLESS_B = ("p16_ps4_pt0_c3", "rst3_p8_ps2_c3")


def _lossless_outputs(torch, dec, names):
    outs = []
    for n in names:
        c = LOSSLESS[n]
        info = {"height": c["height"], "width": c["width"], "num_components": c["components"]}
        outs.append(dec.allocate(info, torch.uint16 if c["dtype"] == "uint16" else torch.uint8))
    return SS.sentinel_like(outs)


def _assert_lossless(snaps, names, what):
    for t, n in zip(snaps, names):
        got = SS.host(t)
        assert got.dtype == np.dtype(LOSSLESS[n]["dtype"]) and SG.sha(got) == LOSSLESS[n]["sha256"], (what, n)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_lossless_decode_writes_behind_the_stream_and_is_seen_by_it(torch_mod, gpu_entropy):
    torch = torch_mod
    files = [_lossless_golden(n) for n in _LOSSLESS_A]
    dec = LL.BatchLosslessDecoder(device=0, num_threads=2, gpu_entropy=gpu_entropy)
    try:
        S = torch.cuda.Stream()
        outs = _lossless_outputs(torch, dec, _LOSSLESS_A)
        SS.ready()
        st = SS.stall(S)
        before = SS.snapshot(S, outs)
        assert st.still_running(), STALL_ENDED
        statuses, _ = dec.decode(files, outs=outs, stream=S)
        if not gpu_entropy:  # (the GPU entropy stage waits once per batch, on the stream, for its verdicts)
            assert st.still_running(), STALL_ENDED
        after = SS.snapshot(S, outs)
        S.synchronize()
        assert statuses == [0] * len(files)
        assert (dec.stats()["gpu_images"] > 0) == gpu_entropy
        assert SS.all_sentinel(before), "(W)"
        _assert_lossless(after, _LOSSLESS_A, "(C)")
    finally:
        dec.close()


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_lossless_decode_twice_on_one_handle_behind_a_stall(torch_mod, gpu_entropy):
    torch = torch_mod
    dec = LL.BatchLosslessDecoder(device=0, num_threads=2, gpu_entropy=gpu_entropy)
    try:
        S = torch.cuda.Stream()
        outs_a, outs_b = _lossless_outputs(torch, dec, _LOSSLESS_A), _lossless_outputs(torch, dec, _LOSSLESS_B)
        SS.ready()
        st = SS.stall(S)
        assert st.still_running(), STALL_ENDED
        sa, _ = dec.decode([_lossless_golden(n) for n in _LOSSLESS_A], outs=outs_a, stream=S)
        if not gpu_entropy:
            assert st.still_running(), STALL_ENDED
        sb, _ = dec.decode([_lossless_golden(n) for n in _LOSSLESS_B], outs=outs_b, stream=S)
        after = SS.snapshot(S, outs_a + outs_b)
        S.synchronize()
        assert sa == [0] * 3 and sb == [0] * 2
        _assert_lossless(after, _LOSSLESS_A + _LOSSLESS_B, "two calls")
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------------------- BatchEncoder
_ENCODE = ((64, 48, "420", 0), (50, 37, "444", 0), (70, 45, "420", 2))  # (width, height, subsampling, restart interval)


def _encode_inputs(torch, input_format, seed):
    """-> (decoy tensors that the call is given, the real pictures on the device, the oracle's files of the real ones and of the decoys)"""
    real = [_picture(w, h, seed + k) for k, (w, h, _, _) in enumerate(_ENCODE)]
    decoy = [_picture(w, h, seed + 50 + k) for k, (w, h, _, _) in enumerate(_ENCODE)]
    shape = (lambda a: a.transpose(2, 0, 1)) if input_format == "rgb_planar" else (lambda a: a)
    want = [oracle.encode(a, sub, 90, rst) for a, (_, _, sub, rst) in zip(real, _ENCODE)]
    unwanted = [oracle.encode(a, sub, 90, rst) for a, (_, _, sub, rst) in zip(decoy, _ENCODE)]
    assert all(a != b for a, b in zip(want, unwanted))
    return [_up(torch, shape(a)) for a in decoy], [_up(torch, shape(a)) for a in real], want, unwanted


@pytest.mark.parametrize("input_format", ["rgb", "rgb_planar"])
@pytest.mark.parametrize("gpu_huffman", [False, True])
def test_encode_reads_behind_the_stream(torch_mod, gpu_huffman, input_format):
    torch = torch_mod
    enc = LL.BatchEncoder(device=0, num_threads=2, gpu_huffman=gpu_huffman, gpu_restart=True)
    try:
        S = torch.cuda.Stream()
        images, real, want, unwanted = _encode_inputs(torch, input_format, 60)
        SS.ready()
        st = SS.stall(S)
        _overwrite(torch, S, images, real)
        assert st.still_running(), STALL_ENDED
        files = enc.encode(images, [e[2] for e in _ENCODE], 90, input_format, [e[3] for e in _ENCODE], stream=S)
        assert (enc.stats()["gpu_entropy_images"] > 0) == gpu_huffman
        for k, (f, w, u) in enumerate(zip(files, want, unwanted)):
            assert f != u, "(P) image %d: the file of the decoy that lay in the input before the stream's copy" % k
            assert f == w, "(P) image %d" % k
    finally:
        enc.close()


@pytest.mark.parametrize("gpu_huffman", [False, True])
def test_encode_submit_three_pages_behind_one_stall_then_reuse_a_page(torch_mod, gpu_huffman):
    torch = torch_mod
    enc = LL.BatchEncoder(device=0, num_threads=2, gpu_huffman=gpu_huffman, gpu_restart=True)
    try:
        S = torch.cuda.Stream()
        sets = [_encode_inputs(torch, "rgb", 70 + 10 * k) for k in range(4)]
        SS.ready()
        st = SS.stall(S)
        for images, real, _, _ in sets:
            _overwrite(torch, S, images, real)
        for images, _, _, _ in sets[:3]:
            enc.submit(images, [e[2] for e in _ENCODE], 90, "rgb", [e[3] for e in _ENCODE], stream=S)
        assert st.still_running(), "hipjpegEncodeBatchSubmit did not return at once (or: " + STALL_ENDED + ")"
        got = [enc.wait()]  # (statuses, files): the files are read here, before the fourth Submit takes the page
        images = sets[3][0]
        enc.submit(images, [e[2] for e in _ENCODE], 90, "rgb", [e[3] for e in _ENCODE], stream=S)
        got += [enc.wait() for _ in range(3)]
        for k, ((statuses, files), (_, _, want, unwanted)) in enumerate(zip(got, sets)):
            assert statuses == [0] * len(_ENCODE), k
            for f, w, u in zip(files, want, unwanted):
                assert f != u, "(P) batch %d: the decoy's file" % k
                assert f == w, "(P) batch %d" % k
    finally:
        enc.close()


# ---------------------------------------------------------------------------------------------------------------- BatchLosslessEncoder
# (height, width, components, precision, predictor, planar)
_LOSSLESS_ENCODE = ((19, 23, 3, 16, 1, False), (10, 21, 3, 8, 4, True), (11, 17, 1, 16, 7, True), (13, 9, 3, 8, 1, False))


def _lossless_samples(seed):
    return [LF.random_samples(seed + k, h, w, n, p).astype(np.uint16 if p > 8 else np.uint8) for k, (h, w, n, p, _, _) in enumerate(_LOSSLESS_ENCODE)]


def test_lossless_encode_reads_behind_the_stream(torch_mod):
    torch = torch_mod
    real, decoy = _lossless_samples(90), _lossless_samples(190)
    want = [M.model_file(s, e[3], e[4]) for s, e in zip(real, _LOSSLESS_ENCODE)]
    unwanted = [M.model_file(s, e[3], e[4]) for s, e in zip(decoy, _LOSSLESS_ENCODE)]
    assert all(a != b for a, b in zip(want, unwanted))
    shape = [(lambda a: a.transpose(2, 0, 1)) if e[5] else (lambda a: a) for e in _LOSSLESS_ENCODE]
    enc = LL.BatchLosslessEncoder(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        images = [_up(torch, f(a)) for f, a in zip(shape, decoy)]
        real_dev = [_up(torch, f(a)) for f, a in zip(shape, real)]
        SS.ready()
        st = SS.stall(S)
        _overwrite(torch, S, images, real_dev)
        assert st.still_running(), STALL_ENDED
        statuses, files = enc.encode(images, [e[3] for e in _LOSSLESS_ENCODE], [e[4] for e in _LOSSLESS_ENCODE], planar=[e[5] for e in _LOSSLESS_ENCODE],
                                     stream=S)
        assert statuses == [0] * len(images)
        for k, (f, w, u) in enumerate(zip(files, want, unwanted)):
            assert f != u, "(P) image %d: the decoy's file" % k
            assert f == w, "(P) image %d" % k
    finally:
        enc.close()


def test_lossless_encode_reads_a_padded_input_behind_the_stream(torch_mod):
    """The same at an odd pitch and offset: uint16 interleaved, 3 bytes of padding per row, the plane 1 byte into its buffer."""
    torch = torch_mod
    real, decoy = _lossless_samples(90)[0], _lossless_samples(190)[0]
    want, unwanted = M.model_file(real, 16, 1), M.model_file(decoy, 16, 1)
    assert want != unwanted
    x, n, real_bufs = M.padded_input(N, real, False, 3, 1)
    _, _, decoy_bufs = M.padded_input(N, decoy, False, 3, 1)
    enc = LL.BatchLosslessEncoder(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        padded, padded_real = [_up(torch, b) for b in decoy_bufs], [_up(torch, b) for b in real_bufs]
        for k, t in enumerate(padded):
            x.plane[k] = t.data_ptr() + 1
        SS.ready()
        st = SS.stall(S)
        _overwrite(torch, S, padded, padded_real)
        assert st.still_running(), STALL_ENDED
        X, P = (N.LosslessEncodeInput * 1)(x), (N.LosslessEncodeParams * 1)(N.LosslessEncodeParams(16, 1, 0, 0, n))
        statuses, files = enc._encode(X, P, 1, S)
        assert statuses == [0] and files[0] != unwanted, "(P) the decoy's file"
        assert files[0] == want, "(P)"
    finally:
        enc.close()


# ---------------------------------------------------------------------------------------------------------------- BatchCoefficients
def _oracle_coefficients(jpeg, info):
    """oracle.decode_coefficients cut to the real block area, [blocks_h, blocks_w, 8, 8]"""
    return [np.ascontiguousarray(c[:bh, :bw]).reshape(bh, bw, 8, 8) for c, bh, bw in zip(oracle.decode_coefficients(jpeg)[0], info["blocks_h"], info["blocks_w"])]


def test_coefficients_decode_writes_behind_the_stream_and_is_seen_by_it(torch_mod):
    torch = torch_mod
    jpegs = [_golden(BASE), _golden("s17x13_420_prog_q50"), _coded(70, 45, 34, "444", 85, 3)]
    infos = [LL.coefficient_info(j) for j in jpegs]
    want = [_oracle_coefficients(j, i) for j, i in zip(jpegs, infos)]
    bc = LL.BatchCoefficients(device=0, num_threads=2, gpu_huffman=True, gpu_restart=True)
    try:
        S = torch.cuda.Stream()
        outs = [SS.sentinel_like(bc.allocate(i)) for i in infos]
        flat = [t for o in outs for t in o]
        SS.ready()
        st = SS.stall(S)
        before = SS.snapshot(S, flat)
        assert st.still_running(), STALL_ENDED
        statuses, _ = bc.decode(jpegs, stream=S, outs=outs)
        after = SS.snapshot(S, flat)
        S.synchronize()
        assert statuses == [0] * len(jpegs)
        assert SS.all_sentinel(before), "(W)"
        for t, w in zip(after, [c for ws in want for c in ws]):
            assert np.array_equal(SS.host(t), w), "(C)"
    finally:
        bc.close()


def _coefficient_pair(torch):
    """One geometry, two pictures: (info, the real file, the decoy's file, tensors holding the decoy, the real coefficients on the device)"""
    real, decoy = _coded(64, 48, 35), _coded(64, 48, 36)
    assert real != decoy
    info = LL.coefficient_info(real)
    assert [np.array_equal(a, b) for a, b in zip(info["qtables"], LL.coefficient_info(decoy)["qtables"])] == [True] * 3
    tensors = [_up(torch, c) for c in _oracle_coefficients(decoy, info)]
    return info, real, decoy, tensors, [_up(torch, c) for c in _oracle_coefficients(real, info)]


def test_coefficients_encode_reads_behind_the_stream(torch_mod):
    """tests/test_gpu_coefficients.py::test_an_edit_on_the_device with a stall in front of the edit: now it can fail."""
    torch = torch_mod
    bc = LL.BatchCoefficients(device=0, num_threads=2, gpu_huffman=True)
    try:
        S = torch.cuda.Stream()
        info, real, decoy, tensors, real_dev = _coefficient_pair(torch)
        SS.ready()
        st = SS.stall(S)
        _overwrite(torch, S, tensors, real_dev)
        assert st.still_running(), STALL_ENDED
        statuses, files = bc.encode([(info, tensors)], stream=S)
        assert statuses == [0] and files[0] != decoy, "(P) the decoy's file"
        assert files[0] == real, "(P)"
    finally:
        bc.close()


def test_coefficients_to_pixels_in_stream_order(torch_mod):
    torch = torch_mod
    bc = LL.BatchCoefficients(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        info, real, decoy, tensors, real_dev = _coefficient_pair(torch)
        assert not np.array_equal(_rgb(real), _rgb(decoy))
        outs = [SS.sentinel_like(torch.empty((48, 64, 3), dtype=torch.uint8, device="cuda:0"))]
        SS.ready()
        st = SS.stall(S)
        before = SS.snapshot(S, outs)
        _overwrite(torch, S, tensors, real_dev)
        statuses, _ = bc.to_pixels([(info, tensors)], outs=outs, stream=S)
        assert st.still_running(), "hipjpegCoefficientsToPixelsBatch blocked (or: " + STALL_ENDED + ")"
        after = SS.snapshot(S, outs)
        S.synchronize()
        assert statuses == [0]
        assert SS.all_sentinel(before), "(W)"
        assert not np.array_equal(SS.host(after[0]), _rgb(decoy)), "(P) the decoy's pixels"
        assert np.array_equal(SS.host(after[0]), _rgb(real)), "(P, C)"
    finally:
        bc.close()


def test_pixels_to_coefficients_in_stream_order(torch_mod):
    torch = torch_mod
    bc = LL.BatchCoefficients(device=0, num_threads=2)
    try:
        S = torch.cuda.Stream()
        real, decoy = _picture(50, 37, 37), _picture(50, 37, 38)
        info = LL.encode_coefficient_info(50, 37, "420", 90)
        want = _oracle_coefficients(oracle.encode(real, "420", 90), info)
        unwanted = _oracle_coefficients(oracle.encode(decoy, "420", 90), info)
        assert not np.array_equal(want[0], unwanted[0])
        image, real_dev = _up(torch, decoy), _up(torch, real)
        outs = SS.sentinel_like(bc.allocate(info))
        SS.ready()
        st = SS.stall(S)
        before = SS.snapshot(S, outs)
        _overwrite(torch, S, image, real_dev)
        statuses, _ = bc.from_pixels([image], "420", 90, outs=[outs], stream=S)
        assert st.still_running(), "hipjpegPixelsToCoefficientsBatch blocked (or: " + STALL_ENDED + ")"
        after = SS.snapshot(S, outs)
        S.synchronize()
        assert statuses == [0]
        assert SS.all_sentinel(before), "(W)"
        for c, (t, w, u) in enumerate(zip(after, want, unwanted)):
            assert not np.array_equal(SS.host(t), u), ("(P) the decoy's coefficients", c)
            assert np.array_equal(SS.host(t), w), ("(P, C)", c)
    finally:
        bc.close()


# ---------------------------------------------------------------------------------------------------------------- BatchTranscoder
def test_transcode_on_a_stalled_stream(torch_mod):
    """A blocking call: the files are final when it returns, and so the stall in front of its work has ended."""
    torch = torch_mod
    jpegs = [_golden(BASE), _golden(PROG), _coded(70, 45, 39, "444", 85)]
    want = [LL.transcode_host(j, optimized_huffman=True) for j in jpegs]
    tr = LL.BatchTranscoder(device=0, num_threads=2, gpu_huffman=True)
    try:
        S = torch.cuda.Stream()
        SS.ready()
        st = SS.stall(S)
        assert st.still_running(), STALL_ENDED
        statuses, files = tr.transcode(jpegs, optimized_huffman=True, stream=S)
        assert not st.still_running(), "hipjpegTranscodeBatch returned before its stream had run"
        assert statuses == [0] * len(jpegs) and files == want
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------- the plugin's C API
def _plugin_decode(lib, inst, dec, data, out, h, w, fmt, channels, sample_type, color_spec, stream):
    """nvimgcodecDecoderDecode of one code stream into the device tensor `out`, with image_info.cuda_stream = stream -> processing status"""
    from nvimagecodec_amd import abi as A
    arr = np.frombuffer(data, dtype=np.uint8)
    cs = C.c_void_p()
    assert lib.nvimgcodecCodeStreamCreateFromHostMem(inst, C.byref(cs), arr.ctypes.data, arr.size) == 0
    pitch = out.stride(0) * out.element_size()
    info = A.init(A.ImageInfo, A.ST_IMAGE_INFO, sample_format=fmt, color_spec=color_spec, num_planes=1, buffer=out.data_ptr(),
                  buffer_size=pitch * h, buffer_kind=A.BUFFER_KIND_STRIDED_DEVICE, cuda_stream=stream)
    pi = info.plane_info[0]
    pi.width, pi.height, pi.row_stride, pi.num_channels, pi.sample_type = w, h, pitch, channels, sample_type
    im = C.c_void_p()
    assert lib.nvimgcodecImageCreate(inst, C.byref(im), C.byref(info)) == 0
    dp = A.init(A.DecodeParams, A.ST_DECODE_PARAMS)
    fut = C.c_void_p()
    assert lib.nvimgcodecDecoderDecode(dec, (C.c_void_p * 1)(cs), (C.c_void_p * 1)(im), 1, C.byref(dp), C.byref(fut)) == 0
    assert lib.nvimgcodecFutureWaitForAll(fut) == 0
    st, n = (C.c_uint32 * 1)(), C.c_size_t()
    lib.nvimgcodecFutureGetProcessingStatus(fut, st, C.byref(n))
    lib.nvimgcodecFutureDestroy(fut)
    lib.nvimgcodecImageDestroy(im)
    lib.nvimgcodecCodeStreamDestroy(cs)
    return st[0]


@pytest.mark.parametrize("kind", ["dct_host_entropy", "dct_gpu_entropy", "lossless_host_entropy", "lossless_gpu_entropy"])
def test_plugin_decoder_with_a_user_stream(torch_mod, kind):
    """BUFFER_KIND_STRIDED_DEVICE and image_info.cuda_stream = a stalled stream.  The plugin decodes on streams of its own (a job stream
    for DCT files, lossless_stream_ for lossless ones): they must start behind the user's stream (W), and the user's stream must wait for
    them (C).  With the host entropy stage nvimgcodecFutureWaitForAll returns while the stall runs -- asserted -- so the clone behind the
    call is queued while the decode has not begun, and only the plugin's hipStreamWaitEvent(user_stream, decoded) makes it see pixels.
    With a GPU entropy stage the plugin waits on the host for that stage's verdicts, and so for the stall: those cases carry (W) only."""
    from nvimagecodec_amd import abi as A
    from test_gpu_plugin import _setup
    torch = torch_mod
    lib = A.bind(N.load_host())
    returns_during_the_stall = kind.endswith("host_entropy")
    if kind.startswith("dct"):
        data = _golden(RST)
        want = _rgb(data)
        out = torch.empty(want.shape, dtype=torch.uint8, device="cuda:0")
        how = (70, 130, A.SAMPLEFORMAT_I_RGB, 3, A.SAMPLE_DATA_TYPE_UINT8, A.COLORSPEC_SRGB)
        options = b"hipjpeg_decoder:gpu_huffman=0" if returns_during_the_stall else b""
    else:
        c = LOSSLESS["p16_ps7_pt0_c1"]
        data = _lossless_golden(c["name"])
        out = torch.empty((c["height"], c["width"]), dtype=torch.uint16, device="cuda:0")
        how = (c["height"], c["width"], A.SAMPLEFORMAT_P_Y, 1, A.SAMPLE_DATA_TYPE_UINT16, A.COLORSPEC_UNCHANGED)
        options = b"" if returns_during_the_stall else b"hipjpeg_decoder:gpu_lossless_entropy=1"
    inst, dec = _setup(lib, options=options)
    try:
        side = torch.cuda.Stream()
        SS.sentinel_like(out)
        gpu_before = LL.plugin_lossless_entropy_stats()["gpu_images"]
        SS.ready()
        st = SS.stall(side)
        before = SS.snapshot(side, out)
        assert st.still_running(), STALL_ENDED
        status = _plugin_decode(lib, inst, dec, data, out, *how, stream=side.cuda_stream)
        if returns_during_the_stall:
            assert st.still_running(), "the plugin waited for the user's stream on the host (or: " + STALL_ENDED + ")"
        after = SS.snapshot(side, out)
        side.synchronize()
        assert status == A.PS_SUCCESS
        assert SS.all_sentinel(before), "(W) the plugin wrote the image before the user's stream had reached the decode"
        if kind.startswith("dct"):
            assert np.array_equal(SS.host(after), want), "(C)"
        else:
            assert LL.plugin_lossless_entropy_stats()["gpu_images"] == gpu_before + (0 if returns_during_the_stall else 1)
            assert SG.sha(SS.host(after)) == c["sha256"], "(C)"
    finally:
        lib.nvimgcodecDecoderDestroy(dec)
        lib.nvimgcodecInstanceDestroy(inst)


@pytest.mark.parametrize("kind", ["baseline", "lossless"])
def test_plugin_encoder_reads_behind_the_user_stream(torch_mod, kind):
    from nvimagecodec_amd import abi as A
    from test_gpu_lossless_encode import _plugin_encode
    torch = torch_mod
    if kind == "baseline":
        real, decoy = _picture(64, 48, 40), _picture(64, 48, 41)
        want, unwanted = oracle.encode(real, "444", 90), oracle.encode(decoy, "444", 90)  # (_plugin_encode: quality 90, SAMPLING_444)
        encoding = A.JPEG_ENCODING_BASELINE_DCT
    else:
        real, decoy = [LF.random_samples(s, 19, 23, 3, 16).astype(np.uint16) for s in (42, 43)]
        want, unwanted = M.model_file(real, 16, 1), M.model_file(decoy, 16, 1)
        encoding = A.JPEG_ENCODING_LOSSLESS_HUFFMAN
    assert want != unwanted
    from nvimagecodec_amd import api
    side = torch.cuda.Stream()
    image, real_dev = _up(torch, decoy), _up(torch, real)
    with api.Encoder(max_num_cpu_threads=2) as enc:  # (made in front of the stall: its streams and threads are not part of the call)
        SS.ready()
        st = SS.stall(side)
        _overwrite(torch, side, image, real_dev)
        assert st.still_running(), STALL_ENDED
        status, data = _plugin_encode(torch, real, A.SAMPLEFORMAT_I_RGB, encoding, dev=image, stream=side.cuda_stream, encoder=enc)
    assert status == A.PS_SUCCESS and data != unwanted, "(P) the decoy's file"
    assert data == want, "(P)"
