"""GPU: every kernel family on arenas that are NOT zero.  The handles of this file are created with tests/helpers/poisoned_memory.py's
allocators (hipjpegSetAllocators; the plugin's execution parameters): every device -- and, in the second configuration, every pinned --
allocation is filled with one byte before the library sees it, and refill() fills the device arenas again between two batches of one
handle.  docs/arena_regions.md is the audit this file checks: no kernel reads a byte of an arena that its own batch did not write.

Expected values come from the references the repository has apart from the kernels -- the libjpeg-turbo goldens and their manifests, the
oracle, the numpy model of the lossless decoder, the host routes (host entropy stages, host coder, transcode_host) -- never from a run of
the same kernels over clean memory.  Everything is exact equality.  A failure at fill 0x00 alone is the harness's; at 0x5A or 0xFF a
kernel read what nobody wrote (or a fill of the planner covers too little): the audit's table names the region and its readers.

Counters are asserted beside the bytes (gpu_entropy_images, interval_images, host_fallbacks, gpu_images, gpu_coded_images ...), as the
lists' own tests assert them: poison must not pass by quietly sending an image to the host stage.

Every test ends (fixture `poison`) with calls >= 1 -- the allocators were really used -- and, its handles closed, all_freed()."""
import contextlib
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case, load_encode_case
from helpers import coder_seams as CS
from helpers import lossless_entropy_cases as EC
from helpers import lossless_files as LF
from helpers import progressive_restart_files as P
from helpers import progressive_seams as PS
from helpers import sampling_goldens as SG
from helpers import scaled_goldens as SC
from helpers import sequential_scans as Q
from helpers import steered_streams as S
from helpers import transcode_cases as T
from helpers.geometry import upright
from helpers.poisoned_memory import PoisonAllocators
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

# (fill, pinned allocator too): the control first, so that `-x` stops at the harness before it stops at the product
CONFIGS = [(0x00, False), (0x00, True), (0x5A, False), (0x5A, True), (0xFF, False), (0xFF, True)]

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _M = json.load(_f)
with open(os.path.join(GOLDEN, "manifest_plain.json")) as _f:
    _PLAIN = {e["name"]: e["plain_rgb_sha256"] for e in json.load(_f)["decode"]}
with open(os.path.join(GOLDEN, "manifest_cmyk.json")) as _f:
    _CMYK = json.load(_f)["cmyk"]
with open(os.path.join(GOLDEN, "manifest_encode_prog.json")) as _f:
    _ENC_PROG = json.load(_f)["encode_progressive"]
with open(os.path.join(GOLDEN, "manifest_encode_extreme.json")) as _f:
    _ENC_EXTREME = json.load(_f)["encode_extreme"]
_LOSSLESS = json.load(open(os.path.join(GOLDEN, "manifest_lossless.json")))["lossless"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=CONFIGS, ids=["fill_%02x_%s" % (b, "device_pinned" if p else "device") for b, p in CONFIGS])
def poison(request, torch):
    a = PoisonAllocators(*request.param)
    yield a
    assert a.calls >= 1 and a.device_calls >= 1, "the allocators were never used"
    assert a.pinned_calls >= 1 or not a.pinned
    assert a.all_freed(), (a.live, a.live_pinned, a.errors)


@contextlib.contextmanager
def _open(cls, poison, **kw):
    """a fresh handle of `cls` on the poisoned allocators, closed on the way out (every allocation goes back then)"""
    h = cls(device=0, allocators=poison, **kw)
    try:
        yield h
    finally:
        h.close()


# ================================================================================================================ decode
@functools.lru_cache(maxsize=None)
def _oracle_rgb(jpeg, fancy):
    a = oracle.decode(jpeg, oracle.FMT_RGB, fancy=fancy)
    a.setflags(write=False)
    return a


def _decode_matrix(torch, dec, jpegs, check, stages=(False, True), counts=None, **kw):
    """Both entropy stages x fancy on / off x rgb / rgb_planar.  check(i, status, H x W x 3 array or None, fancy) judges image i;
    counts(stats, gpu_huffman) the counters of a batch."""
    for gh in stages:
        for fancy in (True, False):
            for fmt in ("rgb", "rgb_planar"):
                outs, st = dec.decode(jpegs, fmt=fmt, fancy=fancy, gpu_huffman=gh, check=False, **kw)
                torch.cuda.synchronize()
                assert dec.host_fallbacks() == 0, (gh, fancy, fmt)
                if counts is not None:
                    counts(dec.stats(), gh)
                bad = []
                for i, (o, s) in enumerate(zip(outs, st)):
                    got = None if s != 0 else o.cpu().numpy()
                    if got is not None and fmt == "rgb_planar":
                        got = got.transpose(1, 2, 0)
                    if not check(i, int(s), got, fancy):
                        bad.append(i)
                assert not bad, ("gpu_huffman" if gh else "host entropy", "fancy" if fancy else "plain", fmt, bad)


def _oracle_check(jpegs):
    return lambda i, s, got, fancy: s == 0 and np.array_equal(got, _oracle_rgb(jpegs[i], fancy))


def test_decode_goldens_in_one_batch(torch, poison):
    """tests/golden/decode: libjpeg-turbo's pixels by hash (manifest.json, fancy; manifest_plain.json, plain), the counter of
    tests/test_gpu_huffman.py"""
    entries = _M["decode"]
    jpegs = [load_decode_case(e)[0] for e in entries]
    on_gpu = sum(1 for e in entries if not (e["progressive"] and "_rst" in e["name"]))

    def check(i, s, got, fancy):
        return s == 0 and _sha(got) == (entries[i]["rgb_sha256"] if fancy else _PLAIN[entries[i]["name"]])

    def counts(stats, gh):
        assert stats["gpu_entropy_images"] == (on_gpu if gh else 0)

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, check, counts=counts)


def test_decode_sampling_goldens(torch, poison):
    """helpers/sampling_goldens.py with the refused layouts, as tests/test_gpu_sampling_layouts.py::test_mixed_batch: the oracle's pixels
    (pinned to libjpeg-turbo by tests/test_sampling_layouts.py), and exactly the declined set the restatement of libjpeg's upsampler gives"""
    from test_gpu_sampling_layouts import _expected
    entries = list(SG.ENTRIES) + [dict(e, refused=True) for e in SG.REFUSED]
    jpegs = [SG.jpeg(e) for e in entries]

    def check(i, s, got, fancy):
        e = entries[i]
        if e.get("refused"):
            return s != 0
        if SG.expected_unsupported(e, "rgb", fancy):
            return s == 3
        return s == 0 and np.array_equal(got, _expected(jpegs[i], e, "rgb", fancy))

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, check)


def test_decode_cmyk_goldens(torch, poison):
    """tests/golden/cmyk: the reference's CMYK -> RGB formula on libjpeg-turbo's samples (fancy: the stored samples, as tests/test_cmyk.py;
    plain: the oracle's, pinned by manifest_plain.json there)"""
    from test_cmyk import _load, _reference_rgb
    cases = [_load(e) for e in _CMYK]
    jpegs = [c[0] for c in cases]

    def check(i, s, got, fancy):
        want = _reference_rgb(cases[i][1], _CMYK[i]["kind"] != "plain") if fancy else _oracle_rgb(jpegs[i], False)
        return s == 0 and np.array_equal(got, want)

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, check)


@pytest.mark.parametrize("denom", SC.DENOMS)
def test_decode_scaled_goldens(torch, poison, denom):
    """helpers/scaled_goldens.py: libjpeg-turbo's scaled pictures by hash, its refusals as UNSUPPORTED -- but BAD_JPEG for the two layouts
    that never pass the header parser (tests/test_gpu_scaled_decode.py _PARSER_REFUSES)"""
    from test_gpu_scaled_decode import _PARSER_REFUSES
    jpegs = [SC.jpeg(e) for e in SC.FILES]

    def check(i, s, got, fancy):
        status, sha = SC.expected(SC.FILES[i], denom, False, fancy)
        status = _PARSER_REFUSES.get(SC.FILES[i]["name"], status)
        return s == status and (status != 0 or _sha(got) == sha)

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, check, scales=[denom] * len(jpegs))


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_decode_steered_streams(torch, poison, name):
    """helpers/steered_streams.py: a placed byte on every seam of the destuff, walk and block kernels; all on the GPU stage, none handed
    back (helpers/steered_streams.py decode_on_device)"""
    files = S.family(name)
    jpegs = [w.jpeg for w in files]

    def counts(stats, gh):
        assert stats["gpu_entropy_images"] == (len(files) if gh else 0)

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, _oracle_check(jpegs), counts=counts)
        S.decode_on_device(dec, files)  # (fmt "y" against the writer's own pixels)


def test_decode_progressive_seams(torch, poison):
    """helpers/progressive_seams.py as tests/test_gpu_progressive_seams.py: the walk's seams and rings; the files over the limits keep the
    host entropy stage and are not counted.  The two files with ten-block MCUs have no interleaved RGB: to planes."""
    planes_only = [n for n in sorted(PS.CASES) if "mcu_of_10" in n]
    names = [n for n in sorted(PS.CASES) if n not in planes_only]
    cases = [PS.get(n) for n in names]
    jpegs = [c.jpeg for c in cases]
    assert sum(not c.in_limit for c in cases) == 4

    def counts(stats, gh):
        assert stats["gpu_entropy_images"] == (sum(c.in_limit for c in cases) if gh else 0)

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, _oracle_check(jpegs), counts=counts)
        for gh in (False, True):
            outs, st = dec.decode([PS.get(n).jpeg for n in planes_only], fmt="yuv_planar", gpu_huffman=gh, check=False)
            torch.cuda.synchronize()
            assert list(st) == [0, 0] and dec.stats()["gpu_entropy_images"] == (2 if gh else 0) and dec.host_fallbacks() == 0
            for n, o in zip(planes_only, outs):
                for a, b in zip(o, oracle.decode_planes(PS.get(n).jpeg)):
                    assert np.array_equal(a.cpu().numpy(), b), n


@functools.lru_cache(maxsize=None)
def _interval_files():
    """every input of tests/test_gpu_progressive_intervals.py the interval kernels take"""
    files = [load_decode_case(e)[0] for e in _M["decode"] if e["progressive"] and "_rst" in e["name"]]
    files += [j for _, j in P.pillow_files()]
    files += [j for _, j in P.transcode_products(GOLDEN)]
    files += [P.helper_file(n)[0] for n in sorted(P.HELPER_CASES)]
    return tuple(files)


def test_decode_progressive_restart_files_on_the_interval_kernels(torch, poison):
    """helpers/progressive_restart_files.py with HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS, counters as
    tests/test_gpu_progressive_intervals.py::test_mixed_batch_takes_the_interval_kernels; the file with different intervals stays on the
    host entropy stage"""
    jpegs = list(_interval_files()) + [P.helper_file(P.DIFFERENT_INTERVALS)[0]]
    n_interval = len(jpegs) - 1
    assert n_interval == 4 + 27 + 12 + len(P.HELPER_CASES)

    def counts(stats, gh):
        assert stats["interval_images"] == (n_interval if gh else 0) and stats["gpu_entropy_images"] == (n_interval if gh else 0)
        assert stats["interval_takeovers"] == 0

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, _oracle_check(jpegs), counts=counts, gpu_progressive_intervals=True)


@functools.lru_cache(maxsize=None)
def _multiscan():
    """(golden entry, re-coded file): every scan script of tests/test_gpu_multiscan_sequential.py over the sequential colour goldens"""
    from test_gpu_multiscan_sequential import SCRIPTS
    out = []
    for e in _M["decode"]:
        if e["progressive"] or e["sub"] == "gray" or not e["pixels"]:
            continue
        src = load_decode_case(e)[0]
        out += [(e, Q.recode(src, script)) for script in SCRIPTS]
    return tuple(out)


def test_decode_multiscan_sequential_files(torch, poison):
    """helpers/sequential_scans.py: the colour goldens re-coded into one scan per component and the other scripts -- the one-component
    scans are where the planner's padding fills apply.  Pixels: the SOURCE golden's libjpeg-turbo hashes (re-coding changes no
    coefficient); every file on the GPU stage (tests/test_gpu_multiscan_sequential.py)."""
    rec = _multiscan()
    jpegs = [j for _, j in rec]

    def check(i, s, got, fancy):
        e = rec[i][0]
        return s == 0 and _sha(got) == (e["rgb_sha256"] if fancy else _PLAIN[e["name"]])

    def counts(stats, gh):
        assert stats["gpu_entropy_images"] == (len(rec) if gh else 0)

    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, check, counts=counts)


_GEOMETRY = [(641, 481, "422", 85), (333, 200, "444", 75), (200, 300, "gray", 90), (77, 50, "411", 80), (130, 70, "420", 90)]


@functools.lru_cache(maxsize=None)
def _geometry_batch():
    """as tests/test_gpu_geometry.py::test_all_orientations_and_regions_interleaved, on its small pictures"""
    jpegs, transforms, expect = [], [], []
    for k, (w, h, sub, q) in enumerate(_GEOMETRY):
        j = oracle.encode(synth_image(w, h, seed=40 + k), sub, q)
        full = oracle.decode(j)
        for orientation in range(1, 9):
            roi = None if orientation % 2 else (w // 5, h // 7, w - w // 3, h - h // 9)
            jpegs.append(j)
            transforms.append((roi, orientation))
            expect.append(upright(full if roi is None else full[roi[1]:roi[3], roi[0]:roi[2]], orientation))
    return jpegs, transforms, expect


def test_decode_regions_and_orientations_and_fast_idct(torch, poison):
    """The geometry pass (its staging planes live in planes_), and once HIPJPEG_FLAG_FAST_IDCT against libjpeg-turbo's IFAST hashes
    (manifest_fast_idct.json)"""
    jpegs, transforms, expect = _geometry_batch()
    with open(os.path.join(GOLDEN, "manifest_fast_idct.json")) as f:
        ifast = json.load(f)["decode"]
    by_name = {e["name"]: e for e in _M["decode"]}
    ifast_jpegs = [load_decode_case(by_name[e["name"]])[0] for e in ifast]
    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        for gh in (False, True):
            outs, st = dec.decode(jpegs, fmt="rgb", gpu_huffman=gh, transforms=transforms)
            torch.cuda.synchronize()
            assert all(s == 0 for s in st) and dec.host_fallbacks() == 0
            assert dec.stats()["gpu_entropy_images"] == (len(jpegs) if gh else 0)
            for o, e, t in zip(outs, expect, transforms):
                assert tuple(o.shape) == e.shape and np.array_equal(o.cpu().numpy(), e), (gh, t)
            outs, st = dec.decode(ifast_jpegs, fmt="rgb", gpu_huffman=gh, fast_idct=True)
            torch.cuda.synchronize()
            assert dec.host_fallbacks() == 0
            bad = [e["name"] for e, o in zip(ifast, outs) if _sha(o.cpu().numpy()) != e["rgb_sha256"]]
            assert not bad, (gh, bad)


# ================================================================================================================ padding fills
@functools.lru_cache(maxsize=None)
def _padding_batch():
    """Non-interleaved 4:2:0 pictures whose luma grids have padding (17 x 13: 3 x 2 real blocks in a 4 x 2 grid; 33 x 47: 5 x 6 in 6 x 6):
    four equal ones in a row and three more behind a picture of another size -- evenly spaced fills, which merge_zero_fills() folds into
    2D fills -- then the other size again and an interleaved picture: single fills.  (lengths of the runs: 4, 1, 3, 1; the interleaved
    picture has no fill)"""
    a = Q.recode(oracle.encode(synth_image(17, 13, seed=1), "420", 90), [[0], [1], [2]])
    b = Q.recode(oracle.encode(synth_image(33, 47, seed=2), "420", 90), [[0], [1], [2]])
    inter = oracle.encode(synth_image(33, 47, seed=3), "420", 90)
    return (a, a, a, a, b, a, a, a, b, inter)


def test_padding_fills_of_non_interleaved_scans(torch, poison):
    """The padding blocks lie outside the picture: no pixel shows them.  What a fill that covers too little -- or lands on a neighbour --
    can reach: the coefficient tensors (over the real block area; the padding itself is not part of any tensor, see
    docs/arena_regions.md), the transcoded files, the pixels.  Against the host entropy decoder's coefficients, transcode_host's
    files and the oracle's pixels."""
    jpegs = list(_padding_batch())
    want_coefs = [lowlevel.decode_coefficients_host(j) for j in jpegs]
    with _open(lowlevel.BatchCoefficients, poison, num_threads=4, gpu_huffman=True) as bc:
        statuses, images = bc.decode(jpegs)
        torch.cuda.synchronize()
        assert list(statuses) == [0] * len(jpegs) and bc.stats()["gpu_decoded_images"] == len(jpegs)
        for i, (im, (info, coefs)) in enumerate(zip(images, want_coefs)):
            assert len(im.coefs) == len(coefs)
            for c, (t, ref) in enumerate(zip(im.coefs, coefs)):
                assert np.array_equal(t.cpu().numpy(), ref), (i, c)
    with _open(lowlevel.BatchTranscoder, poison, num_threads=4, gpu_huffman=True) as t:
        for kw in (T.TARGETS["optimized"], T.TARGETS["progressive"]):
            statuses, files = t.transcode(jpegs, **kw)
            assert list(statuses) == [0] * len(jpegs) and t.stats()["gpu_decoded_images"] == len(jpegs)
            assert files == [lowlevel.transcode_host(j, **kw) for j in jpegs], kw
    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        _decode_matrix(torch, dec, jpegs, _oracle_check(jpegs), stages=(True,))


# ================================================================================================================ lossless
@functools.lru_cache(maxsize=None)
def _lossless_seams():
    return tuple((name, f, LF.model_decode(d, 16, 1, 0, rr)) for name, f, d, rr in EC.seam_cases(lowlevel.lossless_entropy_shape()))


@functools.lru_cache(maxsize=None)
def _lossless_ordinary():
    out = []
    for seed, (h, w, n, ps) in enumerate(((40, 90, 1, 1), (70, 33, 3, 6))):
        d = np.random.default_rng(seed + 1).integers(0, 65536, size=(h, w, n))
        out.append((LF.write_differences(d, 16, ps, table=LF.FLAT), LF.model_decode(d, 16, ps)))
    return tuple(out)


@pytest.mark.parametrize("gpu_entropy", [False, True], ids=["host_entropy", "gpu_entropy"])
def test_lossless(torch, poison, gpu_entropy):
    """tests/golden/lossless by libjpeg-turbo's hashes; helpers/lossless_entropy_cases.py: every seam file (interleaved and planar) against
    the numpy model, the stream that cannot synchronise and the damaged files between good ones with the statuses and guard frames of
    tests/test_gpu_lossless_entropy.py"""
    from test_gpu_lossless_entropy import arena_outputs, check_frame
    seams, ordinary = _lossless_seams(), _lossless_ordinary()
    files = [open(os.path.join(GOLDEN, "lossless", c["name"] + ".jpg"), "rb").read() for c in _LOSSLESS]

    def decode_all(d, fs, **kw):
        statuses, outs = d.decode(fs, **kw)
        torch.cuda.synchronize()
        return statuses, [None if o is None else o.cpu().numpy() for o in outs]

    with _open(lowlevel.BatchLosslessDecoder, poison, num_threads=4, gpu_entropy=gpu_entropy) as d:
        statuses, outs = decode_all(d, files)
        assert statuses == [0] * len(files)
        for c, o in zip(_LOSSLESS, outs):
            assert _sha(o if c["dtype"] == "uint16" else (o & 0xFF).astype(np.uint8)) == c["sha256"], c["name"]
        stats = d.stats()
        assert stats["gpu_images"] == (len(files) if gpu_entropy else 0) and stats["host_fallback_images"] == 0
        for planar in (False, True):
            statuses, outs = decode_all(d, [f for _, f, _ in seams], planar=planar)
            assert statuses == [0] * len(seams)
            for (name, f, want), got in zip(seams, outs):
                assert np.array_equal(np.moveaxis(got, 0, 2) if planar else got, want), (name, planar)
            stats = d.stats()
            assert stats["gpu_images"] == (len(seams) if gpu_entropy else 0) and stats["host_fallback_images"] == 0
        # the stream whose walk cannot converge goes to the host stage alone
        f, diffs = EC.unsynchronisable(lowlevel.lossless_entropy_shape())
        statuses, outs = decode_all(d, [ordinary[0][0], f, ordinary[1][0]])
        assert statuses == [0, 0, 0]
        assert np.array_equal(outs[0], ordinary[0][1]) and np.array_equal(outs[2], ordinary[1][1])
        assert np.array_equal(outs[1], LF.model_decode(diffs, 8, 1))
        stats = d.stats()
        assert (stats["host_fallback_images"], stats["gpu_images"]) == ((1, 2) if gpu_entropy else (0, 0))
        # each damaged file fails alone, with the host decoder's status, and writes nothing
        (good_a, want_a), (good_b, want_b) = ordinary
        for name, bad in EC.bad_cases():
            try:
                lowlevel.decode_lossless_host(bad)
                want_status = 0
            except N.HipJpegError as e:
                want_status = e.status
            info = lowlevel.lossless_info(bad)
            shape_of = np.zeros((info["height"], info["width"], info["num_components"]), dtype=np.uint16)
            raws, frames = arena_outputs(torch, [want_a, shape_of, want_b], 3, False)
            statuses, _ = d.decode([good_a, bad, good_b], raw_outputs=raws)
            torch.cuda.synchronize()
            assert statuses == [0, want_status, 0], (name, statuses)
            for k, want in ((0, want_a), (2, want_b)):
                bufs, h, row_bytes, pitch = frames[k]
                check_frame(bufs[0], h, row_bytes, pitch, 3, [np.ascontiguousarray(r).view(np.uint8) for r in want.reshape(h, -1)])
            if want_status != 0:
                bufs, h, row_bytes, pitch = frames[1]
                check_frame(bufs[0], h, row_bytes, pitch, 3, None)


# ================================================================================================================ encode
@functools.lru_cache(maxsize=None)
def _encode_goldens(gray):
    """(entry, input, libjpeg-turbo's file, the oracle's coefficients) of tests/golden/encode"""
    out = []
    for e in _M["encode"]:
        if (e["sub"] == "gray") != gray:
            continue
        rgb, jpeg = load_encode_case(e)
        src = np.repeat(rgb[:, :, :1], 3, axis=2) if gray else rgb  # (a gray picture goes in as one plane: channel 0, as tests/test_gpu_encode.py)
        out.append((e, rgb, jpeg, oracle.forward(src, e["sub"], e["quality"])[0]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _host_coded(gray, k, **kw):
    e, rgb, _, coefs = _encode_goldens(gray)[k]
    return lowlevel.encode_from_coefficients_host(e["width"], e["height"], coefs, e["sub"], e["quality"], **kw)


def _feed(torch, images, gray):
    return [torch.from_numpy(np.ascontiguousarray(im[:, :, 0] if gray else im)).cuda() for im in images]


def test_encode_goldens_on_every_route_of_the_gpu_coder(torch, poison):
    """tests/golden/encode: baseline output is the oracle's file and carries libjpeg-turbo's scan bytes (tests/test_gpu_encode.py);
    optimized tables, restart intervals, progressive output and progressive output with restart intervals are the host coder's files for
    the oracle's coefficients.  All coded on the device."""
    routes = [dict(), dict(optimized_huffman=True), dict(restart_interval=3), dict(restart_interval=1, optimized_huffman=True),
              dict(progressive=True), dict(progressive=True, restart_interval=2)]
    with _open(lowlevel.BatchEncoder, poison, num_threads=4, gpu_huffman=True, gpu_restart=True, gpu_progressive_restart=True) as enc:
        for gray in (False, True):
            cases = _encode_goldens(gray)
            feed = _feed(torch, [c[1] for c in cases], gray)
            for kw in routes:
                out = enc.encode(feed, subsampling=[c[0]["sub"] for c in cases], quality=[c[0]["quality"] for c in cases],
                                 input_format="gray" if gray else "rgb", **kw)
                assert enc.stats()["gpu_entropy_images"] == len(cases), kw
                for k, ((e, rgb, jpeg, _), got) in enumerate(zip(cases, out)):
                    if not kw:
                        src = np.repeat(rgb[:, :, :1], 3, axis=2) if gray else rgb
                        assert got == oracle.encode(src, e["sub"], e["quality"]), e["name"]
                        assert oracle.scan_bytes(got) == oracle.scan_bytes(jpeg), e["name"]
                    assert got == _host_coded(gray, k, **kw), (e["name"], kw)


def test_encode_progressive_goldens(torch, poison):
    """manifest_encode_prog.json: libjpeg-turbo's progressive files, with and without restart intervals, byte for byte"""
    with _open(lowlevel.BatchEncoder, poison, num_threads=4, gpu_huffman=True, gpu_restart=True, gpu_progressive_restart=True) as enc:
        for rst in sorted({e["restart"] for e in _ENC_PROG}):
            for gray in (False, True):
                entries = [e for e in _ENC_PROG if e["restart"] == rst and (e["sub"] == "gray") == gray]
                if not entries:
                    continue
                images = [np.fromfile(os.path.join(GOLDEN, e["input"]), dtype=np.uint8).reshape(e["height"], e["width"], 3) for e in entries]
                out = enc.encode(_feed(torch, images, gray), subsampling=[e["sub"] for e in entries], quality=[e["quality"] for e in entries],
                                 input_format="gray" if gray else "rgb", restart_interval=rst, progressive=True)
                assert enc.stats()["gpu_entropy_images"] == len(entries), (rst, gray)
                for e, got in zip(entries, out):
                    with open(os.path.join(GOLDEN, "encode_prog", e["name"] + ".jpg"), "rb") as f:
                        assert got == f.read(), e["name"]


@functools.lru_cache(maxsize=None)
def _extreme_cases(gray):
    """(entry, input, the oracle's file, libjpeg-turbo's scan bytes or None) of manifest_encode_extreme.json.  The manifest's gray files
    were made from the colour pictures by the library's own conversion; the encoder takes a gray picture as one plane, so the gray
    entries go in as their first channel and have the oracle's file alone."""
    from helpers.extreme_images import extreme_image
    out = []
    for e in _ENC_EXTREME:
        if (e["sub"] == "gray") != gray:
            continue
        rgb = extreme_image(e["pattern"], e["width"], e["height"], e["seed"])
        src = np.repeat(rgb[:, :, :1], 3, axis=2) if gray else rgb
        with open(os.path.join(GOLDEN, "encode_extreme", e["name"] + ".jpg"), "rb") as f:
            out.append((e, rgb, oracle.encode(src, e["sub"], e["quality"]), None if gray else oracle.scan_bytes(f.read())))
    return tuple(out)


def test_encode_extreme_goldens(torch, poison):
    """manifest_encode_extreme.json (saturated pixels, qualities 1 and 100): the oracle's files byte for byte, libjpeg-turbo's scan bytes"""
    with _open(lowlevel.BatchEncoder, poison, num_threads=4, gpu_huffman=True) as enc:
        for gray in (False, True):
            cases = _extreme_cases(gray)
            out = enc.encode(_feed(torch, [c[1] for c in cases], gray), subsampling=[c[0]["sub"] for c in cases],
                             quality=[c[0]["quality"] for c in cases], input_format="gray" if gray else "rgb")
            assert enc.stats()["gpu_entropy_images"] == len(cases)
            bad = [e["name"] for (e, _, want, scan), got in zip(cases, out) if got != want or (scan is not None and oracle.scan_bytes(got) != scan)]
            assert not bad, bad


@functools.lru_cache(maxsize=None)
def _coder_reference():
    """name -> (case, the host coder's file): built once, left alone"""
    return {c.name: (c, CS.view(c).file) for c in list(CS.cases()) + [c for b in CS.batches() for c in b.cases]}


def test_encode_coder_seams(torch, poison):
    """helpers/coder_seams.py: every case of the census in one launch per flavour, as listed and reversed, and the two batches with more
    files than the layout kernel has lanes -- the host coder's files byte for byte, all coded on the device"""
    ref = _coder_reference()
    with _open(lowlevel.BatchCoefficients, poison, num_threads=8, gpu_huffman=True, gpu_restart=True, gpu_progressive_restart=True) as h:
        def same(cases, what):
            per = {k: [c.params[k] for c in cases] for k in ("optimized_huffman", "progressive", "restart_interval")}
            statuses, files = h.encode([(c.info, [torch.from_numpy(a).to("cuda:0") for a in c.coefs]) for c in cases], **per)
            assert statuses == [0] * len(cases), what
            assert h.stats()["gpu_coded_images"] == len(cases), what
            wrong = [c.name for c, f in zip(cases, files) if f != ref[c.name][1]]
            assert not wrong, what + ": " + " ".join(wrong)

        for progressive in (False, True):
            cases = [c for c in CS.cases() if c.params["progressive"] == progressive]
            same(cases, "as listed")
            same(cases[::-1], "reversed")
        for b in CS.batches()[1:]:
            same(list(b.cases), "more files than layout lanes")


# ================================================================================================================ transcode, tensors
def _host_transcode(data, **kw):
    try:
        return 0, lowlevel.transcode_host(data, **kw)
    except N.HipJpegError as e:
        return e.status, None


@functools.lru_cache(maxsize=None)
def _transcode_expectations():
    sources = tuple(d for _, d in T.golden_files("decode"))
    turn = dict(optimized_huffman=True, orientation=6, trim=True)
    crop = dict(optimized_huffman=True, region=(16, 16, 48, 40), expand=True)
    return sources, ((turn, tuple(_host_transcode(d, **turn) for d in sources)), (crop, tuple(_host_transcode(d, **crop) for d in sources)))


def test_transcode_turned_and_cropped(torch, poison):
    """helpers/transcode_cases.py's golden files at orientation 6 with trim and at one crop: statuses and files of transcode_host"""
    sources, runs = _transcode_expectations()
    with _open(lowlevel.BatchTranscoder, poison, num_threads=8, gpu_huffman=True, gpu_restart=True) as t:
        for kw, want in runs:
            assert any(st == 0 for st, _ in want)
            statuses, files = t.transcode(list(sources), **kw)
            assert list(statuses) == [st for st, _ in want], kw
            bad = [i for i, (a, (_, b)) in enumerate(zip(files, want)) if a != b]
            assert not bad, (kw, bad)
            assert t.stats()["gpu_decoded_images"] > 0 and t.stats()["gpu_coded_images"] == sum(st == 0 for st, _ in want)


@functools.lru_cache(maxsize=None)
def _tensor_goldens():
    """(file, host coefficients) of the decode goldens the tensor route takes: up to three components"""
    out = []
    for e in _M["decode"]:
        j = load_decode_case(e)[0]
        out.append((j, lowlevel.decode_coefficients_host(j)))
    return tuple(out)


def test_coefficient_tensors_and_back_to_pixels(torch, poison):
    """BatchCoefficients: the decode goldens exported (the host entropy stage's coefficients), then to_pixels of those tensors (the
    oracle's pixels, fancy and plain)"""
    cases = _tensor_goldens()
    jpegs = [j for j, _ in cases]
    with _open(lowlevel.BatchCoefficients, poison, num_threads=4, gpu_huffman=True) as bc:
        statuses, images = bc.decode(jpegs)
        torch.cuda.synchronize()
        assert list(statuses) == [0] * len(jpegs) and bc.stats()["gpu_decoded_images"] > 0
        for i, (im, (_, (info, coefs))) in enumerate(zip(images, cases)):
            assert len(im.coefs) == len(coefs)
            assert all(np.array_equal(t.cpu().numpy(), ref) for t, ref in zip(im.coefs, coefs)), i
        for fancy in (True, False):
            statuses, outs = bc.to_pixels(images, fancy=fancy)
            torch.cuda.synchronize()
            assert list(statuses) == [0] * len(jpegs)
            bad = [i for i, o in enumerate(outs) if not np.array_equal(o.cpu().numpy(), _oracle_rgb(jpegs[i], fancy))]
            assert not bad, (fancy, bad)


# ================================================================================================================ across batches
@functools.lru_cache(maxsize=None)
def _busy_jpeg():
    """640 x 480 at 4:4:4 (the geometry of the largest small golden, c1_640x480_444_base_q90) with every coefficient +-1023: the
    longest codes, the fullest arenas -- what tests/test_gpu_coefficient_pixels.py::test_stale_arena leaves behind, as a file"""
    from helpers import jpeg_from_coefficients as J
    rng = np.random.default_rng(11)
    sampling = [(1, 1)] * 3
    coefs = [np.where(rng.integers(0, 2, size=(bh, bw, 64)) == 1, 1023, -1023).astype(np.int32) for bh, bw in J.block_grid(640, 480, sampling)]
    for c in coefs:
        c[..., 0] = np.where(np.indices(c.shape[:2]).sum(axis=0) % 2 == 0, 1023, -1023)  # differences of +-2046: eleven bits
    return J.write_baseline(640, 480, sampling, coefs, [np.ones(64, dtype=np.int32)] * 3)


_SMALL_NAMES = ["s17x13_420_base_q90", "s3x5_420_base_q90", "s50x37_420_base_q50", "s33x65_422_prog_q50", "s64x48_444_base_q90", "s17x13_gray_base_q90",
                "r130x70_420_base_rst7"]


def _small_decode_lists():
    by_name = {e["name"]: e for e in _M["decode"]}
    goldens = [load_decode_case(by_name[n])[0] for n in _SMALL_NAMES]
    return [goldens, list(_padding_batch()), [w.jpeg for w in S.family("seams")[:8]]]


def test_decode_handle_across_batches(torch, poison):
    """One BatchDecoder: a busy batch, refill() on the idle handle, the small lists; then the small lists first and the busy batch
    behind them without a refill, and the small lists once more over what it left.  (docs/arena_regions.md: no buffer of a decode
    handle carries data from one batch to the next, so refill() is legitimate here.)"""
    busy = _busy_jpeg()
    lists = _small_decode_lists()
    with _open(lowlevel.BatchDecoder, poison, num_threads=4) as dec:
        def run_busy():
            # (sixty-three coefficients of ten bits per block: the walks of such a stream run out of their round budget and the host
            # decoder takes the picture over -- after every kernel of the stage has filled its share of the arenas, which is the point)
            outs, st = dec.decode([busy], gpu_huffman=True)
            torch.cuda.synchronize()
            assert list(st) == [0] and dec.stats()["gpu_entropy_images"] == 1
            assert np.array_equal(outs[0].cpu().numpy(), _oracle_rgb(busy, True))

        def run_small():
            for jpegs in lists:
                _decode_matrix(torch, dec, jpegs, _oracle_check(jpegs))

        run_busy()
        poison.refill()
        run_small()
        run_busy()
        run_small()


def test_encode_handle_across_batches(torch, poison):
    """One BatchEncoder: a noisy picture larger than any that follows, refill(), the encode goldens on three routes; then again behind
    the busy batch without the refill.  (No buffer of an encode handle carries data between batches either.)"""
    noise = np.random.default_rng(5).integers(0, 256, size=(768, 1024, 3), dtype=np.uint8)
    want_noise = oracle.encode(noise, "444", 100)
    routes = [dict(), dict(optimized_huffman=True), dict(progressive=True, restart_interval=2)]
    cases = _encode_goldens(False)
    with _open(lowlevel.BatchEncoder, poison, num_threads=4, gpu_huffman=True, gpu_restart=True, gpu_progressive_restart=True) as enc:
        def run_busy():
            out = enc.encode([torch.from_numpy(noise).cuda()], subsampling="444", quality=100)
            assert enc.stats()["gpu_entropy_images"] == 1 and out[0] == want_noise

        def run_small():
            feed = _feed(torch, [c[1] for c in cases], False)
            for kw in routes:
                out = enc.encode(feed, subsampling=[c[0]["sub"] for c in cases], quality=[c[0]["quality"] for c in cases], **kw)
                assert enc.stats()["gpu_entropy_images"] == len(cases), kw
                bad = [c[0]["name"] for k, (c, got) in enumerate(zip(cases, out)) if got != _host_coded(False, k, **kw)]
                assert not bad, (kw, bad)

        run_busy()
        torch.cuda.synchronize()
        poison.refill()
        run_small()
        run_busy()
        run_small()


def test_lossless_and_tensor_handles_across_batches(torch, poison):
    """BatchLosslessDecoder (GPU entropy stage) and BatchCoefficients, each: a large batch, refill(), small ones; the large one again, the
    small ones without a refill"""
    big_d = np.random.default_rng(9).integers(0, 65536, size=(300, 500, 3))
    big = (LF.write_differences(big_d, 16, 4, table=LF.FLAT), LF.model_decode(big_d, 16, 4))
    seams = _lossless_seams()[:12]
    with _open(lowlevel.BatchLosslessDecoder, poison, num_threads=4, gpu_entropy=True) as d:
        def run(files, wants):
            statuses, outs = d.decode(files)
            torch.cuda.synchronize()
            assert statuses == [0] * len(files) and d.stats()["gpu_images"] == len(files) and d.stats()["host_fallback_images"] == 0
            for k, (o, w) in enumerate(zip(outs, wants)):
                assert np.array_equal(o.cpu().numpy(), w), k

        run([big[0]], [big[1]])
        poison.refill()
        run([f for _, f, _ in seams], [w for _, _, w in seams])
        run([big[0]], [big[1]])
        run([f for _, f, _ in seams], [w for _, _, w in seams])
    busy = _busy_jpeg()
    small = _small_decode_lists()[0] + list(_padding_batch())
    with _open(lowlevel.BatchCoefficients, poison, num_threads=4, gpu_huffman=True, gpu_restart=True) as bc:
        def run_files(jpegs):
            statuses, images = bc.decode(jpegs)
            torch.cuda.synchronize()
            assert list(statuses) == [0] * len(jpegs) and bc.stats()["gpu_decoded_images"] == len(jpegs)
            for j, im in zip(jpegs, images):
                _, coefs = lowlevel.decode_coefficients_host(j)
                assert all(np.array_equal(t.cpu().numpy(), ref) for t, ref in zip(im.coefs, coefs))
            statuses, outs = bc.to_pixels(images)
            torch.cuda.synchronize()
            assert all(np.array_equal(o.cpu().numpy(), _oracle_rgb(j, True)) for j, o in zip(jpegs, outs))
            eligible = [i for i, j in enumerate(jpegs) if T.expected_eligible(j) == (True, True)]
            statuses, files = bc.encode([images[i] for i in eligible], optimized_huffman=True)
            assert list(statuses) == [0] * len(eligible)
            assert files == [lowlevel.transcode_host(jpegs[i], optimized_huffman=True) for i in eligible]

        run_files([busy])
        poison.refill()
        run_files(small)
        run_files([busy])
        run_files(small)


# ================================================================================================================ the plugin's routes
def test_plugin_decoder_and_encoder(torch, poison):
    """nvimgcodecDecoderCreate / nvimgcodecEncoderCreate with the poison allocators in the execution parameters: one decode call that
    mixes DCT and lossless samples (hipjpeg_decoder:gpu_lossless_entropy=1) and one encode call per kind of output"""
    from nvimagecodec_amd import abi as A
    from nvimagecodec_amd import api
    from nvimagecodec_amd.api import _api, _check
    from test_gpu_lossless import noise_file, plugin_decode_batch
    C = ctypes
    da, pa = poison.plugin_allocators()
    ep = A.init(A.ExecutionParams, A.ST_EXECUTION_PARAMS, device_id=0, max_num_cpu_threads=2)
    ep.device_allocator = C.pointer(da)
    if pa is not None:
        ep.pinned_allocator = C.pointer(pa)
    lib = A.bind(N.load_host())
    ci = A.init(A.InstanceCreateInfo, A.ST_INSTANCE_CREATE_INFO, load_builtin_modules=1, load_extension_modules=1)
    inst = C.c_void_p()
    assert lib.nvimgcodecInstanceCreate(C.byref(inst), C.byref(ci)) == 0
    try:
        dec = C.c_void_p()
        assert lib.nvimgcodecDecoderCreate(inst, C.byref(dec), C.byref(ep), b"hipjpeg_decoder:gpu_lossless_entropy=1") == 0
        by_name = {e["name"]: e for e in _M["decode"]}
        (dct_a, want_a), (dct_b, want_b) = (load_decode_case(by_name[n]) for n in ("s64x48_420_base_q90", "s50x37_420_base_q90"))
        gray, want_gray = noise_file(71, 70, 90, 1, 4, precision=12)
        rgb, want_rgb = noise_file(72, 66, 70, 3, 1)
        U16, U8 = A.SAMPLE_DATA_TYPE_UINT16, A.SAMPLE_DATA_TYPE_UINT8
        outs = [torch.zeros(shape, dtype=dtype, device="cuda:0")
                for shape, dtype in (((48, 64, 3), torch.uint8), ((70, 90), torch.uint16), ((66, 70, 3), torch.uint16), ((37, 50, 3), torch.uint8))]
        before = lowlevel.plugin_lossless_entropy_stats()
        statuses = plugin_decode_batch(lib, dec, inst, [
            (dct_a, 48, 64, A.SAMPLEFORMAT_I_RGB, 1, 3, U8, outs[0].data_ptr(), 192, A.COLORSPEC_SRGB, None),
            (gray, 70, 90, A.SAMPLEFORMAT_P_Y, 1, 1, U16, outs[1].data_ptr(), 180, None, None),
            (rgb, 66, 70, A.SAMPLEFORMAT_I_UNCHANGED, 1, 3, U16, outs[2].data_ptr(), 420, None, None),
            (dct_b, 37, 50, A.SAMPLEFORMAT_I_RGB, 1, 3, U8, outs[3].data_ptr(), 150, A.COLORSPEC_SRGB, None)])
        torch.cuda.synchronize()
        assert statuses == [A.PS_SUCCESS] * 4
        after = lowlevel.plugin_lossless_entropy_stats()
        assert after["gpu_images"] - before["gpu_images"] == 2 and after["host_fallback_images"] == before["host_fallback_images"]
        assert np.array_equal(outs[0].cpu().numpy(), want_a) and np.array_equal(outs[3].cpu().numpy(), want_b)
        assert np.array_equal(outs[1].cpu().numpy(), want_gray[:, :, 0]) and np.array_equal(outs[2].cpu().numpy(), want_rgb)
        lib.nvimgcodecDecoderDestroy(dec)
    finally:
        lib.nvimgcodecInstanceDestroy(inst)
    # the encoder (GPU entropy coder: the plugin's default), through the Python marshalling of api.Encoder
    elib, einst = _api()
    enc = api.Encoder.__new__(api.Encoder)
    enc._torch, enc.device_id, enc._h = torch, 0, C.c_void_p()
    _check(elib.nvimgcodecEncoderCreate(einst, C.byref(enc._h), C.byref(ep), b""), "nvimgcodecEncoderCreate")
    try:
        imgs = [synth_image(w, h, seed=w) for (w, h) in ((64, 48), (131, 77), (320, 240))]
        dev = [torch.from_numpy(i).cuda() for i in imgs]
        coefs = [oracle.forward(im, "420", 90)[0] for im in imgs]
        jp = api.JpegEncodeParams
        for extra, kw in ((None, {}), (jp(optimized_huffman=True), dict(optimized_huffman=True)), (jp(progressive=True), dict(progressive=True))):
            params = api.EncodeParams(quality=90, chroma_subsampling=api.ChromaSubsampling.CSS_420, **({} if extra is None else {"jpeg_encode_params": extra}))
            out = enc.encode([api.as_image(d) for d in dev], "jpeg", params)
            want = [lowlevel.encode_from_coefficients_host(im.shape[1], im.shape[0], c, "420", 90, **kw) for im, c in zip(imgs, coefs)]
            assert out == want, kw
            if not kw:
                assert out == [oracle.encode(im, "420", 90) for im in imgs]
    finally:
        enc.close()


# ================================================================================================================ the entry point
def test_allocators_are_refused_after_the_first_batch(torch):
    """hipjpegSetAllocators: accepted on a fresh handle, INVALID_ARGUMENT once a batch of any kind has allocated -- a buffer must go back
    to the allocator it came from"""
    first = PoisonAllocators(0x5A)
    jpeg = load_decode_case(next(e for e in _M["decode"] if e["name"] == "s17x13_420_base_q90"))[0]
    for cls, use in ((lowlevel.BatchDecoder, lambda h: h.decode([jpeg])),
                     (lowlevel.BatchEncoder, lambda h: h.encode([torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda:0")])),
                     (lowlevel.BatchTranscoder, lambda h: h.transcode([jpeg])),
                     (lowlevel.BatchCoefficients, lambda h: h.decode([jpeg])),
                     (lowlevel.BatchLosslessDecoder, lambda h: h.decode([_lossless_ordinary()[0][0]]))):
        h = cls(device=0, allocators=first)
        try:
            second = PoisonAllocators(0xFF, pinned=True)
            table = second.hipjpeg_allocators()
            assert N.load().hipjpegSetAllocators(h._h, ctypes.byref(table)) == 0  # still fresh: the second set replaces the first
            assert N.load().hipjpegSetAllocators(h._h, None) == 1
            calls = first.calls
            use(h)
            torch.cuda.synchronize()
            assert second.calls >= 1 and second.pinned_calls >= 1 and first.calls == calls, cls.__name__
            assert N.load().hipjpegSetAllocators(h._h, ctypes.byref(first.hipjpeg_allocators())) == 1, cls.__name__
        finally:
            h.close()
        assert second.all_freed() and first.all_freed(), cls.__name__
