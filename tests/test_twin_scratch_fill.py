"""The host twins of the GPU algorithms over scratch that is NOT zero, without a GPU.  On the device the twins' vectors are regions of
grow-only arenas that nobody clears (docs/arena_regions.md): a kernel may read only what a copy, a memset or a kernel of the same batch
wrote.  hipjpegTestSetScratchFill makes every stand-in for such a region start from a byte of the caller's choice (csrc/scratch_fill.h;
the zeros the twins keep each name the device-side clear they mirror), and the case lists of the twins' own tests run again here at

    0x00   the control: the bytes the twins had before, so a failure at this fill alone is the harness's
    0x5A   the project's poison byte (gpu_huffman_host.cpp fills coded blocks with it)
    0xFF   all ones: kRecInvalid as a record mark, kLlInvalidPacked as a lossless state, -1 as a count or an index

with the expectations those tests have: the writers' coefficients, the host entropy stage, the oracle, the numpy model of the lossless
decoder, the host coder's files.  (A 16-bit record mark below kRecOverflow -- a record that reads as usable -- is 0x0000 .. 0x00FD: of
all uniform fills only the control produces one, with a count of zero blocks; no further byte would add a plausible value.)"""
import functools

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import coder_seams as CS
from helpers import lossless_entropy_cases as EC
from helpers import lossless_files as LF
from helpers import progressive_restart_files as P
from helpers import progressive_seams as PS
from helpers import steered_streams as S
from helpers import walk_files as W
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from test_walk_long_codes import PASSES_AT_B0FFFD0

FILLS = [0x00, 0x5A, 0xFF]
INTERNAL_ERROR, UNSUPPORTED = 10, 3


@pytest.fixture(params=FILLS, ids=["fill_%02x" % b for b in FILLS])
def fill(request):
    lowlevel.set_twin_scratch_fill(request.param)
    yield request.param
    lowlevel.set_twin_scratch_fill(0)


def test_the_hook_takes_bytes_only():
    for bad in (-1, 256):
        with pytest.raises(N.HipJpegError) as err:
            lowlevel.set_twin_scratch_fill(bad)
        assert err.value.status == 1  # INVALID_ARGUMENT
    lowlevel.set_twin_scratch_fill(0)


# ---------------------------------------------------------------- hipjpegEntropyDecodeGpuAlgorithmHost: sequential streams
@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_steered_streams(fill, name):
    """helpers/steered_streams.py, as tests/test_steered_streams.py::test_decoders_agree_with_the_writer"""
    for k, w in enumerate(S.family(name)):
        want = w.coefficients()
        algo, _ = lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)  # (raises on any status, INTERNAL_ERROR included)
        host, _ = lowlevel.entropy_decode_host(w.jpeg)
        assert algo[0].shape == want.shape and np.array_equal(algo[0], want), (name, k)
        assert np.array_equal(algo[0], host[0]), (name, k)


def test_walk_table_class_files(fill):
    """helpers/walk_files.py class_files(), as tests/test_walk_table_classes.py: one- and multi-scan files, up to ten MCU positions; the
    one-component scans among them have padding blocks, which only the planner's zero fills reach"""
    for name, jpeg, meant, samp in W.class_files():
        got, passes = lowlevel.entropy_decode_gpu_algorithm_host(jpeg)
        host, _ = lowlevel.entropy_decode_host(jpeg)
        ref, _ = oracle.decode_coefficients(jpeg)
        assert passes >= 1
        for c, (a, b, r) in enumerate(zip(got, host, ref)):
            assert np.array_equal(a, b), (name, "component", c, "differs from the host decoder")
            assert np.array_equal(a, r), (name, "component", c, "differs from the oracle")
        if len(samp) > 1:
            for c, (a, m) in enumerate(zip(got, meant)):
                assert np.array_equal(a, m), (name, "component", c, "differs from what the writer meant")


def test_walk_long_code_files(fill):
    """helpers/walk_files.py long_code_files(), as tests/test_walk_long_codes.py: coefficients, the pinned sync_passes, and the host
    decoder's status for the damaged stream"""
    files = W.long_code_files()
    assert {n for n, _, ok in files if ok} == set(PASSES_AT_B0FFFD0)
    for name, w, ok in files:
        if not ok:
            with pytest.raises(N.HipJpegError) as host:
                lowlevel.entropy_decode_host(w.jpeg)
            with pytest.raises(N.HipJpegError) as emulated:
                lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)
            assert emulated.value.status == host.value.status and host.value.status != INTERNAL_ERROR, name
            continue
        got, passes = lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)
        host, _ = lowlevel.entropy_decode_host(w.jpeg)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[0], w.coefficients()), name
        assert passes == PASSES_AT_B0FFFD0[name], name


# ---------------------------------------------------------------- ... progressive streams (walk + replay)
def test_progressive_seams(fill):
    """helpers/progressive_seams.py, as tests/test_progressive_seams.py::test_every_decoder_gives_back_the_chosen_coefficients"""
    assert len(PS.CASES) == 87
    for name in sorted(PS.CASES):
        c = PS.get(name)
        if not c.in_limit:
            with pytest.raises(N.HipJpegError) as err:
                lowlevel.entropy_decode_gpu_algorithm_host(c.jpeg)
            assert err.value.status == UNSUPPORTED, name
            continue
        got, _ = oracle.decode_coefficients(c.jpeg)
        emu, _ = lowlevel.entropy_decode_gpu_algorithm_host(c.jpeg)
        assert len(got) == len(emu) == len(c.coefs), name
        for k in range(len(c.coefs)):
            rows, cols = PS.real_blocks(c, k)
            want = np.asarray(c.coefs[k])[:rows, :cols].astype(np.int16)
            assert np.array_equal(np.asarray(emu[k])[:rows, :cols], want), (name, "GPU algorithm on the host", k)
            assert np.array_equal(emu[k], got[k]), (name, "blocks of the MCU padding", k)


# ---------------------------------------------------------------- hipjpegEntropyDecodeGpuIntervalAlgorithmHost
def _interval_algorithm_equals_oracle(jpeg, what):
    ref, _ = oracle.decode_coefficients(jpeg)
    got = lowlevel.entropy_decode_gpu_interval_algorithm_host(jpeg)
    assert len(ref) == len(got), what
    for c, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), (what, c)


def test_progressive_restart_files(fill):
    """helpers/progressive_restart_files.py, as tests/test_progressive_intervals.py: the chosen scripts, the project's own progressive
    files, the refused case"""
    for name in sorted(P.HELPER_CASES):
        jpeg, coefs = P.helper_file(name)
        got, _ = oracle.decode_coefficients(jpeg)
        emu = lowlevel.entropy_decode_gpu_interval_algorithm_host(jpeg)
        for c in range(len(coefs)):
            rows, cols = P.real_blocks(name, c)
            want = np.asarray(coefs[c])[:rows, :cols].astype(np.int16)
            assert np.array_equal(np.asarray(emu[c])[:rows, :cols], want), (name, "interval algorithm on the host", c)
            assert np.array_equal(emu[c], got[c]), (name, "blocks of the MCU padding", c)
    files = P.transcode_products(GOLDEN)
    assert len(files) == 12
    for name, jpeg in files:
        _interval_algorithm_equals_oracle(jpeg, name)
    with pytest.raises(N.HipJpegError) as err:
        lowlevel.entropy_decode_gpu_interval_algorithm_host(P.helper_file(P.DIFFERENT_INTERVALS)[0])
    assert err.value.status == UNSUPPORTED


def test_progressive_restart_files_of_libjpeg_turbo(fill):
    pytest.importorskip("PIL")
    files = P.pillow_files()
    assert len(files) == 27
    for name, jpeg in files:
        _interval_algorithm_equals_oracle(jpeg, name)


# ---------------------------------------------------------------- hipjpegLosslessEntropyAlgorithmHost
def _host_status(f):
    try:
        lowlevel.decode_lossless_host(f)
        return 0
    except N.HipJpegError as e:
        return e.status


def test_lossless_entropy_cases(fill):
    """helpers/lossless_entropy_cases.py, as tests/test_lossless_gpu_entropy_host.py: the seams against the numpy model, the stream that
    cannot synchronise, the damaged files' statuses"""
    shape = lowlevel.lossless_entropy_shape()
    cases = EC.seam_cases(shape)
    assert len(cases) == 1 + 6 + 8 + 2 + 2 + 9 + 1 + 2 + 1 + 1
    for name, f, d, rr in cases:
        st, planes, converged = lowlevel.lossless_entropy_algorithm_host(f)
        assert st == 0 and converged, name
        assert np.array_equal(np.moveaxis(planes, 0, 2), (d & 0xFFFF).astype(np.uint16)), name
        model = LF.model_decode(np.moveaxis(planes.astype(np.int64), 0, 2), 16, 1, 0, rr)
        assert np.array_equal(model, LF.model_decode(d, 16, 1, 0, rr)), name
    f, d = EC.unsynchronisable(shape)
    st, planes, converged = lowlevel.lossless_entropy_algorithm_host(f)
    assert st == 0 and not converged and not planes.any()
    st, planes, converged = lowlevel.lossless_entropy_algorithm_host(LF.write_differences(d, 8, 1, table=LF.LONG))
    assert st == 0 and converged and not planes.any()
    bad = EC.bad_cases()
    assert len(bad) == 8
    for name, f in bad:
        st, planes, converged = lowlevel.lossless_entropy_algorithm_host(f)
        assert st == _host_status(f), name


# ---------------------------------------------------------------- hipjpegEncodeBaselineGpuAlgorithmHost, ...ProgressiveGpuAlgorithmHost
@functools.lru_cache(maxsize=None)
def _coder_files():
    return {c.name: CS.view(c).file for c in CS.cases()}  # the host coder's files: no scratch of the twins in them


def test_coder_seams(fill):
    """helpers/coder_seams.py, as tests/test_coder_seams.py::test_kernel_code_on_host_gives_the_same_files"""
    entries = set()
    for c in CS.cases():
        for entry, file in CS.algorithm_host_files(c).items():
            assert file == _coder_files()[c.name], (c.name, entry)
            entries.add(entry)
    assert entries == {"hipjpegEncodeBaselineGpuAlgorithmHost", "hipjpegEncodeFromCoefficientsGpuAlgorithmHost",
                       "hipjpegEncodeProgressiveGpuAlgorithmHost"}
