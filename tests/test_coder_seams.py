"""The steered coefficient pictures of tests/helpers/coder_seams.py, checked without a GPU: every case sits on the seam of the GPU
entropy coder it claims (predicate over the host coder's file; for baseline files the bit model's self-check), the host coder's
entropy-coded bytes are those of an independent writer, the host executions of the kernels' code give the same files, the census of
seams is complete and the kernels' constants restated in the helper are still the ones in the sources.  tests/test_gpu_coder_seams.py
runs the same cases through the kernels."""
import functools
import os

import numpy as np

from helpers import coder_seams as CS
from nvimagecodec_amd import lowlevel

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nvimagecodec_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _views():
    return {c.name: CS.view(c) for c in CS.cases()}


def test_every_case_sits_on_its_seam():
    """Predicate and, for baseline files, the model's self-check: its total rounded up to bytes is the unstuffed length and every RSTn
    sits where the model puts it."""
    names = [c.name for c in CS.cases()]
    assert len(set(names)) == len(names)
    for c in CS.cases():
        v = _views()[c.name]
        assert c.predicate(v), c.name
        if not c.params["progressive"]:
            assert len(v.segs) == 1, c.name
            v.model.self_check(v.segs[0])
            assert v.model.n <= 2400, c.name
        assert all((q == 1).all() for q in c.info["qtables"]), c.name
        assert all(np.abs(a[..., 0, 0]).max() <= 1023 and np.abs(a).max() <= 1023 for a in c.coefs), c.name


def test_annex_k_entropy_bytes_are_an_independent_writers():
    checked = 0
    for c in CS.cases():
        if c.params["progressive"] or c.params["optimized_huffman"]:
            continue
        assert CS.entropy_bytes(_views()[c.name].file) == CS.entropy_bytes(CS.anchor_file(c)), c.name
        checked += 1
    assert checked >= 40


def test_kernel_code_on_host_gives_the_same_files():
    entries = set()
    for c in CS.cases():
        for entry, file in CS.algorithm_host_files(c).items():
            assert file == _views()[c.name].file, (c.name, entry)
            entries.add(entry)
    assert entries == {"hipjpegEncodeBaselineGpuAlgorithmHost", "hipjpegEncodeFromCoefficientsGpuAlgorithmHost",
                       "hipjpegEncodeProgressiveGpuAlgorithmHost"}


def test_census_is_complete():
    claimed = {s for c in CS.cases() for s in c.seams} | {s for b in CS.batches() for s in b.seams}
    assert claimed == set(CS.SEAMS), sorted(set(CS.SEAMS) ^ claimed)
    by = lambda seam, **kw: [c for c in CS.cases() if seam in c.seams and all(bool(c.params[k]) == v for k, v in kw.items())]
    # the write kernel's seams: without restart intervals, and with them where the list asks for it
    for seam in ("W1", "W2", "W3", "W5"):
        assert by(seam, progressive=False, restart_interval=False), seam
    for seam in ("W1", "W4", "W5", "S1"):
        assert by(seam, progressive=False, restart_interval=True), seam
    assert by("S1", restart_interval=False)
    # count / layout / expand: baseline and progressive output; the marker seams need restart intervals
    for seam in ("E1", "E2", "E3", "E4", "E5", "E7"):
        assert by(seam, progressive=False) and by(seam, progressive=True), seam
    for seam in ("E6", "E6b", "E6c"):
        assert by(seam, progressive=False, restart_interval=True) and by(seam, progressive=True, restart_interval=True), seam


def test_alignment_combinations_are_all_reached():
    """E3: destination misalignment 0..3 of a chunk c >= 1 with every residue of its output length, for both kinds of output"""
    for progressive in (False, True):
        seen = set()
        for c in CS.cases():
            if "E3" in c.seams and c.params["progressive"] == progressive:
                seen |= CS.alignment_combinations(_views()[c.name])
        assert seen == {(a, r) for a in range(4) for r in range(4)}, progressive


def test_reached_values():
    """What DESIGN.md states: the largest window and the smallest write-through range, exactly; the share of 0xFF"""
    v = _views()
    assert v["w3_window_4096"].model.words(1) == CS.WINDOW_WORDS and v["w3_through_4097"].model.words(1) == CS.WINDOW_WORDS + 1
    assert max(CS.ff_share(s) for s in v["base_e7_half_ff"].segs) >= 0.5
    assert max(CS.ff_share(s) for s in v["prog_e7_half_ff"].segs) >= 0.5


def test_batches_mix_what_they_claim():
    w6, e8a, e8b = CS.batches()
    assert CS.p_mixed_launch(w6.cases)
    for b, n in ((e8a, 257), (e8b, 513)):
        assert len(b.cases) == n and all(c.info["blocks_w"] == [1] and c.info["blocks_h"] == [1] for c in b.cases)
        segments = [len(CS.view(c).segs) for c in b.cases]
        assert all(s == 1 for s in segments[0::2]) and all(s > 1 for s in segments[1::2])


def test_constants_are_the_sources():
    for name, places in CS.SOURCE_TEXT.items():
        for fname, text in places:
            with open(os.path.join(_CSRC, fname)) as f:
                assert text in f.read(), (name, fname, text)


def test_reference_files_round_trip():
    for c in list(CS.cases()) + [c for b in CS.batches()[1:] for c in b.cases]:
        info, coefs = lowlevel.decode_coefficients_host(CS.view(c).file)
        assert info["blocks_w"] == c.info["blocks_w"] and info["blocks_h"] == c.info["blocks_h"], c.name
        assert all(np.array_equal(a, b) for a, b in zip(coefs, c.coefs)), c.name
