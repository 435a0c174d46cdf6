"""Crafted progressive scans on every seam of the GPU walk (csrc/progressive_gpu.hip, csrc/progressive_gpu_core.h), without a GPU: each file of
tests/helpers/progressive_seams.py is first shown to BE where it claims to be -- its condition is a predicate over the writer's own log of
bit positions, asserted here --, then pinned: the oracle gives back the coefficients the file was written from, the host entropy decoder and
the host emulation of the walk + replay agree, and for one- and three-component files libjpeg-turbo (Pillow) decodes the same pixels as the
oracle, which ties the constructs libjpeg's coder never writes (blocks closed by a run of sixteen, thousands of correction bits behind one
run symbol, a declared run longer than the scan) to the real library.  tests/test_gpu_progressive_seams.py runs the same files through the kernels."""
import io

import numpy as np
import pytest

import oracle
from helpers import progressive_seams as S
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

OVER_THE_LIMIT = ["limit_7_stages", "limit_16_ac_scans", "limit_25_scans", "limit_10_second_level_tables"]


def test_the_list_of_cases():
    assert sorted(n for n in S.CASES if not S.CASES[n]()[0].in_limit) == sorted(OVER_THE_LIMIT)
    assert len(S.CASES) == 87 and all(S.CASES[n]()[0].name == n for n in S.CASES)
    assert sum(n.startswith("window_") for n in S.CASES) == 2 * 5 * 3 + 3  # two scan kinds x five event kinds x three positions, + 3


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_the_file_sits_on_its_seam(name):
    """The case's condition holds, and the log it is read from accounts for every bit of every scan: the events lie end to end from bit 0
    to the scan's last bit before the padding, and the scan's destuffed bytes are those bits."""
    assert S.holds(name)
    c = S.get(name)
    assert max(a.shape[0] * a.shape[1] for a in c.coefs) <= 640
    assert b"\xff\xdd" not in c.jpeg[: c.jpeg.find(b"\xff\xda")]  # no DRI segment
    for s in c.log:
        pos = 0
        for ev in sorted((ev for ev in s.events if ev.kind != "block"), key=lambda ev: ev.pos):
            assert ev.pos == pos and ev.nbits > 0, (s.entry, ev)
            pos += ev.nbits
        assert pos == s.bits and len(s.data) == -(-s.bits // 8), s.entry
        assert all(0 <= ev.pos <= s.bits for ev in s.events if ev.kind == "block")


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_every_decoder_gives_back_the_chosen_coefficients(name):
    c = S.get(name)
    got, _ = oracle.decode_coefficients(c.jpeg)
    host, _ = lowlevel.entropy_decode_host(c.jpeg)
    if c.in_limit:
        emu, _ = lowlevel.entropy_decode_gpu_algorithm_host(c.jpeg)
    else:
        with pytest.raises(N.HipJpegError) as err:
            lowlevel.entropy_decode_gpu_algorithm_host(c.jpeg)
        assert err.value.status == 3  # UNSUPPORTED: the host entropy stage keeps the file
        emu = host
    assert len(got) == len(host) == len(emu) == len(c.coefs)
    for k in range(len(c.coefs)):
        rows, cols = S.real_blocks(c, k)
        want = np.asarray(c.coefs[k])[:rows, :cols].astype(np.int16)
        assert np.array_equal(np.asarray(got[k])[:rows, :cols], want), ("oracle", k)
        assert np.array_equal(np.asarray(host[k])[:rows, :cols], want), ("host decoder", k)
        assert np.array_equal(np.asarray(emu[k])[:rows, :cols], want), ("GPU algorithm on the host", k)
        assert np.array_equal(emu[k], got[k]), ("blocks of the MCU padding", k)


@pytest.mark.parametrize("name", sorted(n for n in S.CASES if len(S.CASES[n]()[0].sampling) in (1, 3)))
def test_libjpeg_turbo_decodes_the_oracles_pixels(name):
    pytest.importorskip("PIL")
    from PIL import Image
    c = S.get(name)
    im = np.asarray(Image.open(io.BytesIO(c.jpeg)).convert("RGB"))
    assert np.array_equal(im, oracle.decode(c.jpeg))


def test_the_writer_agrees_with_the_helper_it_builds_on():
    """Without options write_seams() is write_progressive_restart() without its DRI segments, bit for bit."""
    from helpers import progressive_restart_files as P
    samp, w, h, script, _, max_run, dense = P.HELPER_CASES["bands_cut_anywhere"]
    _, coefs = P.helper_file("bands_cut_anywhere")
    qt = [np.full(64, 3 + c, dtype=np.int32) for c in range(3)]
    ours, log = S.write_seams(w, h, samp, coefs, qt, script, max_run)
    theirs = P.write_progressive_restart(w, h, samp, coefs, qt, script, [0] * len(script), max_run)
    assert ours == theirs.replace(b"\xff\xdd\x00\x04\x00\x00", b"") and len(log) == len(script)
    assert any(ev.arg > 1 for s in log for ev in S.find(s, "eob"))  # end-of-band runs of several blocks, as the helper codes them
