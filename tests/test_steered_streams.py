"""The steered files of tests/helpers/steered_streams.py are what they claim to be, on the CPU: the oracle decodes exactly the
coefficients the writer meant, the host entropy decoder and the host emulation of the GPU entropy stage agree, the placed bytes lie on
the raw offsets asked for -- and a destuffing gone wrong at any placed byte shows in the pixels, which is what makes the pixel
comparison of tests/test_gpu_steered_streams.py a test of the device's destuffing.  No GPU needed."""
import numpy as np
import pytest

import oracle
from helpers import steered_streams as S
from nvimagecodec_amd import lowlevel

CHUNK, WG = S.CHUNK, S.WG_BYTES
FAMILIES = list(S.FAMILIES)


def _destuffed(scan):
    out, k = bytearray(), 0
    while k < len(scan):
        out.append(scan[k])
        k += 2 if scan[k] == 0xFF and k + 1 < len(scan) and scan[k + 1] == 0 else 1
    return bytes(out)


@pytest.mark.parametrize("name", FAMILIES)
def test_decoders_agree_with_the_writer(name):
    for k, w in enumerate(S.family(name)):
        want = w.coefficients()
        ref, qt = oracle.decode_coefficients(w.jpeg)
        assert np.array_equal(ref[0], want), (name, k)
        assert list(qt[0]) == S.QUANT_TABLE   # (position 62 is the same in zigzag and in natural order)
        host, _ = lowlevel.entropy_decode_host(w.jpeg)              # (raises HipJpegError on any status, UNSUPPORTED included)
        algo, _ = lowlevel.entropy_decode_gpu_algorithm_host(w.jpeg)
        assert host[0].shape == want.shape and np.array_equal(host[0], want), (name, k)
        assert algo[0].shape == want.shape and np.array_equal(algo[0], want), (name, k)
        assert int(S.pixels(w).max()) - int(S.pixels(w).min()) >= 32   # no flat picture, in which lost coefficients would not show


@pytest.mark.parametrize("name", FAMILIES)
def test_placed_bytes_are_where_they_were_asked_for(name):
    """Found again in the file's bytes, behind its SOS header, and the only FFs near them."""
    for w in S.family(name):
        assert w.jpeg[len(w.header):-2] == w.scan and w.jpeg.endswith(b"\xff\xd9")
        for kind, at in w.placed:
            assert w.scan[at] == 0xFF and at > 0 and w.scan[at - 1] != 0xFF
            assert w.scan[at + 1] == 0 if kind == "ff" else 0xD0 <= w.scan[at + 1] <= 0xD7


def _offsets(name, kind="ff"):
    return [sorted(at for k, at in w.placed if k == kind) for w in S.family(name)]


def test_seams_cover_what_they_should():
    ffs = _offsets("seams")
    single = {o[0] for o in ffs if len(o) == 1}
    assert single == {s + d for s in (16, 64, 128, 4096 - 192, 4096) for d in (-2, -1, 0, 1)}
    pairs, triples = [o for o in ffs if len(o) == 2], [o for o in ffs if len(o) == 3]
    assert all(o == [o[0] + 2 * k for k in range(len(o))] for o in pairs + triples)          # FF 00 FF 00 [FF 00]
    assert {o[0] % 64 for o in pairs} == {61, 62, 63, 0} and {o[0] % 64 for o in triples} == {59, 60, 61, 62, 63, 0}
    assert {len(w.scan) & 15 for w in S.family("seams")} == {0, 1, 15}
    assert all(len(w.scan) <= CHUNK for w in S.family("seams"))


def test_chunk_seams_cover_every_output_alignment():
    seen = set()
    for w, ffs in zip(S.family("chunks"), _offsets("chunks")):
        assert len(w.scan) > 2 * CHUNK
        early = [at for at in ffs if at < CHUNK - 2]
        d = ffs[len(early)] - CHUNK
        assert ffs[len(early):] == [CHUNK + d, 2 * CHUNK + d]
        # bytes dropped in front of chunk 1 (the 00 of an FF on a chunk's last byte belongs to the next chunk)
        seen.add((d, sum(1 for at in ffs if at + 1 < CHUNK) % 4))
    assert seen == {(d, a) for d in (-2, -1, 0, 1) for a in range(4)}


def test_last_chunk_lengths():
    lengths = [len(w.scan) for w in S.family("last_chunk")]
    assert sorted(set(lengths)) == sorted([CHUNK + n for n in (1, 2, 3, 4, 15, 16, 17, 63, 64, 65)] + [CHUNK, 2 * CHUNK])
    ends = [w.scan[-2:] == b"\xff\x00" for w in S.family("last_chunk")]
    assert sum(ends) >= 3 and {len(w.scan) for w, e in zip(S.family("last_chunk"), ends) if e} >= {CHUNK, 2 * CHUNK, CHUNK + 2}


def test_restart_markers_cover_what_they_should():
    rst = {at for o in _offsets("restart_placed", "rst") for at in o}
    assert rst >= {CHUNK - 2, CHUNK - 1, CHUNK, 191, 192, 64 * 40 - 1, 64 * 40}
    both = [(sorted(at for k, at in w.placed if k == "ff"), sorted(at for k, at in w.placed if k == "rst"))
            for w in S.family("restart_placed")]
    assert {r[-1] for f, r in both if f and f[-1] == r[-1] - 2} == {255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1}   # FF 00 FF Dn
    for w in S.family("restart_placed"):   # restart_interval = 1 and blocks of mostly one byte: most raw bytes are markers
        assert 2 * w.nrst > 0.55 * len(w.scan)
    for w, ri in zip(S.family("restart_intervals"), (2, 7, 128, 127, 129)):
        assert w.ri == ri and w.nrst == -(-w.closed // ri) - 1 and w.dbits == 64 * w.closed


def test_stream_ends_have_the_lengths_asked_for():
    got = sorted((w.dbits // 8, 8 * len(_destuffed(w.scan)) - w.dbits) for w in S.family("stream_ends"))
    assert [g[1] for g in got] == [0] * len(got)   # whole bytes, padding included
    want = (127, 128, 129, WG - 1, WG, WG + 1, WG + 128, 2 * WG - 1, 2 * WG + 1)
    assert [g[0] for g in got] == sorted(want + want)
    for w in S.family("stream_ends"):   # the padding: the last byte ends in seven ones, or the last block ends with it
        assert sum(1 for v in S.family("stream_ends") if v.dbits == w.dbits) == 2
    assert sum(1 for w in S.family("stream_ends") if w.scan[-1] & 0x7F == 0x7F) >= len(want)


def test_fixed_size_blocks_have_their_size():
    for w, bits in zip(S.family("record_slots"), (33, 34, 35, 1024, 512)):
        assert w.closed == 64 * 40 and w.dbits == bits * w.closed
    long_ones = [sum(1 for dc, ac in w.blocks if len(ac) == 63) for w in S.family("long_blocks")]
    assert long_ones == [4, 8, 12, 7]
    assert [w.closed for w in S.family("strips")] == [127, 128, 129, 255, 256, 257]


@pytest.mark.parametrize("name", ["seams", "chunks", "last_chunk", "restart_placed", "stream_ends", "strips"])  # (those that place bytes)
def test_a_destuffing_gone_wrong_at_a_placed_byte_shows_in_the_pixels(name):
    """Mutation check: for every placed byte, the files a wrong compact kernel would in effect have decoded (helpers/steered_streams.py
    mutants) are refused by the oracle or decode to other pixels than the intact file.  The one exception is asserted too: a 00
    kept behind an FF that is the last data byte of its restart interval or of the scan lies behind the last bit any decoder reads,
    so that file must decode to the SAME pixels (mutants() says which these are and why the device would still show the error)."""
    checked = blind = 0
    for k, w in enumerate(S.family(name)):
        good = S.pixels(w)
        for what, jpeg, shows in S.mutants(w):
            try:
                bad = oracle.decode(jpeg, oracle.FMT_GRAY)
            except oracle.OracleError:
                assert shows, (name, k, what)
                checked += 1
                continue
            assert bad.shape == good.shape and np.array_equal(bad, good) != shows, (name, k, what)
            checked += shows
            blind += not shows
    placed = sum(len(w.placed) for w in S.family(name))
    assert checked >= 3 * placed - 2 * len(S.family(name)) and blind <= placed // 4
