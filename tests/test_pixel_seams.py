"""No GPU: the framed arena of tests/helpers/framed_outputs.py catches a stray byte wherever it is planted, and the case list of
tests/helpers/pixel_seams.py sits where it claims -- every case's claimed classes are reached under the restated tile arithmetic and path
conditions, the census reaches every required class, and the restated constants and conditions stand in the sources as text.
tests/test_gpu_pixel_seams.py decodes the cases."""
import os

import numpy as np
import pytest
import torch

import oracle
from helpers import framed_outputs as F
from helpers import pixel_seams as P
from nvimagecodec_amd import lowlevel

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nvimagecodec_amd", "csrc")


# ---------------------------------------------------------------- the arena
def _small_layout():
    """one output of every kind: interleaved, planar (three planes), luma, raw planes"""
    lay = F.Layout()
    lay.add("rgb", "rgb", (5, 7, 3), pitch=40, residue=3)
    lay.add("planar", "rgb_planar", (3, 4, 9), pitch=24, residue=8, plane_stride=4 * 24 + 132)
    lay.add("y", "y", (3, 10), pitch=17, residue=1)
    lay.add("yuv", "yuv_planar", [(6, 10), (3, 5), (3, 5)], planes=[(16, 0), (9, 5), (8, 2)])
    return lay


def _filled(lay, sentinel):
    """an arena on the CPU whose outputs hold their expectations, as after a faultless decode"""
    rng = np.random.default_rng(7)
    arena = F.Arena(lay, sentinel, device="cpu", torch=torch)
    expected = []
    for frame, out in zip(lay.frames, arena.outs):
        if frame.fmt == "yuv_planar":
            want = [rng.integers(0, 256, s, dtype=np.uint8) for s in frame.shape]
            for o, w in zip(out, want):
                o.copy_(torch.from_numpy(w))
        else:
            want = rng.integers(0, 256, frame.shape, dtype=np.uint8)
            out.copy_(torch.from_numpy(want))
        expected.append(want)
    return arena, expected


def test_arena_layout_keeps_lead_tail_and_gaps():
    lay = _small_layout()
    rows = lay.rows()
    assert rows[0, 0] >= F.LEAD and lay.nbytes - rows[-1, 1] >= F.TAIL
    owned = lay.owned()
    assert owned.sum() == 5 * 21 + 3 * 4 * 9 + 30 + 60 + 15 + 15
    # between two frames and between two planes: at least GAP sentinel bytes
    for a, b in zip(rows[:-1], rows[1:]):
        if (a[2], a[3]) != (b[2], b[3]):
            assert b[0] - a[1] >= F.GAP, (a, b)
    # the views are where the layout says, with the strides BatchDecoder._marshal reads
    arena = F.Arena(lay, 0xAB, device="cpu", torch=torch)
    base = arena.buf.data_ptr()
    rgb, planar, y, yuv = arena.outs
    assert rgb.data_ptr() - base == lay.frames[0].planes[0].offset and rgb.stride(0) == 40 and rgb.data_ptr() % 256 == 3
    assert [planar[p].data_ptr() - base for p in range(3)] == [q.offset for q in lay.frames[1].planes] and planar.stride(1) == 24
    assert [t.data_ptr() % 256 for t in yuv] == [0, 5, 2] and [t.stride(0) for t in yuv] == [16, 9, 8]
    assert y.stride(0) == 17


@pytest.mark.parametrize("sentinel", F.SENTINELS)
def test_check_passes_on_a_clean_arena_and_names_wrong_pixels(sentinel):
    arena, expected = _filled(_small_layout(), sentinel)
    arena.check(expected)
    assert np.array_equal(arena.decoded(arena.host(), 1), expected[1])
    expected[1] = expected[1].copy()
    expected[1][2, 3, 4] ^= 1
    with pytest.raises(AssertionError, match=r"image 1 \(planar, rgb_planar\) plane 2: 1 wrong bytes, first at row 3 byte 4"):
        arena.check(expected)


def _places(lay):
    """one arena offset in each kind of place a stray byte can land, with what check() must say about it"""
    f = lay.frames
    rgb, planar, yuv = f[0].planes[0], f[1].planes, f[3].planes
    return {
        "lead": (rgb.offset - 1, r"in the lead, 1 bytes before image 0 \(rgb\) plane 0 row 0"),
        "lead_start": (0, r"in the lead, \d+ bytes before image 0"),
        "row_gap": (rgb.offset + 2 * rgb.pitch + rgb.row_bytes, r"image 0 \(rgb\) plane 0 row 2, \+1 bytes past the row's end"),
        "row_gap_far": (rgb.offset + 3 * rgb.pitch - 1, r"image 0 \(rgb\) plane 0 row 2, \+19 bytes past the row's end"),
        "between_planes": (planar[1].offset - 2, r"image 1 \(planar\) plane 0 row 3, \+\d+ bytes past the row's end \(between planes\)"),
        "between_yuv_planes": (yuv[0].offset + 5 * 16 + 10 + 3, r"image 3 \(yuv\) plane 0 row 5, \+4 bytes past the row's end \(between planes\)"),
        "between_frames": (planar[2].offset + 3 * 24 + 9 + 14, r"image 1 \(planar\) plane 2 row 3, \+15 bytes past the row's end \(between frames\)"),
        "tail": (yuv[2].offset + 2 * 8 + 5, r"image 3 \(yuv\) plane 2 row 2, \+1 bytes past the row's end \(the tail\)"),
        "tail_end": (lay.nbytes - 1, r"\(the tail\)"),
    }


@pytest.mark.parametrize("place", sorted(_places(_small_layout())))
def test_check_catches_a_stray_byte_wherever_it_lands(place):
    lay = _small_layout()
    offset, message = _places(lay)[place]
    for sentinel in F.SENTINELS:
        arena, expected = _filled(lay, sentinel)
        arena.buf[offset] = 0x11
        with pytest.raises(AssertionError, match=message) as err:
            arena.check(expected)
        assert "stray byte 0x11 at arena offset %d" % offset in str(err.value) and "1 stray bytes in all" in str(err.value)


def test_a_stray_byte_that_equals_one_sentinel_is_caught_by_the_other():
    lay = _small_layout()
    offset = _places(lay)["row_gap"][0]
    for value in F.SENTINELS:
        caught = []
        for sentinel in F.SENTINELS:
            arena, expected = _filled(lay, sentinel)
            arena.buf[offset] = value
            try:
                arena.check(expected)
                caught.append(False)
            except AssertionError as e:
                assert "stray byte 0x%02X" % value in str(e)
                caught.append(True)
        # invisible in the arena it equals, seen in the other: a pair of runs always sees it
        assert caught == [sentinel != value for sentinel in F.SENTINELS]
    assert F.SENTINELS[0] ^ F.SENTINELS[1] == 0xFF


def test_check_takes_hashes_and_skips_refused_images():
    import hashlib
    arena, expected = _filled(_small_layout(), 0xAB)
    bgr = expected[0][:, :, ::-1]
    sha = hashlib.sha256(np.ascontiguousarray(bgr).tobytes()).hexdigest()
    arena.check([F.Hashed(sha, lambda a: a[:, :, ::-1]), None, expected[2], expected[3]])
    with pytest.raises(AssertionError, match="image 0 .* do not hash"):
        arena.check([F.Hashed(sha, lambda a: a), None, expected[2], expected[3]])


def test_overlapping_placements_are_refused():
    lay = F.Layout()
    with pytest.raises(AssertionError):
        lay.add("p", "rgb_planar", (3, 4, 9), pitch=24, plane_stride=4 * 24)  # no gap between the planes
    with pytest.raises(AssertionError):
        lay.add("r", "rgb", (4, 9, 3), pitch=26)


# ---------------------------------------------------------------- the case list
def test_restated_constants_and_conditions_stand_in_the_sources():
    text = {}
    for key, places in P.SOURCE_TEXT.items():
        for name, needle in places:
            if name not in text:
                with open(os.path.join(CSRC, name)) as f:
                    text[name] = f.read()
            assert text[name].count(needle) >= 1, (key, name, needle)
    assert P.WIDE_ROW_BYTES == 768 and P.NARROW_ROW_BYTES == 384 and 6 * 64 * 16 == 8 * P.WIDE_ROW_BYTES == 16 * P.NARROW_ROW_BYTES


def test_every_case_reaches_the_classes_it_claims():
    assert len(P.cases()) > 250
    for c in P.cases():
        got = P.reached(c)
        assert set(c.seams) <= got, (c.name, sorted(set(c.seams) - got))


def test_census_reaches_every_required_class():
    claimed = set()
    for c in P.cases():
        claimed |= set(c.seams)
    assert not [k for k in P.REQUIRED if k not in claimed]
    # the three tile situations of the staged store see all 16 residues of row_bytes, every sampling K2 fuses meets both tile shapes,
    # and every flavour of family A sees every case
    a = P.family("A")
    assert len(a) == 3 * 49 and {c.fmt + str(c.fancy) for c in a} == {"rgbTrue", "bgrTrue", "rgbFalse"}
    for letter in "ABCDEF":
        assert P.family(letter), letter
    # every format a family decodes has neighbours from other families to share its batch with, at least once per family
    for letter in "ABCDEF":
        assert any(P.neighbours(letter, fmt, fancy) for (fmt, fancy) in P.groups(P.family(letter))), letter


def test_pictures_stay_small_and_placements_leave_guard_bytes():
    for c in P.cases():
        i = P.info(c.source)
        assert i["width"] * i["height"] <= 400 * 80 * 2, c.name
        if c.source[0] == "synth":
            assert max(i["width"], i["height"]) <= 400 and min(i["width"], i["height"]) <= 80, c.name
    # every family's whole list places without overlap, and every row has at least 16 sentinel bytes behind it: a store of up to 15 bytes
    # past a row's end lands on guard bytes, not on the next row
    for letter in "ABCDEF":
        lay = F.Layout()
        for c in P.family(letter):
            lay.add(c.name, c.fmt, P.output_shape(c), **c.place)
        rows = lay.rows()
        assert np.all(rows[1:, 0] - rows[:-1, 1] >= 16), letter
        lay.owned()
        assert lay.nbytes < 32 << 20


def test_restated_grids_are_the_hosts():
    """the restated luma grid and the oracle's component sizes against hipjpegGetImageInfo (host only)"""
    seen = set()
    for c in P.cases():
        if c.source in seen or c.source[0] != "synth":
            continue
        seen.add(c.source)
        _, w, h, sub = c.source
        hi = lowlevel.get_image_info(P.jpeg(c.source))
        oi = P.info(c.source)
        assert (hi["width"], hi["height"]) == (w, h) and P.sub_of(c.source) == sub
        assert P.luma_grid(w, h, sub) == (hi["blocks_w"][0], hi["blocks_h"][0]), c.name
        assert hi["blocks_w"] == oi["bw"] and hi["blocks_h"] == oi["bh"] and hi["samp_w"] == oi["dw"] and hi["samp_h"] == oi["dh"], c.name


def test_tile_arithmetic_on_known_pictures():
    # 1920 x 1080, 4:2:0: 240 block columns = 7 wide tiles + 16 columns of narrow tiles; 135 real block rows
    t = P.luma_tiles(1920, 1080, "420")
    assert len([x for x in t if not x[2]]) == 7 * 34 and len([x for x in t if x[2]]) == 17 and {x[0] for x in t if x[2]} == {224}
    # a region whose narrow tiles start in the middle of the whole picture's: one narrow tile from block row 4, none from 0
    x0, y0, x1, y1, _ = P.REGIONS[0]
    t = P.luma_tiles(400, 80, "420", (x0, y0, x1, y1))
    assert t == [(32, 4, True)]
    assert P.luma_tiles(384, 80, "420") == [(0, 0, False), (0, 4, False), (0, 8, False), (32, 0, True), (32, 8, True)]
    assert len(P.luma_tiles(400, 80, "420")) == 6  # 18 ragged columns: more than half a tile, a second wide one
    # the staged store of a narrow tile that ends one pixel row into its second block row
    assert P.staged_waves(120, 9, "444") == [(True, 0, 0, 360, 9)]
    assert P.staged_waves(256, 7, "444") == [(False, 0, 0, 768, 7)]


def test_expectations_restatement_equals_the_oracle_on_the_default_idct():
    """pixels_from_planes on the default IDCT's planes IS oracle.decode, for every sampling and both upsamplings of family A: the same
    function on helpers.ifast_idct's planes is then the fast-IDCT expectation"""
    seen = set()
    for c in P.family("A"):
        sub = P.sub_of(c.source)
        if (sub, c.fmt, c.fancy) in seen:
            continue
        seen.add((sub, c.fmt, c.fancy))
        j = P.jpeg(c.source)
        got = P.pixels_from_planes(oracle.decode_planes(j), P.info(c.source), c.fancy, c.fmt == "bgr")
        assert np.array_equal(got, P.expected(c)), c.name
        fast = P.expected(c, fast_idct=True)
        assert fast.shape == got.shape and np.abs(fast.astype(int) - got.astype(int)).max() <= 24, c.name
    assert len(seen) == 15


def test_predicted_kernel_flavours():
    a = P.family("A")
    n = P.luma_units(a)
    assert all(v > 0 for v in n[:2]) and n[2] == 0
    assert P.luma_units(P.family("B"))[2] > 0 and P.luma_units(P.family("C")) == [0, 0, 0] == P.luma_units(P.family("F"))
