"""The pixel stage's stores on every seam of tests/helpers/pixel_seams.py, decoded into framed arenas (tests/helpers/framed_outputs.py):
every output at a chosen offset and pitch of one byte arena, bit-exact against the oracle (the scaled cases: against libjpeg-turbo's
hashes of tests/golden/manifest_scaled.json), and EVERY other byte of the arena still the sentinel -- twice, with two sentinels, since a
stray byte can equal one of them.  One test per family plus one batch of everything; each family's batches carry a few cases of the other
families, so a store by one picture into another's frame is caught.  tests/test_pixel_seams.py (no GPU) proves that the cases sit where
they claim."""
import pytest

from helpers import framed_outputs as F
from helpers import pixel_seams as P
from helpers import scaled_goldens as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


_SCALED_FULL = {}


def _scaled_full(dec, case):
    """the whole scaled picture of a region case, decoded into a tight tensor and held to the manifest's hash"""
    import torch
    key = (case.source, case.scale)
    if key not in _SCALED_FULL:
        outs, _ = dec.decode([P.jpeg(case.source)], fmt="rgb", scales=[case.scale])
        torch.cuda.synchronize()
        got = outs[0].cpu().numpy()
        assert S.sha(got) == S.expected(S.by_name(case.source[1]), case.scale)[1], case.name
        _SCALED_FULL[key] = got
    return _SCALED_FULL[key]


def _run(dec, case_list, gpu_huffman=True, fast_idct=False):
    """One decode call per (format, upsampling) of the cases and per sentinel, all of the call's outputs in one arena.
    -> the K2 units per kernel flavour, summed over the calls of one sentinel."""
    import torch
    flavours = [0, 0, 0]
    for (fmt, fancy), group in P.groups(case_list).items():
        layout = F.Layout()
        for c in group:
            layout.add(c.name, c.fmt, P.output_shape(c), **c.place)
        jpegs = [P.jpeg(c.source) for c in group]
        transforms = [(c.roi, c.orientation) if P.has_transform(c) else None for c in group]
        scales = [c.scale for c in group]
        expected = [P.expected(c, fast_idct, _scaled_full(dec, c) if c.scale != 1 and P.has_transform(c) else None) for c in group]
        units = P.luma_units(group)
        for sentinel in F.SENTINELS:
            arena = F.Arena(layout, sentinel)
            _, statuses = dec.decode(jpegs, fmt=fmt, fancy=fancy, outs=arena.outs, gpu_huffman=gpu_huffman, fast_idct=fast_idct,
                                     transforms=transforms, scales=scales, check=False)
            torch.cuda.synchronize()
            what = (fmt, fancy, gpu_huffman, fast_idct, hex(sentinel))
            assert all(s == 0 for s in statuses), (what, [(c.name, s) for c, s in zip(group, statuses) if s])
            if gpu_huffman:
                assert dec.host_fallbacks() == 0, what
            # the tiles the host planned are the ones the restated arithmetic predicts, flavour by flavour
            assert dec.kernel_flavours()[1] == units, what
            try:
                arena.check(expected)
            except AssertionError as e:
                raise AssertionError("%s\n%s" % (what, e)) from None
        flavours = [a + b for a, b in zip(flavours, units)]
    return flavours


def _with_neighbours(letter):
    cases = P.family(letter)
    extra = []
    for fmt, fancy in P.groups(cases):
        extra += P.neighbours(letter, fmt, fancy)
    assert extra, letter
    return cases + extra


def test_family_a_staged_interleaved_store(dec):
    """All 16 residues of row_bytes for a narrow tile alone, a last wide tile and a narrow tile behind a wide one, both tiles exactly
    full, every nrows branch, every sampling K2 fuses on both tile shapes; as rgb (COMMON flavour), bgr and rgb without fancy
    upsampling (run-time flags); every offset modulo 16, pitches of 0 modulo 16 and odd.  GPU and host entropy stage, and the fast
    IDCT's kernels."""
    flavours = _run(dec, _with_neighbours("A"))
    assert flavours[0] > 0 and flavours[1] > 0
    _run(dec, P.family("A"), gpu_huffman=False)
    _run(dec, P.family("A"), fast_idct=True)


def test_family_b_planar_store(dec):
    """W % 8 != 0 with all planes 8-aligned (8-byte stores plus a byte-wise last block), an odd pitch (rows alternate between the two
    paths) and exactly one misaligned plane; a wide and a narrow tile each; rgb_planar / bgr_planar, fancy on and off."""
    flavours = _run(dec, _with_neighbours("B"))
    assert flavours[0] > 0 and flavours[2] > 0


def test_family_c_k1_stores_to_the_output(dec):
    """y of colour and gray files and yuv_planar of 4:2:0 / 4:2:2 / 4:4:4: an aligned base with a ragged last block, a misaligned base,
    a pitch that is no multiple of 8, components of more than one workgroup with a ragged last one, ragged 4:2:0 chroma planes."""
    _run(dec, _with_neighbours("C"))


def test_family_d_generic_and_cmyk_kernels(dec):
    """4:1:1 and 4:1:0 at widths 255, 256, 257 (one thread per pixel, 256 threads) and a CMYK and a YCCK golden, at padded pitches."""
    _run(dec, _with_neighbours("D"))


def test_family_e_geometry_pass_and_regions(dec):
    """All eight orientations into padded pitches at output widths 255 / 256 / 257 and heights 7 / 8 / 9, as rgb, rgb_planar and y; and
    regions whose tiles start at block column 32 and block row 4 with a narrow tile inside the picture, in every K2 flavour -- the unit
    counts pin the tiles the host planned for them."""
    _run(dec, _with_neighbours("E"))


def test_family_f_scaled_decode(dec):
    """Denominators 2, 4, 8 into rows that are 16-byte aligned with W % 16 != 0 (the wide loop AND its tail run, the tail ragged),
    4-byte aligned only, unaligned, planar with one misaligned plane; direct and upsampled pictures; rgb, bgr, rgb_planar, y; a turned
    region at a scale."""
    _run(dec, _with_neighbours("F"))


def test_everything_in_one_batch_per_format(dec):
    """Every case of every family, one arena per (format, upsampling); the three K2 flavours all get units."""
    flavours = _run(dec, list(P.cases()))
    assert all(v > 0 for v in flavours), flavours
    # and through the host entropy stage
    _run(dec, [c for c in P.cases() if c.family in "DE"], gpu_huffman=False)
