"""Every legal sampling layout beyond the seven a stock encoder writes (tests/golden/make_golden_sampling.py): the stock ratios with larger
factors, 410V, factor 3, luma below the maximum, Cb != Cr, one-component frames with factors above 1, four-component frames that need
each triangle filter.  Here, without a GPU: the coefficient writer, the oracle against libjpeg-turbo's pixels, the host entropy decoders
against the oracle, and what hipjpegGetImageInfo reports.  tests/test_gpu_sampling_layouts.py decodes the same files on the GPU."""
import hashlib

import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as jc
from helpers import sampling_goldens as G
from nvimagecodec_amd import _native, lowlevel

LAYOUTS = {}
for _e in G.ENTRIES:
    LAYOUTS.setdefault(_e["layout"], [tuple(s) for s in _e["sampling"]])

# hipjpegGetImageInfo names a layout by its ratios: the enlarged-factor ones by the stock name, the others UNKNOWN
NAMED = {"y21c21": "444", "y12c12": "444", "y22c12": "422", "y22c21": "440", "y24c11": "410V"}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _real_blocks(sampling, w, h, c):
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return -(-(-(-h * sampling[c][1] // vmax)) // 8), -(-(-(-w * sampling[c][0] // hmax)) // 8)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("variant", ["plain", "adobe", "restart"])
def test_writer_round_trip(layout, variant):
    """write_baseline puts the chosen coefficients where the oracle's decoder finds them: interleaved MCUs of every layout, a
    one-component frame non-interleaved over its real blocks, with an Adobe segment and with restart intervals"""
    samp = LAYOUTS[layout]
    for w, h in ((83, 61), (17, 9), (8, 8)):
        rng = np.random.default_rng(w * 1000 + h)
        coefs = jc.random_coefficients(rng, w, h, samp, 40, dc=200)
        kw = {"adobe": {1: None, 3: 1, 4: 2}[len(samp)]} if variant == "adobe" else {"restart_interval": 3} if variant == "restart" else {}
        jpeg = jc.write_baseline(w, h, samp, coefs, [np.full(64, 2 + c) for c in range(len(samp))], **kw)
        got, _ = oracle.decode_coefficients(jpeg)
        info = oracle.read_info(jpeg)
        assert (info["h"], info["v"]) == ([s[0] for s in samp], [s[1] for s in samp])
        assert info["restart_interval"] == (3 if variant == "restart" else 0)
        for c in range(len(samp)):
            want = np.asarray(coefs[c]).astype(np.int16)
            if len(samp) == 1:  # only the real blocks are coded; the padding of the grid decodes as zeros
                rows, cols = _real_blocks(samp, w, h, c)
                assert not got[c][rows:].any() and not got[c][:, cols:].any(), (w, h)
                want = want.copy()
                want[rows:] = 0
                want[:, cols:] = 0
            assert np.array_equal(got[c], want), (layout, w, h, c)


def test_writer_one_component_scan_is_non_interleaved():
    """a 2x2 gray frame of 8 x 8 pixels: one real block in a 2 x 2 grid, so the scan holds exactly one block"""
    coefs = [np.zeros((2, 2, 64), dtype=np.int32)]
    coefs[0][0, 0, 0] = 5
    one = jc.write_baseline(8, 8, [(2, 2)], coefs, [np.full(64, 1)])
    ref = jc.write_baseline(8, 8, [(1, 1)], [coefs[0][:1, :1]], [np.full(64, 1)])
    assert oracle.scan_bytes(one) == oracle.scan_bytes(ref)


def test_adobe_transform_sets_the_colour_model():
    samp3, samp4 = LAYOUTS["y21c21"], LAYOUTS["k22111122"]
    rng = np.random.default_rng(1)
    c3, c4 = jc.random_coefficients(rng, 17, 9, samp3, 5), jc.random_coefficients(rng, 17, 9, samp4, 5)
    q = [np.full(64, 4)] * 4
    model = {}
    for adobe in (None, 0, 1):
        model[3, adobe] = lowlevel.get_image_info(jc.write_baseline(17, 9, samp3, c3, q, adobe=adobe))["color_model"]
    for adobe in (None, 0, 2):
        model[4, adobe] = lowlevel.get_image_info(jc.write_baseline(17, 9, samp4, c4, q, adobe=adobe))["color_model"]
    assert model == {(3, None): 1, (3, 0): 2, (3, 1): 1, (4, None): 3, (4, 0): 3, (4, 2): 4}


def test_manifest_covers_the_layouts():
    assert set(LAYOUTS) >= {"y21c21", "y12c12", "y22c12", "y22c21", "y24c11", "y31c11", "y32c11", "y13c11", "y14c11", "y11c22",
                            "y22cb11cr21", "y21cb11cr21", "y41cb21cr11", "gray22", "gray12", "gray21", "gray44", "gray31",
                            "k22111122", "k12111112", "k22211211", "k11111122", "k31111131"}
    assert len([e for e in G.ENTRIES if e["progressive"]]) == 4 and len([e for e in G.ENTRIES if e["restart_interval"]]) == 2
    assert {e["kind"] for e in G.ENTRIES} == {"ycc", "gray", "rgb", "adobe0", "adobe2", "plain"}
    widths = {e["width"] for e in G.ENTRIES}
    assert max(widths) > 256 and min(widths) <= 4


def _oracle(entry, jpeg, fancy):
    n = len(entry["sampling"])
    if n == 4:
        return oracle.decode_cmyk(jpeg, fancy=fancy)
    return oracle.decode(jpeg, oracle.FMT_GRAY if n == 1 else oracle.FMT_RGB, fancy=fancy)


@pytest.mark.parametrize("entry", G.ENTRIES, ids=lambda e: e["name"])
def test_oracle_equals_libjpeg_turbo(entry):
    jpeg = G.jpeg(entry)
    assert _sha(_oracle(entry, jpeg, True)) == entry["sha256"]
    assert _sha(_oracle(entry, jpeg, False)) == entry["plain_sha256"]


def test_declines_cover_each_libjpeg_rule():
    """the goldens reach every rule of the restatement the GPU tests take their expected declines from: h2v1, h2v2 and h1v2 triangle
    filters in the replicated path, the downsampled_width <= 2 exception of h2v1 / h2v2, a luma below full size in `y`"""
    reasons = set()
    for e in G.ENTRIES:
        samp = e["sampling"]
        if len(samp) != 3 or G.luma_kernel_layout(samp):
            continue
        hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
        for h, v in samp:
            m = G.libjpeg_upsampler(h, v, hmax, vmax, -(-e["width"] * h // hmax), True)
            reasons.add((m, G.expected_unsupported(e, "rgb", True)))
    assert {("h2v1_fancy", True), ("h2v2_fancy", True), ("h1v2_fancy", True), ("h2v1", False), ("h2v2", False), ("int", False)} <= reasons
    assert any(G.expected_unsupported(e, "y", False) and e["kind"] == "ycc" for e in G.ENTRIES)


@pytest.mark.parametrize("entry", G.ENTRIES, ids=lambda e: e["name"])
def test_planes_replicated_are_the_plain_decode(entry):
    """decode_planes at each component's own size; replicated and colour-converted they are the decode without fancy upsampling
    (libjpeg replicates there, jdsample.c int_upsample / h2v1_upsample / h2v2_upsample, and jdmerge.c computes the same)"""
    jpeg = G.jpeg(entry)
    samp, W, H = entry["sampling"], entry["width"], entry["height"]
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    planes = oracle.decode_planes(jpeg)
    assert [p.shape for p in planes] == [(-(-H * v // vmax), -(-W * h // hmax)) for h, v in samp]
    full = [G.replicate(p, fx, fy, W, H) for p, (fx, fy) in zip(planes, G.ratios(samp))]
    if len(samp) == 1:
        want = full[0].astype(np.uint8)
    elif entry["kind"] == "rgb":
        want = np.stack(full, axis=2).astype(np.uint8)
    elif len(samp) == 3:
        want = G.ycc_to_rgb(*full)
    elif entry["kind"] == "adobe2":  # YCCK: jdcolor.c ycck_cmyk_convert
        want = np.dstack([255 - G.ycc_to_rgb(*full[:3]), full[3].astype(np.uint8)])
    else:
        want = np.stack(full, axis=2).astype(np.uint8)
    assert _sha(want) == entry["plain_sha256"]


@pytest.mark.parametrize("entry", G.ENTRIES, ids=lambda e: e["name"])
def test_host_entropy_decoders_give_the_oracles_coefficients(entry):
    jpeg = G.jpeg(entry)
    ref, qref = oracle.decode_coefficients(jpeg)
    host, qt = lowlevel.entropy_decode_host(jpeg)
    emu, _ = lowlevel.entropy_decode_gpu_algorithm_host(jpeg)
    assert len(host) == len(emu) == len(ref)
    for c in range(len(ref)):
        assert host[c].shape == ref[c].shape and emu[c].shape == ref[c].shape, c
        assert np.array_equal(host[c], ref[c]), ("host decoder", c)
        assert np.array_equal(emu[c], ref[c]), ("GPU algorithm on the host", c)
        assert np.array_equal(qt[c], qref[c]), c
    if not entry["progressive"] and not entry["restart_interval"]:
        sparse, _ = lowlevel.entropy_decode_host_sparse(jpeg)
        assert all(np.array_equal(s, r) for s, r in zip(sparse, ref))


@pytest.mark.parametrize("entry", G.ENTRIES, ids=lambda e: e["name"])
def test_image_info(entry):
    jpeg = G.jpeg(entry)
    info = lowlevel.get_image_info(jpeg)
    o = oracle.read_info(jpeg)
    samp = entry["sampling"]
    n = len(samp)
    assert (info["width"], info["height"], info["num_components"]) == (entry["width"], entry["height"], n)
    assert info["h"] == [s[0] for s in samp] and info["v"] == [s[1] for s in samp]
    assert (info["blocks_w"], info["blocks_h"]) == (o["bw"], o["bh"])
    assert (info["samp_w"], info["samp_h"]) == (o["dw"], o["dh"])
    assert info["restart_interval"] == entry["restart_interval"]
    name = "gray" if n == 1 else NAMED.get(entry["layout"]) if n == 3 else None
    want = {"410V": 7}.get(name, _native.CSS.get(name, -1))
    assert info["subsampling"] == want, (entry["layout"], info["subsampling"])
    assert info["color_model"] == {"gray": 0, "ycc": 1, "rgb": 2, "adobe0": 3, "plain": 3, "adobe2": 4}[entry["kind"]]


@pytest.mark.parametrize("entry", G.REFUSED, ids=lambda e: e["name"])
def test_refused_layouts(entry):
    """libjpeg refuses more than 10 blocks per MCU (JERR_BAD_MCU_SIZE) and fractional ratios (JERR_FRACT_SAMPLE_NOTIMPL).  The parser
    refuses the first; the second parses (its coefficients are well defined) and the decoder declines it (tests/test_gpu_sampling_layouts.py)"""
    jpeg = G.jpeg(entry)
    samp = entry["sampling"]
    if sum(h * v for h, v in samp) > 10:
        for f in (lowlevel.get_image_info, lowlevel.entropy_decode_host, lowlevel.entropy_decode_gpu_algorithm_host):
            with pytest.raises(_native.HipJpegError) as e:
                f(jpeg)
            assert e.value.status == 2, f  # BAD_JPEG
    else:
        hmax = max(h for h, _ in samp)
        assert any(hmax % h for h, _ in samp)
        assert lowlevel.get_image_info(jpeg)["subsampling"] == -1
        with pytest.raises(oracle.OracleError):
            oracle.decode(jpeg)
