"""The sampling-layout goldens (tests/golden/make_golden_sampling.py) on the GPU: stock ratios with larger factors, 410V, factor 3, luma
below the maximum, Cb != Cr, one-component frames with factors above 1 and four-component frames that need each triangle filter.
Every accepted image is bit-exact against the oracle (pinned to libjpeg-turbo by tests/test_sampling_layouts.py); the set of declined
ones is exactly what a restatement of libjpeg-turbo's upsampler choice (helpers/sampling_goldens.py) says the decoder cannot match."""
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case
from helpers import ifast_idct
from helpers import sampling_goldens as G
from helpers.geometry import upright
from test_cmyk import _reference_rgb

pytestmark = pytest.mark.gpu

FORMATS = ["rgb", "bgr", "rgb_planar", "bgr_planar", "y", "yuv_planar"]
UNSUPPORTED = 3

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _STOCK = json.load(_f)["decode"]
# stock neighbours in the same batch: one file of each stock layout the luma and generic kernels take
NEIGHBOURS = [next(e for e in _STOCK if e["sub"] == s and e["pixels"] and e["width"] >= 40) for s in ("420", "422", "444", "440", "411", "gray")]


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    yield d
    d.close()


@pytest.fixture(scope="module")
def batch():
    """(jpegs, entries): the sampling goldens, the refused layouts and the stock neighbours interleaved"""
    items = [(G.jpeg(e), e) for e in G.ENTRIES]
    for k, e in enumerate(NEIGHBOURS):
        items.insert(1 + 17 * k, (load_decode_case(e)[0], dict(e, sampling=None)))
    items += [(G.jpeg(e), dict(e, refused=True)) for e in G.REFUSED]
    return [j for j, _ in items], [e for _, e in items]


def _cpu(o):
    return [p.cpu().numpy() for p in o] if isinstance(o, list) else o.cpu().numpy()


def _expected(jpeg, entry, fmt, fancy):
    ncomp = oracle.read_info(jpeg)["ncomp"]
    if fmt == "yuv_planar":
        return oracle.decode_planes(jpeg)
    if ncomp == 4:
        # the oracle's CMYK samples are libjpeg-turbo's (tests/test_sampling_layouts.py); the RGB step is the reference's
        rgb = _reference_rgb(oracle.decode_cmyk(jpeg), entry["kind"] != "plain") if fancy else oracle.decode(jpeg, fancy=False)
        if fmt == "y":
            r, g, b = [rgb[:, :, i].astype(np.float32) for i in range(3)]
            return (np.float32(0.299) * r + np.float32(0.587) * g + np.float32(0.114) * b).astype(np.uint8)
    elif fmt == "y":
        return oracle.decode(jpeg, oracle.FMT_GRAY, fancy=fancy)
    else:
        rgb = oracle.decode(jpeg, oracle.FMT_RGB, fancy=fancy)
    return {"rgb": rgb, "bgr": rgb[:, :, ::-1], "rgb_planar": rgb.transpose(2, 0, 1), "bgr_planar": rgb[:, :, ::-1].transpose(2, 0, 1)}[fmt]


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
@pytest.mark.parametrize("fancy", [True, False], ids=["fancy", "plain"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_mixed_batch(dec, batch, fmt, fancy, gpu_huffman):
    import torch
    jpegs, entries = batch
    outs, st = dec.decode(jpegs, fmt=fmt, fancy=fancy, gpu_huffman=gpu_huffman, check=False)
    torch.cuda.synchronize()
    declined = {e["name"] for e, s in zip(entries, st) if s == UNSUPPORTED and not e.get("refused")}
    want = {e["name"] for e in entries if e["sampling"] and not e.get("refused") and G.expected_unsupported(e, fmt, fancy)}
    assert declined == want, ("declined but expected to decode", sorted(declined - want), "decoded but expected to decline", sorted(want - declined))
    bad = []
    for j, e, o, s in zip(jpegs, entries, outs, st):
        if e.get("refused"):
            assert s != 0, e["name"]
            continue
        if e["name"] in want:
            continue
        assert s == 0, (e["name"], s)
        got, ref = _cpu(o), _expected(j, e, fmt, fancy)
        same = len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref)) if fmt == "yuv_planar" else np.array_equal(got, ref)
        if not same:
            bad.append(e["name"])
    assert not bad, bad


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
def test_routing(dec, gpu_huffman):
    """enlarged-factor layouts and gray frames reach the luma kernels, the others the replicating generic kernel, four components
    neither (planes + cmyk_color_kernel)"""
    import torch
    for e in G.ENTRIES:
        if e["width"] != 83:
            continue
        _, st = dec.decode([G.jpeg(e)], fmt="rgb", fancy=False, gpu_huffman=gpu_huffman)
        torch.cuda.synchronize()
        plane, luma, generic = dec.stats()["units"]
        samp = e["sampling"]
        if len(samp) == 4:
            assert plane > 0 and luma == 0 and generic == 0, e["name"]
        elif len(samp) == 1 or G.luma_kernel_layout(samp):
            assert luma > 0 and generic == 0, (e["name"], plane, luma, generic)
        else:
            assert luma == 0 and generic > 0 and plane > 0, (e["name"], plane, luma, generic)


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
def test_region_and_orientation(dec, gpu_huffman):
    by_name = {e["name"]: e for e in G.ENTRIES}
    picks = ["y22c12_83x61", "y31c11_83x61", "gray22_83x61", "y24c11_83x61"]
    windows = [(None, 6), ((5, 3, 70, 50), 1), ((17, 9, 40, 30), 5), ((1, 1, 82, 60), 8), ((0, 0, 9, 7), 3), ((30, 20, 83, 61), 2)]
    for fancy in (True, False):
        for name in picks:
            e = by_name[name]
            j = G.jpeg(e)
            fmt = "y" if len(e["sampling"]) == 1 else "rgb"
            full = oracle.decode(j, oracle.FMT_GRAY if fmt == "y" else oracle.FMT_RGB, fancy=fancy)
            W, H = e["width"], e["height"]
            outs, _ = dec.decode([j] * len(windows), fmt=fmt, fancy=fancy, gpu_huffman=gpu_huffman, transforms=windows)
            for (roi, o), g in zip(windows, _cpu(outs)):
                x0, y0, x1, y1 = roi or (0, 0, W, H)
                assert np.array_equal(g, upright(full[y0:y1, x0:x1], o)), (name, fancy, roi, o)


def _ifast_plain_rgb(jpeg, entry):
    """fast IDCT + replication + colour conversion: the decode without fancy upsampling under JDCT_IFAST (helpers/ifast_idct.py)"""
    samp, W, H = entry["sampling"], entry["width"], entry["height"]
    full = [G.replicate(p, fx, fy, W, H) for p, (fx, fy) in zip(ifast_idct.planes(jpeg), G.ratios(samp))]
    if len(samp) == 1:
        return np.repeat(full[0].astype(np.uint8)[:, :, None], 3, axis=2)
    if len(samp) == 3:
        return np.stack(full, axis=2).astype(np.uint8) if entry["kind"] == "rgb" else G.ycc_to_rgb(*full)
    cmyk = np.stack(full, axis=2).astype(np.uint8)
    if entry["kind"] == "adobe2":
        cmyk = np.dstack([255 - G.ycc_to_rgb(*full[:3]), cmyk[:, :, 3]])
    return _reference_rgb(cmyk, entry["kind"] != "plain")


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
def test_fast_idct(dec, batch, gpu_huffman):
    import torch
    jpegs, entries = batch
    keep = [i for i, e in enumerate(entries) if e["sampling"] and not e.get("refused")]
    jpegs, entries = [jpegs[i] for i in keep], [entries[i] for i in keep]
    rgb, st = dec.decode(jpegs, fmt="rgb", fancy=False, gpu_huffman=gpu_huffman, fast_idct=True)
    yuv, st2 = dec.decode(jpegs, fmt="yuv_planar", gpu_huffman=gpu_huffman, fast_idct=True, check=False)
    ys, st3 = dec.decode(jpegs, fmt="y", gpu_huffman=gpu_huffman, fast_idct=True, check=False)
    torch.cuda.synchronize()
    bad = []
    for j, e, o, p, y, s2, s3 in zip(jpegs, entries, rgb, yuv, ys, st2, st3):
        ref = ifast_idct.planes(j)
        if not np.array_equal(_cpu(o), _ifast_plain_rgb(j, e)):
            bad.append((e["name"], "rgb"))
        if s2 == 0 and not all(np.array_equal(a, b) for a, b in zip(_cpu(p), ref)):
            bad.append((e["name"], "yuv_planar"))
        if s3 == 0 and len(ref) != 4 and not np.array_equal(_cpu(y), ref[0]):
            bad.append((e["name"], "y"))
        assert (s2 == UNSUPPORTED) == G.expected_unsupported(e, "yuv_planar", True) and (s3 == UNSUPPORTED) == G.expected_unsupported(e, "y", True)
    assert not bad, bad


@pytest.mark.parametrize("gpu_huffman", [False, True], ids=["host_entropy", "gpu_entropy"])
@pytest.mark.parametrize("fmt", ["rgb", "bgr", "y"])
def test_four_components(dec, fmt, gpu_huffman):
    """every four-component layout against the reference's CMYK -> RGB step on libjpeg-turbo's own samples (Adobe and plain)"""
    import torch
    entries = [e for e in G.ENTRIES if len(e["sampling"]) == 4]
    jpegs = [G.jpeg(e) for e in entries]
    outs, st = dec.decode(jpegs, fmt=fmt, gpu_huffman=gpu_huffman)
    torch.cuda.synchronize()
    bad = [e["name"] for j, e, o in zip(jpegs, entries, outs) if not np.array_equal(_cpu(o), _expected(j, e, fmt, True))]
    assert not bad, bad
