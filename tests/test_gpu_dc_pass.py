"""GPU: the DC pass of the GPU entropy stage (csrc/gpu_huffman.hip huff_dc_group_kernel) hands every lane whole MCUs of one component
-- two a lane, or one where a free fourth wave takes the second half of component 0 -- and runs one wave scan over the lane totals.
Pictures of one MCU row whose MCU counts sit on the seams of that mapping (a lane's pair, the 64 MCUs of a half, the 128 of a group,
two and three groups and one more), two-row pictures whose rows end inside a group, in every stock sampling layout, a three-component
frame of ten blocks per MCU, a [Y] [Cb] [Cr] multi-scan file, a restart-interval file (which takes huff_dc_kernel) and DC runs whose
predictor leaves int16 (the stored values wrap).  Every file must be decoded by the GPU entropy stage, none handed back to the host
decoder, and give the oracle's samples bit for bit."""
import functools

import numpy as np
import pytest

import oracle
from helpers import jpeg_from_coefficients as jc
from helpers import sequential_scans

pytestmark = pytest.mark.gpu

MCUS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385)
MAX_WIDTH = 3080
LAYOUTS = {"gray": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "440": [(1, 2), (1, 1), (1, 1)],
           "420": [(2, 2), (1, 1), (1, 1)], "411": [(4, 1), (1, 1), (1, 1)], "y42c11": [(4, 2), (1, 1), (1, 1)]}
TWO_ROWS = (("gray", 200), ("444", 70), ("444", 129), ("422", 65), ("411", 96))   # (layout, MCUs per row): two rows of 8 pixels
QUANT = [8] * 64


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


def _written(name, mcus_x, rows, seed):
    samp = LAYOUTS[name]
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    width, height = 8 * hmax * mcus_x - (seed % 3), 8 * vmax * rows     # (widths that end inside the last MCU as well)
    coef = jc.random_coefficients(np.random.default_rng(seed), width, height, samp, extreme=20, dense=3)
    return jc.write_baseline(width, height, samp, coef, [QUANT] * len(samp))


def _wrapping(samp, blocks):
    """One MCU row whose luma DC values climb by 2,047 a block beyond +32,767, come back, and go below -32,768: libjpeg keeps the
    predictor in an int and stores its low 16 bits."""
    hmax = max(h for h, _ in samp)
    width, height = 8 * blocks, 8 * max(v for _, v in samp)
    assert blocks % hmax == 0
    coef = [np.zeros((bh, bw, 64), dtype=np.int32) for bh, bw in jc.block_grid(width, height, samp)]
    steps = [2047] * 20 + [-2047] * 40 + [2047] * 20
    walk = np.cumsum([steps[k % len(steps)] for k in range(coef[0].shape[0] * coef[0].shape[1])])
    assert walk.max() > 32767 + 2047 and walk.min() < -32768 - 2047
    # (in MCU order: that is the order the differences are coded in)
    order = [(my * v + by, mx * h + bx) for h, v in samp[:1] for my in range(coef[0].shape[0] // v) for mx in range(coef[0].shape[1] // h)
             for by in range(v) for bx in range(h)]
    for (y, x), dc in zip(order, walk):
        coef[0][y, x, 0] = dc
        coef[0][y, x, 1] = 3
    return jc.write_baseline(width, height, samp, coef, [[1] * 64] * len(samp))


@functools.lru_cache(maxsize=None)
def _files():
    """{output format: [(name, file)]}"""
    from nvimagecodec_amd.synth import synth_image
    res = {"rgb": [], "y": [], "yuv_planar": []}
    seed = 100
    for name, samp in LAYOUTS.items():
        fmt = "y" if name == "gray" else "yuv_planar" if name == "y42c11" else "rgb"
        for m in MCUS:
            if 8 * max(h for h, _ in samp) * m <= MAX_WIDTH:
                seed += 1
                res[fmt].append(("%s, %d MCUs" % (name, m), _written(name, m, 1, seed)))
    for name, m in TWO_ROWS:
        seed += 1
        res["y" if name == "gray" else "rgb"].append(("%s, 2 rows of %d MCUs" % (name, m), _written(name, m, 2, seed)))
    photo = oracle.encode(synth_image(16 * 65, 16, seed=5), "420", 90)
    res["rgb"].append(("[Y] [Cb] [Cr], 65 MCUs", sequential_scans.recode(photo, [[0], [1], [2]])))
    res["rgb"].append(("[Y] [Cb Cr], 65 MCUs", sequential_scans.recode(photo, [[0], [1, 2]])))
    res["rgb"].append(("restart interval 3, 129 MCUs", oracle.encode(synth_image(16 * 129, 16, seed=6), "420", 90, restart_interval=3)))
    res["y"].append(("gray, DC beyond int16, 320 blocks", _wrapping(LAYOUTS["gray"], 320)))
    res["rgb"].append(("420, luma DC beyond int16", _wrapping(LAYOUTS["420"], 160)))
    res["rgb"].append(("411, luma DC beyond int16", _wrapping(LAYOUTS["411"], 96 * 4)))
    return res


def test_the_files_cover_the_seams():
    files = _files()
    assert sum(len(v) for v in files.values()) > 60
    for fmt, items in files.items():
        for name, data in items:
            info = oracle.read_info(data)
            assert info["width"] <= MAX_WIDTH and info["height"] <= 16, name


@pytest.mark.parametrize("fmt", ["rgb", "y", "yuv_planar"])
def test_mcu_counts_on_the_lane_seams(dec, fmt):
    import torch
    items = _files()[fmt]
    jpegs = [data for _, data in items]
    outs, st = dec.decode(jpegs, fmt=fmt, gpu_huffman=True)
    torch.cuda.synchronize()
    assert list(st) == [0] * len(jpegs)
    assert dec.stats()["gpu_entropy_images"] == len(jpegs)
    assert dec.host_fallbacks() == 0
    bad = []
    for (name, data), o in zip(items, outs):
        if fmt == "yuv_planar":
            same = all(np.array_equal(p.cpu().numpy(), r) for p, r in zip(o, oracle.decode_planes(data)))
        else:
            same = np.array_equal(o.cpu().numpy(), oracle.decode(data, oracle.FMT_GRAY if fmt == "y" else oracle.FMT_RGB))
        if not same:
            bad.append(name)
    assert not bad, bad
