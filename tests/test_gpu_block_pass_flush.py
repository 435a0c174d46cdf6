"""GPU: the end of a round of the block pass (csrc/gpu_huffman.hip, huff_blocks_kernel).  A team of 256 lanes decodes 256 blocks of
its unit (128 MCUs) per round into swizzled 128-byte LDS buffers; then every wave flushes its 64 buffers, eight lanes per block, each
lane fetching the destination of the block it stores from the lane that decoded it, and clears its buffers -- through the same swizzle
-- for the next round.  A lane without a block hands over a null destination and its buffer is not stored.  What can go wrong there
shows in the last round of a unit: 1, 7, 8, 9, 63, 64 and 65 blocks put the first absent destination at the start, the end and
the middle of an eight-lane flush group and of a wave; a round that is not the unit's first reads buffers the zero fill has cleared
(a chunk it missed keeps the coefficients of the round before).  Gray strips give every count (one block per MCU); 4:4:4, 4:2:0 (one
MCU in all, an odd number of MCU rows) and a two-scan file ([Y] [Cb Cr]) the counts their blocks per MCU allow, in first and later
rounds and in the second team's unit.  One batch mixes them with a 129-MCU strip, so that consecutive units belong to different images
and components; one puts small images behind a 1080p one, whose coefficients lie far from theirs.

The coefficient tensors of the GPU entropy stage must equal the host entropy stage's bit for bit, the pixels the oracle's, and no
image may be handed back to the host decoder."""
import numpy as np
import pytest

import oracle
from helpers import sequential_scans as Q
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

UNIT, ROUND = 128, 256        # MCUs of a unit (kHuffMcusPerWg), blocks of a round (kBTeamThreads)
COUNTS = (1, 7, 8, 9, 63, 64, 65)
MCU = {"420": (16, 16, 6), "444": (8, 8, 3), "gray": (8, 8, 1)}


def _image(sub, mcus_x, mcus_y, seed, quality=90):
    mw, mh, _ = MCU[sub]
    return oracle.encode(synth_image(mw * mcus_x, mh * mcus_y, seed=seed), sub, quality)


def _last_rounds(sub, mcus):
    """Blocks in the last round of every unit of a one-scan picture of `mcus` MCUs."""
    bpm = MCU[sub][2]
    units = [min(UNIT, mcus - first) * bpm for first in range(0, mcus, UNIT)]
    return [(items - 1) % ROUND + 1 for items in units]


# name -> (subsampling, MCU columns, MCU rows); the last rounds they give are asserted below
SHAPES = {}
for n in COUNTS:
    SHAPES["gray_%d" % n] = ("gray", n, 1)                 # unit 0, the only round: n blocks
    SHAPES["gray_128_%d" % n] = ("gray", UNIT + n, 1)      # the second team's unit: n blocks
SHAPES.update({
    "444_3": ("444", 3, 1),          # 9 blocks
    "444_21": ("444", 7, 3),         # 63 blocks, an odd number of MCU rows
    "444_88": ("444", 88, 1),        # 264: second round 8
    "444_107": ("444", 107, 1),      # 321: second round 65
    "444_128_21": ("444", 149, 1),   # units of 128 and 21 MCUs: 384 (second round 128) and 63
    "420_one_mcu": ("420", 1, 1),    # 6 blocks
    "420_44": ("420", 44, 1),        # 264: second round 8
    "420_96": ("420", 32, 3),        # 576: third round 64, three MCU rows
    "420_odd_rows": ("420", 20, 7),  # 140 MCUs in seven rows: units of 128 and 12 MCUs, 768 (three full rounds) and 72
})


def test_the_shapes_give_the_last_rounds_they_are_there_for():
    for n in COUNTS:
        assert _last_rounds("gray", n) == [n] and _last_rounds("gray", UNIT + n) == [UNIT, n]
    assert _last_rounds("444", 3) == [9] and _last_rounds("444", 21) == [63]
    assert _last_rounds("444", 88) == [8] and _last_rounds("444", 107) == [65] and _last_rounds("444", 149) == [128, 63]
    assert _last_rounds("420", 1) == [6] and _last_rounds("420", 44) == [8] and _last_rounds("420", 96) == [64]
    assert _last_rounds("420", 140) == [256, 72]
    for sub, mx, my in SHAPES.values():
        assert MCU[sub][2] * min(mx * my, UNIT) <= 3 * ROUND


@pytest.fixture(scope="module")
def files():
    """name -> JPEG file, made once: the shapes above, the two-scan files, a 129-MCU strip and a 1080p picture."""
    f = {name: _image(sub, mx, my, seed=300 + k) for k, (name, (sub, mx, my)) in enumerate(SHAPES.items())}
    # [Y] [Cb Cr] of 4:2:0: the luma scan's MCU is one block, the chroma scan's two.  21 x 3 MCUs: 252 luma blocks in two units (128 +
    # 124 blocks), 63 chroma MCUs = 126 blocks.  57 x 9 pixels, short of the MCU grid: the luma scan covers ceil(57 / 8) x ceil(9 / 8)
    # = 8 x 2 blocks, the chroma scan 4 x 1 MCUs = 8 blocks
    f["two_scans_21x3"] = Q.recode(_image("420", 21, 3, seed=390), [[0], [1, 2]])
    f["two_scans_57x9"] = Q.recode(oracle.encode(synth_image(57, 9, seed=391), "420", 90), [[0], [1, 2]])
    f["strip_129"] = _image("420", 129, 1, seed=392)
    f["large"] = oracle.encode(synth_image(1920, 1080, seed=393), "420", 90)
    return f


@pytest.fixture(scope="module")
def refs(files):
    """name -> (host entropy stage's coefficient planes, oracle's RGB pixels): computed once, left alone."""
    return {name: (lowlevel.decode_coefficients_host(j)[1], oracle.decode(j)) for name, j in files.items()}


@pytest.fixture(scope="module")
def handles():
    import torch
    assert torch.cuda.is_available()
    dec = lowlevel.BatchDecoder(0, num_threads=4)
    coef = lowlevel.BatchCoefficients(device=0, num_threads=4, gpu_huffman=True)
    yield dec, coef
    dec.close()
    coef.close()


def _check(handles, files, refs, names):
    import torch
    dec, coef = handles
    jpegs = [files[n] for n in names]
    statuses, images = coef.decode(jpegs)
    torch.cuda.synchronize()
    assert list(statuses) == [0] * len(jpegs)
    assert coef.stats()["gpu_decoded_images"] == len(jpegs)
    for n, im in zip(names, images):
        want = refs[n][0]
        assert len(im.coefs) == len(want), n
        for c, (g, w) in enumerate(zip(im.coefs, want)):
            g = g.cpu().numpy()
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), "%s: coefficients of component %d" % (n, c)
    outs, st = dec.decode(jpegs, gpu_huffman=True)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st)
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
    for n, o in zip(names, outs):
        got, want = o.cpu().numpy(), refs[n][1]
        assert got.shape == want.shape and np.array_equal(got, want), "%s: pixels" % n


@pytest.mark.parametrize("layout", ["gray", "gray_128", "444", "420", "two_scans"])
def test_last_rounds_of_each_layout(handles, files, refs, layout):
    """The files of one layout as a batch, in both orders: the unit behind an image's last belongs to another image."""
    names = [n for n in files if n.startswith(layout + "_") and (layout != "gray" or not n.startswith("gray_128_"))]
    assert len(names) >= 2
    _check(handles, files, refs, names)
    _check(handles, files, refs, names[::-1])


@pytest.mark.parametrize("name", ["gray_1", "gray_65", "444_107", "420_one_mcu", "420_odd_rows", "two_scans_57x9"])
def test_a_file_alone(handles, files, refs, name):
    """The grid's only working workgroup: nothing else has written near the image's coefficients."""
    _check(handles, files, refs, [name])


def test_every_layout_mixed_with_a_129_mcu_strip(handles, files, refs):
    """Every small file, a 129-MCU strip (two units: 768 blocks and 6) after every third: consecutive units belong to different images
    and components, and the rounds of one workgroup's two teams end at different counts."""
    small = [n for n in files if n not in ("large", "strip_129")]
    names = []
    for k, n in enumerate(small):
        names.append(n)
        if k % 3 == 2:
            names.append("strip_129")
    assert names.count("strip_129") >= 8
    _check(handles, files, refs, names)


def test_small_images_behind_a_large_one(handles, files, refs):
    """A 1080p picture (8,160 MCUs, 6 MB of coefficients) in front of files of one to nine blocks: the destinations of one batch lie
    megabytes apart."""
    _check(handles, files, refs, ["large", "gray_1", "444_3", "420_one_mcu", "gray_9", "large", "gray_128_7"])
