"""GPU tests: sequential pictures whose components are coded in several scans, or in one scan in another component order
(helpers/sequential_scans.py), decoded by the GPU entropy stage -- one stream per scan -- must give exactly the pixels of the single-scan
originals, through every route, format and transform; damaged scans get the host route's statuses."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import sequential_scans as S
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = [[[0], [1], [2]], [[0], [1, 2]], [[1, 2], [0]], [[2], [1], [0]], [[2, 0, 1]]]

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _M = json.load(_f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _golden(e):
    with open(os.path.join(GOLDEN, "decode", e["name"] + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


def _sync():
    import torch
    torch.cuda.synchronize()


def _cpu(outs):
    return [o.cpu().numpy().copy() if not isinstance(o, (list, tuple)) else [p.cpu().numpy().copy() for p in o] for o in outs]


def _recoded():
    """(manifest entry, script, re-coded file) for every sequential colour golden with pixels"""
    out = []
    for e in _M["decode"]:
        if e["progressive"] or e["sub"] == "gray" or not e["pixels"]:
            continue
        for script in SCRIPTS:
            out.append((e, script, S.recode(_golden(e), script)))
    return out


def test_mixed_batch_counts_every_multiscan_picture(dec):
    """On a tree that sends several scans to the host stage, gpu_entropy_images falls short of this count."""
    rec = _recoded()
    neighbours = [_golden(e) for e in _M["decode"] if e["pixels"]]
    dec.decode(neighbours, gpu_huffman=True)
    _sync()
    neighbours_on_gpu = dec.stats()["gpu_entropy_images"]
    jpegs = [d for _, _, d in rec] + neighbours
    outs, statuses = dec.decode(jpegs, gpu_huffman=True)
    _sync()
    assert all(s == 0 for s in statuses)
    assert dec.stats()["gpu_entropy_images"] == len(rec) + neighbours_on_gpu
    assert dec.host_fallbacks() == 0
    for (e, script, _), o in zip(rec, outs):
        assert _sha(o.cpu().numpy()) == e["rgb_sha256"], (e["name"], script)


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "rgb_planar", "y", "yuv_planar"])
@pytest.mark.parametrize("fancy,fast_idct", [(True, False), (False, False), (True, True)])
def test_output_formats(dec, fmt, fancy, fast_idct):
    srcs = [oracle.encode(synth_image(w, h, seed=w), sub, 88) for w, h, sub in ((333, 201, "420"), (256, 128, "422"), (97, 65, "444"), (163, 90, "411"))]
    jpegs = [S.recode(j, script) for j in srcs for script in SCRIPTS]
    want = _cpu(dec.decode(jpegs, fmt=fmt, fancy=fancy, fast_idct=fast_idct, gpu_huffman=False)[0])
    got = _cpu(dec.decode(jpegs, fmt=fmt, fancy=fancy, fast_idct=fast_idct, gpu_huffman=True)[0])
    assert dec.stats()["gpu_entropy_images"] == len(jpegs)
    for w, g in zip(want, got):
        if isinstance(w, list):
            assert all(np.array_equal(a, b) for a, b in zip(w, g))
        else:
            assert np.array_equal(w, g)


def test_large_pictures_and_periodic_stream(dec):
    flat = np.full((1080, 1920, 3), 128, dtype=np.uint8)
    srcs = [oracle.encode(synth_image(1920, 1080, seed=1), "420", 90), oracle.encode(synth_image(3840, 2160, seed=2), "422", 92)]
    jpegs, refs = [], []
    for src in srcs:
        for restarts in (None, [8, 3, 5]):
            jpegs.append(S.recode(src, [[0], [1], [2]], restarts))
            refs.append(oracle.decode(src))
    flat_jpeg = oracle.encode(flat, "420", 90)
    jpegs.append(S.recode(flat_jpeg, [[0], [1], [2]]))
    refs.append(oracle.decode(flat_jpeg))
    outs, statuses = dec.decode(jpegs, gpu_huffman=True)
    _sync()
    assert all(s == 0 for s in statuses)
    assert dec.stats()["gpu_entropy_images"] == len(jpegs)
    for r, o in zip(refs, outs):
        assert np.array_equal(o.cpu().numpy(), r)


def test_regions_and_orientations(dec):
    src = oracle.encode(synth_image(301, 203, seed=7), "420", 90)
    transforms = [((0, 0, 301, 203), 1), ((17, 9, 100, 60), 1), (None, 6), ((33, 40, 120, 90), 8), (None, 3)]
    want = _cpu(dec.decode([src] * len(transforms), transforms=transforms, gpu_huffman=True)[0])
    for script in ([[0], [1], [2]], [[2, 0, 1]], [[1, 2], [0]]):
        j = S.recode(src, script)
        got = _cpu(dec.decode([j] * len(transforms), transforms=transforms, gpu_huffman=True)[0])
        assert all(np.array_equal(a, b) for a, b in zip(want, got)), script


def test_damaged_scans_get_the_host_route_statuses(dec):
    src = oracle.encode(synth_image(320, 240, seed=9), "420", 90)
    good = S.recode(src, [[0], [1], [2]])
    starts = [k for k in range(len(good) - 1) if good[k] == 0xFF and good[k + 1] == 0xDA]
    jpegs = [good]
    for s in starts[1:]:
        end = good.index(b"\xff\xda", s + 2) if s != starts[-1] else len(good) - 2
        mid = (s + end) // 2
        flipped = bytearray(good)
        for k in range(mid, mid + 24):
            if flipped[k] != 0xFF and flipped[k - 1] != 0xFF and flipped[k] ^ 0x24 != 0xFF:
                flipped[k] ^= 0x24
        jpegs.append(bytes(flipped))
        jpegs.append(good[:mid] + b"\xff\xd9")
    outs = dec.allocate_outputs(jpegs)
    _, st_gpu = dec.decode(jpegs, outs=outs, gpu_huffman=True, check=False)
    got = _cpu(outs)
    _, st_host = dec.decode(jpegs, outs=outs, gpu_huffman=False, check=False)
    want = _cpu(outs)
    assert list(st_gpu) == list(st_host)
    assert st_gpu[0] == 0 and np.array_equal(got[0], oracle.decode(src))
    for s, a, b in zip(st_host, got, want):
        if s == 0:
            assert np.array_equal(a, b)


def test_zero_copy_input(dec):
    import torch
    srcs = [oracle.encode(synth_image(640, 480, seed=s), "420", 90) for s in range(3)]
    jpegs = [S.recode(j, script) for j in srcs for script in ([[0], [1], [2]], [[1, 2], [0]])]
    pinned = [torch.frombuffer(bytearray(j), dtype=torch.uint8).pin_memory() for j in jpegs]
    outs, statuses = dec.decode(pinned, gpu_huffman=True)
    _sync()
    assert all(s == 0 for s in statuses)
    assert dec.stats()["zero_copy_images"] == len(jpegs)
    for j, o in zip(jpegs, outs):
        assert np.array_equal(o.cpu().numpy(), oracle.decode(j))


def test_submit_wait_and_plugin_routes(dec):
    import torch
    from nvimagecodec_amd import api
    srcs = [oracle.encode(synth_image(480, 320, seed=20 + s), "420", 90) for s in range(3)]
    jpegs = [S.recode(j, script) for j in srcs for script in SCRIPTS]
    refs = [oracle.decode(j) for j in srcs for _ in SCRIPTS]
    dec.set_pipeline_depth(3)
    batches = [jpegs[k::3] for k in range(3)]
    out_sets = [dec.allocate_outputs(b) for b in batches]
    for b, o in zip(batches, out_sets):
        dec.submit(b, o, gpu_huffman=True)
    for _ in batches:
        dec.wait()
    _sync()
    for k, o in enumerate(out_sets):
        for r, x in zip(refs[k::3], o):
            assert np.array_equal(x.cpu().numpy(), r)
    with api.Decoder(max_num_cpu_threads=4, options="hipjpeg_decoder:gpu_huffman=1") as d:
        imgs = d.decode(jpegs)
        torch.cuda.synchronize()
        for r, im in zip(refs, imgs):
            assert np.array_equal(np.asarray(im.cpu()._array), r)


FUSED_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np, torch, oracle
from helpers import sequential_scans as S
from nvimagecodec_amd.lowlevel import BatchDecoder
from nvimagecodec_amd.synth import synth_image
srcs = [oracle.encode(synth_image(640, 360, seed=s), "420", 90) for s in range(2)]
jpegs = srcs + [S.recode(j, sc) for j in srcs for sc in ([[0], [1], [2]], [[2, 0, 1]])]
dec = BatchDecoder(0, num_threads=2)
for rep in range(2):
    outs, st = dec.decode(jpegs, gpu_huffman=True)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st)
    assert dec.stats()["gpu_entropy_images"] == len(jpegs)
    for j, o in zip(jpegs, outs):
        assert np.array_equal(o.cpu().numpy(), oracle.decode(j))
only_single, st = dec.decode(srcs, gpu_huffman=True)
torch.cuda.synchronize()
assert dec.fused_units() > 0  # the switch is in effect for a batch of single-scan pictures
dec.close()
print("fused ok")
"""


def test_fused_builds_take_the_plain_path_for_multiscan_batches():
    env = dict(os.environ)
    env["HIPJPEG_FUSED_DECODE"] = "1"
    code = FUSED_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fused ok" in r.stdout
