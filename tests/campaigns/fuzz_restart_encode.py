"""Restart-interval output, GPU coder against host coder (dev tool, GPU box): random pictures, sizes, samplings, qualities, input
layouts, restart intervals (none, 1, a few MCUs, one MCU row, more than the picture has) and tables (Annex K or optimized), a few
flat or noisy pictures among them (short intervals; stuffed bytes in front of markers), coded by an encoder with gpu_huffman and
gpu_restart and by one without -- every file byte for byte equal, and every image taken by the GPU coder.

    fuzz_restart_encode.py [seed] [rounds]
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvimagecodec_amd.lowlevel import BatchEncoder  # noqa: E402
from nvimagecodec_amd.synth import synth_image  # noqa: E402

MCU = {"444": (8, 8), "422": (16, 8), "420": (16, 16), "440": (8, 16), "411": (32, 8), "410": (32, 16), "gray": (8, 8)}

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rng = random.Random(seed)
gpu, host = BatchEncoder(0, num_threads=16, gpu_huffman=True, gpu_restart=True), BatchEncoder(0, num_threads=16, gpu_huffman=False)
n, nbytes, nmarkers, t0 = 0, 0, 0, time.time()
for rnd in range(rounds):
    fmt = rng.choice(["rgb", "rgb", "bgr", "rgb_planar", "gray"])
    opt = rng.random() < 0.4
    feeds, subs, quals, rsts = [], [], [], []
    for _ in range(rng.choice([4, 12, 24])):
        big = rng.random() < 0.1
        w = rng.randrange(1000, 2600) if big else rng.choice([rng.randrange(1, 40), rng.randrange(40, 700)])
        h = rng.randrange(800, 1800) if big else rng.choice([rng.randrange(1, 40), rng.randrange(40, 500)])
        kind = rng.random()
        if kind < 0.1:  # flat: blocks of a few bits, many intervals per byte range
            im = np.full((h, w, 3), rng.randrange(256), np.uint8)
        elif kind < 0.25:  # noise: long blocks, 0xFF bytes everywhere
            im = np.random.default_rng(rng.randrange(1 << 30)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        else:
            im = synth_image(w, h, seed=rng.randrange(1 << 30))
        sub = "gray" if fmt == "gray" else rng.choice(["420", "422", "444", "440", "411", "410"])
        mcus_x, mcus_y = -(-w // MCU[sub][0]), -(-h // MCU[sub][1])
        rsts.append(min(65535, rng.choice([0, 1, 1, rng.randrange(2, 10), mcus_x, mcus_x * rng.randrange(1, 4), mcus_x * mcus_y,
                                           mcus_x * mcus_y + 1, rng.randrange(1, 65536), 65535])))
        subs.append(sub)
        quals.append(rng.choice([rng.randrange(1, 101), 100, 95, 90, 75]))
        if fmt == "gray":
            feeds.append(torch.from_numpy(np.ascontiguousarray(im[:, :, 1])).cuda())
        elif fmt.endswith("planar"):
            feeds.append(torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda())
        else:
            feeds.append(torch.from_numpy(np.ascontiguousarray(im[:, :, ::-1] if fmt == "bgr" else im)).cuda())
    got = gpu.encode(feeds, subsampling=subs, quality=quals, input_format=fmt, restart_interval=rsts, optimized_huffman=opt)
    assert gpu.stats()["gpu_entropy_images"] == len(feeds), ("routing", rnd)
    want = host.encode(feeds, subsampling=subs, quality=quals, input_format=fmt, restart_interval=rsts, optimized_huffman=opt)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, ("gpu vs host", seed, rnd, i, fmt, subs[i], quals[i], rsts[i], opt, tuple(feeds[i].shape))
    n += len(feeds)
    nbytes += sum(len(a) for a in got)
    nmarkers += sum(sum(a.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) for a in got)
    print("round %d ok: %d images (%.1f MB of files, about %d markers) so far, %.1f s" % (rnd, n, nbytes / 1e6, nmarkers, time.time() - t0), flush=True)
print("fuzz_restart_encode seed %d: %d rounds, %d images, every file equal to the host coder's" % (seed, rounds, n))
