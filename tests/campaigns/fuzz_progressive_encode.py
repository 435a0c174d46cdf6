"""Progressive output, GPU coder against host coder (dev tool, GPU box): random pictures, sizes, samplings, qualities and input layouts,
a few flat or sparse pictures among them (long EOB runs), coded with progressive=True by an encoder with gpu_huffman and one
without -- every file byte for byte equal, and every image taken by the GPU coder.

    fuzz_progressive_encode.py [seed] [rounds]
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

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rng = random.Random(seed)
gpu, host = BatchEncoder(0, num_threads=16, gpu_huffman=True), BatchEncoder(0, num_threads=16, gpu_huffman=False)
n, nbytes, t0 = 0, 0, time.time()
for rnd in range(rounds):
    fmt = rng.choice(["rgb", "rgb", "bgr", "rgb_planar", "gray"])
    feeds, subs, quals = [], [], []
    for _ in range(rng.choice([4, 12, 24])):
        big = rng.random() < 0.1
        w = rng.randrange(1000, 2600) if big else rng.choice([rng.randrange(1, 40), rng.randrange(40, 700)])
        h = rng.randrange(800, 1800) if big else rng.choice([rng.randrange(1, 40), rng.randrange(40, 500)])
        kind = rng.random()
        if kind < 0.1:  # flat: every AC coefficient zero, one EOB run per AC scan
            im = np.full((h, w, 3), rng.randrange(256), np.uint8)
        elif kind < 0.2:  # sparse detail on a flat field
            im = np.full((h, w, 3), 128, np.uint8)
            npts = rng.randrange(1, 40)
            ys, xs = [rng.randrange(h) for _ in range(npts)], [rng.randrange(w) for _ in range(npts)]
            im[ys, xs] = 255
        else:
            im = synth_image(w, h, seed=rng.randrange(1 << 30))
        sub = "gray" if fmt == "gray" else rng.choice(["420", "422", "444", "440", "411", "410"])
        subs.append(sub)
        quals.append(rng.choice([rng.randrange(1, 101), 100, 95, 90, 75]))
        if fmt == "gray":
            feeds.append(torch.from_numpy(np.ascontiguousarray(im[:, :, 1])).cuda())
        elif fmt.endswith("planar"):
            feeds.append(torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda())
        else:
            feeds.append(torch.from_numpy(np.ascontiguousarray(im[:, :, ::-1] if fmt == "bgr" else im)).cuda())
    got = gpu.encode(feeds, subsampling=subs, quality=quals, input_format=fmt, progressive=True)
    assert gpu.stats()["gpu_entropy_images"] == len(feeds), ("routing", rnd)
    want = host.encode(feeds, subsampling=subs, quality=quals, input_format=fmt, progressive=True)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, ("gpu vs host", seed, rnd, i, fmt, subs[i], quals[i], tuple(feeds[i].shape))
    n += len(feeds)
    nbytes += sum(len(a) for a in got)
    print("round %d ok: %d images (%.1f MB of files) so far, %.1f s" % (rnd, n, nbytes / 1e6, time.time() - t0), flush=True)
print("fuzz_progressive_encode seed %d: %d rounds, %d images, every file equal to the host coder's" % (seed, rounds, n))
