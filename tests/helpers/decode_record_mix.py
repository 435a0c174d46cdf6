"""Test helper (run as a child process, so that the library's switches apply -- they are read once per process): one batch that
mixes bench-like photographs with pictures whose block-start records overflow (constant colour), periodic pictures (stripes: the
host decoder takes them), damaged streams and restart-interval streams.  Decoded through the GPU entropy stage and the host one:
same statuses, same pixels, and the oracle's pixels for every intact stream."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def batch():
    import numpy as np
    import oracle
    from nvimagecodec_amd.synth import synth_image
    photos = [oracle.encode(synth_image(1920, 1080, seed=s), "420", 90) for s in (1234, 1237, 1240)]
    flat = np.full((1080, 1920, 3), 90, np.uint8)
    stripes = np.full((1080, 1920, 3), 137, np.uint8)
    stripes[:, ::16] = 30
    wide = np.full((1080, 1920, 3), 137, np.uint8)
    wide[:, ::32] = 30
    intact = photos + [oracle.encode(flat, "420", 90), oracle.encode(flat, "444", 75), oracle.encode(stripes, "420", 90),
                       oracle.encode(wide, "420", 90),
                       oracle.encode(synth_image(640, 360, seed=3), "420", 90, restart_interval=1),
                       oracle.encode(synth_image(400, 300, seed=5), "420", 85, restart_interval=7),
                       oracle.encode(synth_image(1920, 1080, seed=9), "444", 95, restart_interval=120)]
    rng = random.Random(4242)
    damaged = []
    for n in range(9):
        b = bytearray(intact[n % 3] if n < 6 else intact[8 + n % 2])
        sos = bytes(b).rfind(b"\xff\xda") + 14
        if n % 3 == 0:
            for _ in range(rng.randrange(1, 6)):
                i = rng.randrange(sos, len(b) - 2)
                b[i] ^= 1 << rng.randrange(8)
        elif n % 3 == 1:
            i = rng.randrange(sos, len(b) - 40)
            for k in range(rng.randrange(1, 32)):
                b[i + k] = rng.randrange(256)
        else:
            b = b[: rng.randrange(sos + 1, len(b) - 2)] + b"\xff\xd9"
        damaged.append(bytes(b))
    return intact, damaged


def main():
    import numpy as np
    import torch
    import oracle
    from nvimagecodec_amd.lowlevel import BatchDecoder
    intact, damaged = batch()
    jpegs = [x for pair in zip(intact, damaged + [None] * len(intact)) for x in pair if x is not None]
    dec = BatchDecoder(device=0, num_threads=4)
    for rep in range(2):  # the second time on reused work buffers
        outs = dec.allocate_outputs(jpegs)
        _, st_gpu = dec.decode(jpegs, outs=outs, gpu_huffman=True, check=False)
        torch.cuda.synchronize()
        assert dec.stats()["gpu_entropy_images"] >= len(intact)
        got = [o.cpu().numpy().copy() for o in outs]
        _, st_cpu = dec.decode(jpegs, outs=outs, gpu_huffman=False, check=False)
        torch.cuda.synchronize()
        assert list(st_gpu) == list(st_cpu), (list(st_gpu), list(st_cpu))
        for i, (s, o) in enumerate(zip(st_cpu, outs)):
            if s == 0:
                assert np.array_equal(got[i], o.cpu().numpy()), i
        for j in intact:
            k = jpegs.index(j)
            assert st_gpu[k] == 0 and np.array_equal(got[k], oracle.decode(j)), k
    dec.close()
    print("records ok")


if __name__ == "__main__":
    main()
