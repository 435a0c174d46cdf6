"""Test helper (also run as a child process, so that the library's switches apply -- they are read once per process): one small batch
in which the three ways to a block's start position run side by side -- a 4:2:0 photograph (its records are copied), a flat picture
(more blocks start in a subsequence than a record holds: its subsequences are walked) and a restart-interval picture (walked, with the
interval check).  Decoded through the GPU entropy stage: all of them stay there, and the pixels are the oracle's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def batch():
    import numpy as np
    import oracle
    from nvimagecodec_amd.synth import synth_image
    flat = np.full((256, 384, 3), 90, np.uint8)
    return [oracle.encode(synth_image(320, 240, seed=31), "420", 90), oracle.encode(flat, "420", 90),
            oracle.encode(synth_image(200, 152, seed=32), "420", 85, restart_interval=3), oracle.encode(flat[:128, :136], "444", 75),
            oracle.encode(synth_image(264, 136, seed=33), "422", 90)]


def check(dec):
    import numpy as np
    import torch
    import oracle
    jpegs = batch()
    for rep in range(2):   # the second time on reused work buffers
        outs, st = dec.decode(jpegs, gpu_huffman=True)
        torch.cuda.synchronize()
        assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
        for k, (j, o) in enumerate(zip(jpegs, outs)):
            assert np.array_equal(o.cpu().numpy(), oracle.decode(j)), (rep, k)


def main():
    from nvimagecodec_amd.lowlevel import BatchDecoder
    dec = BatchDecoder(device=0, num_threads=4)
    check(dec)
    dec.close()
    print("positions ok")


if __name__ == "__main__":
    main()
