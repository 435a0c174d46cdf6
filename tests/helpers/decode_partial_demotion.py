"""Test helper (run as a child process, because HIPJPEG_PROG_LDS_LIMIT is read once per process): one batch in which the planner has to hand
SOME progressive images to the host entropy stage to keep the walk / replay launches inside the LDS limit, and keep the others on the GPU.
The batch: the file with the largest walk launch there is (tests/helpers/progressive_seams.py LARGEST: 4 + 15 table slots of 2,560 entries and
11 rings, 119,808 bytes), two small progressive files with two AC scans and the Annex K tables (1,536 entries per slot), a baseline file.
With a limit of 65,536 bytes the first must go (its replay alone needs 40 KiB + 6 slots of 5,120 bytes), the others must stay."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import numpy as np
    import torch
    import oracle
    from conftest import GOLDEN, load_decode_case
    from helpers import jpeg_from_coefficients as jc
    from helpers import progressive_seams as S
    from nvimagecodec_amd.lowlevel import BatchDecoder
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        baseline = next(e for e in json.load(f)["decode"] if not e["progressive"] and e["width"] >= 33)
    small = []
    for seed, (w, h) in enumerate(((70, 45), (33, 17))):
        coefs = jc.random_coefficients(np.random.default_rng(seed), w, h, S.GRAY, 100, dense=8, small=4, dc=40)
        small.append(jc.write_progressive(w, h, S.GRAY, coefs, [np.full(64, 3, dtype=np.int32)], [("dc", [0]), ("ac", 0, 1, 5), ("ac", 0, 6, 63)]))
    jpegs = [S.get(S.LARGEST).jpeg, small[0], load_decode_case(baseline)[0], small[1]]
    dec = BatchDecoder(device=0, num_threads=2)
    outs, st = dec.decode(jpegs, fmt="rgb", gpu_huffman=True)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st), st
    taken = dec.stats()["gpu_entropy_images"]
    assert dec.host_fallbacks() == 0
    for i, (j, o) in enumerate(zip(jpegs, outs)):
        assert np.array_equal(o.cpu().numpy(), oracle.decode(j)), i
    dec.close()
    print("partial demotion ok: gpu_entropy_images", taken, "of", len(jpegs))


if __name__ == "__main__":
    main()
