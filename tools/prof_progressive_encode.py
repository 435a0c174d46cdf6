"""Progressive output of configs[2]'s inputs (256 x 1080p 4:2:0 q90, RGB in HBM -> SOF2 files in host memory) through Submit/Wait:
the GPU coder (progressive_encode.hip) and the host coder in turn within one process, images/s per repeat and their spread.

    prof_progressive_encode.py [reps]          both routes, alternating; one line per route and repeat, then min / median / max
    prof_progressive_encode.py kernels [N]     the GPU coder only, N batches: run under rocprofv3 --kernel-trace --stats
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nvimagecodec_amd.lowlevel import BatchEncoder  # noqa: E402
from nvimagecodec_amd.synth import synth_image  # noqa: E402

BATCH = 256


def pipelined(enc, imgs, gpu_huffman, batches):
    """batches x Submit/Wait with up to three batches in flight; seconds per batch."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(batches):
        enc.submit(imgs, "420", 90, "rgb", gpu_huffman=gpu_huffman, progressive=True)
        if i >= 2:
            enc.wait(fetch=False)
    for _ in range(min(2, batches)):
        enc.wait(fetch=False)
    return (time.perf_counter() - t0) / batches


def main():
    src = [torch.from_numpy(synth_image(1920, 1080, seed=s)).cuda() for s in range(4)]
    imgs = [src[i % 4] for i in range(BATCH)]
    enc = BatchEncoder(0, num_threads=16)
    if len(sys.argv) > 1 and sys.argv[1] == "kernels":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
        t = pipelined(enc, imgs, True, n)
        print("gpu coder: %.2f ms/batch = %.0f images/s" % (t * 1e3, BATCH / t), flush=True)
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    pipelined(enc, imgs, True, 3)  # every page sizes its arenas on first use
    pipelined(enc, imgs, False, 1)
    rates = {"gpu": [], "host": []}
    for r in range(reps):
        for name, gh, n in (("gpu", True, 6), ("host", False, 2)):
            t = pipelined(enc, imgs, gh, n)
            rates[name].append(BATCH / t)
            print("rep %d %-4s coder: %8.2f ms/batch = %7.0f images/s" % (r, name, t * 1e3, BATCH / t), flush=True)
    for name, v in rates.items():
        print("%-4s coder: images/s min %.0f median %.0f max %.0f over %d repeats" % (name, min(v), statistics.median(v), max(v), len(v)))
    print("ratio of the medians (gpu / host): %.1f" % (statistics.median(rates["gpu"]) / statistics.median(rates["host"])))


if __name__ == "__main__":
    main()
