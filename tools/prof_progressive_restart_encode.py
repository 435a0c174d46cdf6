"""Progressive output with restart intervals of configs[2]'s inputs (256 x 1080p 4:2:0 q90, RGB in HBM -> SOF2 files in host memory,
one MCU row per interval) through Submit/Wait: the GPU coder under gpu_progressive_restart (progressive_encode.hip, the RST flavour)
and the route without the flag -- gpu_huffman alone, which leaves these images to the host coder -- in turn within one process,
images/s per repeat and their spread.  A third case runs the GPU coder without intervals, for the cost of the intervals themselves.

    prof_progressive_restart_encode.py [reps] [interval]      the routes, alternating; one line per route and repeat, then min / median / max
    prof_progressive_restart_encode.py kernels [N] [interval] the GPU coder only, N batches: run under rocprofv3 --kernel-trace --stats

interval: MCUs per restart interval (default: one MCU row, 120).
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
ROW = 1920 // 16  # MCUs per row of 1080p 4:2:0


def pipelined(enc, imgs, interval, batches):
    """batches x Submit/Wait with up to three batches in flight; seconds per batch, images the GPU coder took of the last batch."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(batches):
        enc.submit(imgs, "420", 90, "rgb", restart_interval=interval, progressive=True)
        if i >= 2:
            enc.wait(fetch=False)
    for _ in range(min(2, batches)):
        enc.wait(fetch=False)
    return (time.perf_counter() - t0) / batches, enc.stats()["gpu_entropy_images"]


def main():
    args = sys.argv[1:]
    kernels = bool(args) and args[0] == "kernels"
    if kernels:
        args = args[1:]
    count = int(args[0]) if args else (6 if kernels else 3)
    interval = int(args[1]) if len(args) > 1 else ROW
    src = [torch.from_numpy(synth_image(1920, 1080, seed=s)).cuda() for s in range(4)]
    imgs = [src[i % 4] for i in range(BATCH)]
    gpu = BatchEncoder(0, num_threads=16, gpu_huffman=True, gpu_progressive_restart=True)
    if kernels:
        t, took = pipelined(gpu, imgs, interval, count)
        print("gpu coder, interval %d: %.2f ms/batch = %.0f images/s (%d images on the GPU coder)" % (interval, t * 1e3, BATCH / t, took), flush=True)
        return
    off = BatchEncoder(0, num_threads=16, gpu_huffman=True)  # the flag off: progressive + restart goes to the host coder
    cases = (("gpu", gpu, interval, 6, BATCH), ("flag_off", off, interval, 2, 0), ("gpu_r0", gpu, 0, 6, BATCH))
    for name, enc, r, n, _ in cases:  # every page sizes its arenas on first use
        pipelined(enc, imgs, r, 3 if n > 2 else 1)
    rates = {name: [] for name, *_ in cases}
    for rep in range(count):
        for name, enc, r, n, want in cases:
            t, took = pipelined(enc, imgs, r, n)
            assert took == want, (name, took)
            rates[name].append(BATCH / t)
            print("rep %d %-8s interval %5d: %8.2f ms/batch = %7.0f images/s" % (rep, name, r, t * 1e3, BATCH / t), flush=True)
    for name, v in rates.items():
        print("%-8s images/s min %.0f median %.0f max %.0f over %d repeats" % (name, min(v), statistics.median(v), max(v), len(v)))
    print("ratio of the medians (gpu / flag_off): %.1f" % (statistics.median(rates["gpu"]) / statistics.median(rates["flag_off"])))
    print("ratio of the medians (gpu / gpu_r0): %.2f" % (statistics.median(rates["gpu"]) / statistics.median(rates["gpu_r0"])))


if __name__ == "__main__":
    main()
