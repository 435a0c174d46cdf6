"""Restart-interval output of configs[2]'s inputs (256 x 1080p 4:2:0 q90, RGB in HBM -> files in host memory) through Submit/Wait
three deep: images/s of five cases in one process, alternating, each repeated so that the spread shows.

    a        no restart interval                                    (GPU coder)
    b        an interval of one MCU row (120 MCUs)                  (GPU coder)
    c        interval 1                                             (GPU coder)
    d        case b with optimized tables                           (GPU coder)
    e_row    case b through the host coder (gpu_restart=False)
    e_1      case c through the host coder

    prof_restart_encode.py [reps]              all cases, alternating; one line per case and repeat, then min / median / max
    prof_restart_encode.py kernels CASE [N]    case a, b or c only, N batches: run under rocprofv3 --kernel-trace --stats
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
ROW = 1920 // 16  # MCUs per row of a 1080p 4:2:0 picture
WINDOW = 1.2  # seconds per measurement
#        name: (restart interval, optimized tables, the GPU coder takes restart intervals)
CASES = {"a": (0, False, True), "b": (ROW, False, True), "c": (1, False, True), "d": (ROW, True, True), "e_row": (ROW, False, False),
         "e_1": (1, False, False)}


def pipelined(enc, imgs, rst, opt, seconds=0.0, batches=3):
    """Submit/Wait with up to three batches in flight, at least `batches` of them and until `seconds` have passed; -> (seconds per
    batch, window length)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    i = 0
    while i < batches or time.perf_counter() - t0 < seconds:
        enc.submit(imgs, "420", 90, "rgb", restart_interval=rst, optimized_huffman=opt, gpu_huffman=True)
        if i >= 2:
            enc.wait(fetch=False)
        i += 1
    for _ in range(min(2, i)):
        enc.wait(fetch=False)
    t = time.perf_counter() - t0
    return t / i, t


def main():
    src = [torch.from_numpy(synth_image(1920, 1080, seed=s)).cuda() for s in range(4)]
    imgs = [src[i % 4] for i in range(BATCH)]
    # with gpu_huffman on both: images with a restart interval go to the host coder unless gpu_restart is set
    enc = {True: BatchEncoder(0, num_threads=16, gpu_huffman=True, gpu_restart=True), False: BatchEncoder(0, num_threads=16, gpu_huffman=True)}
    if len(sys.argv) > 1 and sys.argv[1] == "kernels":
        rst, opt, gr = CASES[sys.argv[2]]
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 6
        t, _ = pipelined(enc[gr], imgs, rst, opt, batches=n)
        print("case %s: %.2f ms/batch = %.0f images/s" % (sys.argv[2], t * 1e3, BATCH / t), flush=True)
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    for name, (rst, opt, gr) in CASES.items():  # every page sizes its arenas on first use
        pipelined(enc[gr], imgs, rst, opt, batches=3)
    sizes = {}
    for name in ("a", "b", "c", "d"):
        rst, opt, gr = CASES[name]
        sizes[name] = len(enc[gr].encode(imgs[:1], "420", 90, "rgb", restart_interval=rst, optimized_huffman=opt)[0])
    print("file bytes of image 0: " + ", ".join("%s %d" % kv for kv in sizes.items()), flush=True)
    rates = {name: [] for name in CASES}
    for r in range(reps):
        for name, (rst, opt, gr) in CASES.items():
            t, window = pipelined(enc[gr], imgs, rst, opt, WINDOW)
            rates[name].append(BATCH / t)
            print("rep %d case %-5s: %8.2f ms/batch = %7.0f images/s (window %.2f s)" % (r, name, t * 1e3, BATCH / t, window), flush=True)
    for name, v in rates.items():
        print("case %-5s: images/s min %.0f median %.0f max %.0f over %d repeats" % (name, min(v), statistics.median(v), max(v), len(v)))


if __name__ == "__main__":
    main()
