"""Multi-scan sequential pictures on the GPU entropy stage: configs[1]'s batch (256 x 1920x1080 4:2:0 q90, the bench's seeded sources)
as single-scan files and re-coded as [Y] [Cb] [Cr] (tests/helpers/sequential_scans.py), timed three ways:
  (a) single-scan files, resident device step as bench.py times it (host + transfer once, then entropy stage + K1 + K2 between events)
  (b) the [Y] [Cb] [Cr] files, the same step
  (c) the [Y] [Cb] [Cr] files through the host entropy route, end to end (decode call + synchronize)
Prints one line per case (images/s, median and spread over the repetitions) and the ratios.
  python tools/prof_multiscan.py [reps]          the three cases
  python tools/prof_multiscan.py kernels [N]     case (b)'s device step N times, for rocprofv3 --kernel-trace --stats"""
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import sequential_scans as S  # noqa: E402
from nvimagecodec_amd import lowlevel  # noqa: E402
from nvimagecodec_amd.synth import synth_image  # noqa: E402

BATCH, SOURCES = 256, 8


def batches():
    from PIL import Image
    single = []
    for s in range(SOURCES):  # bench.py's configs[1] sources: seeds 1234.., Pillow (libjpeg-turbo) q90 4:2:0
        b = io.BytesIO()
        Image.fromarray(synth_image(1920, 1080, seed=1234 + s)).save(b, "JPEG", quality=90, subsampling=2)
        single.append(b.getvalue())
    multi = [S.recode(j, [[0], [1], [2]], coefficients=lowlevel.entropy_decode_host(j)[0]) for j in single]
    return [single[k % SOURCES] for k in range(BATCH)], [multi[k % SOURCES] for k in range(BATCH)]


def device_step(dec, jpegs, reps):
    """bench.py's configs[1] step on a batch whose bitstreams are resident: entropy stage enqueued (which=6), K1, K2 -- between events"""
    outs = dec.allocate_outputs(jpegs)
    dec.host_stage(jpegs, outs, gpu_huffman=True)
    dec.transfer()
    dec.device_stage(which=3)  # entropy stage + its verdicts: every picture decoded on the GPU, none handed to the host
    print("    %d pictures: %d on the GPU entropy stage" % (len(jpegs), dec.stats()["gpu_entropy_images"]))

    def step():
        dec.device_stage(which=6)
        dec.device_stage(which=0)
        dec.device_stage(which=1)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return times


def end_to_end(dec, jpegs, reps, gpu_huffman):
    outs = dec.allocate_outputs(jpegs)
    dec.decode(jpegs, outs=outs, gpu_huffman=gpu_huffman)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        dec.decode(jpegs, outs=outs, gpu_huffman=gpu_huffman)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return times


def line(name, times):
    rates = [BATCH / t for t in times]
    med = statistics.median(rates)
    print("%-48s %9.0f images/s  (median of %d; min %.0f max %.0f; %.3f ms per batch)" % (name, med, len(rates), min(rates), max(rates),
                                                                                          1e3 * statistics.median(times)))
    return med


def main():
    single, multi = batches()
    dec = lowlevel.BatchDecoder(0, num_threads=16)
    if len(sys.argv) > 1 and sys.argv[1] == "kernels":
        device_step(dec, multi, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    a = line("(a) single scan, resident device step", device_step(dec, single, reps))
    b = line("(b) [Y] [Cb] [Cr], resident device step", device_step(dec, multi, reps))
    c = line("(c) [Y] [Cb] [Cr], host entropy route, end to end", end_to_end(dec, multi, max(3, reps // 4), False))
    print("(b) / (c) = %.1fx   time (b) / time (a) = %.3f" % (b / c, a / b))
    dec.close()


if __name__ == "__main__":
    main()
