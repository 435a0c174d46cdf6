"""Coefficient tensors on one MI355X with the batch of DESIGN 3.7 (256 x 1920x1080 4:2:0 q90, files resident in host memory, warm):
 (a) coef_export_kernel and coef_import_kernel next to coef_relayout_kernel in the SAME run on the same batch -- the relayout kernel
     moves the same blocks and is the yardstick -- each as the median of the library's own event brackets (HIPJPEG_DEBUG_TIMING) over
     several launches, the three kernels taking turns so that clock and memory state are shared;
 (b) images/s of BatchCoefficients.decode, .encode and decode -> encode with the tensors staying on the device, next to
     hipjpegTranscodeBatch for the same target (optimized Huffman tables), all with both entropy stages on the GPU.
usage: python tools/prof_coefficients.py [--batch 256] [--steps 7]"""
import argparse
import os
import re
import sys
import tempfile
import time

os.environ["HIPJPEG_DEBUG_TIMING"] = "1"  # read once by the library: set before it loads
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from nvimagecodec_amd import lowlevel  # noqa: E402

KERNELS = ("coef_relayout_kernel", "coef_export_kernel", "coef_import_kernel")


def kernel_times(fn):
    """runs fn() with stderr captured at the file-descriptor level; -> (result, {kernel: [ms of every line it printed]})"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return res, {k: [float(m) for m in re.findall(k + r": .* ([0-9.]+) ms", text)] for k in KERNELS}


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    src, what = bench.make_inputs()
    jpegs = [src[i % len(src)] for i in range(a.batch)]
    print("inputs:", what, "x", a.batch)
    kw = dict(optimized_huffman=True)
    t = lowlevel.BatchTranscoder(device=0, num_threads=bench.usable_cpus(), gpu_huffman=True)
    c = lowlevel.BatchCoefficients(device=0, num_threads=bench.usable_cpus(), gpu_huffman=True)
    info = lowlevel.coefficient_info(jpegs[0])
    outs = [c.allocate(info) for _ in jpegs]  # the tensors are allocated once: the calls are timed, not torch's allocator
    for _ in range(2):  # warm: arenas sized, code objects loaded
        statuses, files = t.transcode(jpegs, **kw)
        assert statuses == [0] * a.batch
        statuses, images = c.decode(jpegs, outs=outs)
        assert statuses == [0] * a.batch
        statuses, written = c.encode(images, **kw)
        assert statuses == [0] * a.batch
    assert written == files, "the tensor route must write the transcode's files"
    host_info, host_coefs = lowlevel.decode_coefficients_host(jpegs[0])
    assert all(bool((x.cpu() == torch.from_numpy(y)).all()) for x, y in zip(images[0].coefs, host_coefs)), "the device route must read the host route's tensors"

    def kernels():
        for _ in range(a.steps):  # the three take turns
            t.transcode(jpegs, **kw)
            _, images = c.decode(jpegs, outs=outs)
            c.encode(images, **kw)

    _, ms = kernel_times(kernels)
    blocks = t.stats()["relayout_blocks"]
    assert c.stats()["moved_blocks"] == blocks
    base = median(ms["coef_relayout_kernel"])
    for k in KERNELS:
        v = ms[k]
        assert len(v) == a.steps, (k, len(v))
        print(f"{k}: median {median(v):.4f} ms per batch (min {min(v):.4f}, max {max(v):.4f}, {len(v)} launches), {blocks} blocks, "
              f"{2 * blocks * 128 / median(v) / 1e6:.0f} GB/s of traffic; / coef_relayout_kernel = {median(v) / base:.3f}")

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return a.batch * a.steps / (time.perf_counter() - t0)

    def round_trip():
        _, images = c.decode(jpegs, outs=outs)
        c.encode(images, **kw)

    (r_transcode, r_decode, r_encode, r_round), _ = kernel_times(lambda: (rate(lambda: t.transcode(jpegs, **kw)), rate(lambda: c.decode(jpegs, outs=outs)),
                                                                           rate(lambda: c.encode(images, **kw)), rate(round_trip)))
    st = c.stats()
    print(f"images/s (optimized tables; GPU-decoded {st['gpu_decoded_images']}, GPU-coded {st['gpu_coded_images']} of {a.batch}): decode {r_decode:.0f}, "
          f"encode {r_encode:.0f}, decode -> encode {r_round:.0f}, hipjpegTranscodeBatch {r_transcode:.0f}")
    t.close()
    c.close()


if __name__ == "__main__":
    main()
