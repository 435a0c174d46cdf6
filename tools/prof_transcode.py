"""Lossless transcode on one MI355X with the bench's batch (256 x 1920x1080 4:2:0 q90, files resident in host memory, warm):
 (a) coef_relayout_kernel: time per batch (the library's own event bracket, HIPJPEG_DEBUG_TIMING) and its bytes/time against a
     device-to-device copy of the same byte count in the same run;
 (b) images/s of hipjpegTranscodeBatch to optimized baseline and to progressive files, next to hipimtrans' decode -> encode route with
     the same output settings, one call outstanding (its decoding + encoding stage times, file reading and parsing left out);
 (c) with --orientation: coef_transform_kernel on the same batch turned for each of the given EXIF orientations (with trim: 1080 is no
     multiple of the 16-row iMCU), its time next to coef_relayout_kernel's of (a), per batch and per block moved.
 (d) with --crop WxH+X+Y (jpegtran's spelling; the origin on the 16x16 iMCU grid): coef_transform_kernel on the same batch cut to that
     region, as it is and brought upright for orientation 6, its time per carried block next to coef_relayout_kernel's of (a); and images/s
     of hipjpegTranscodeBatch for that crop next to the pixel route decode (the region through hipjpegDecodeBatchSetTransforms) -> encode
     of this library, optimized tables both ways.
usage: python tools/prof_transcode.py [--batch 256] [--steps 5] [--orientation 2,5,6] [--crop 1280x720+320+176] [--skip-pixel-route]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

os.environ["HIPJPEG_DEBUG_TIMING"] = "1"  # read once by the library: set before it loads
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from nvimagecodec_amd import _native as N  # noqa: E402
from nvimagecodec_amd import lowlevel  # noqa: E402


def kernel_times(fn):
    """runs fn() with stderr captured at the file-descriptor level; -> (result, [ms of every coef_relayout_kernel line],
    [ms of every coef_transform_kernel line])"""
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
    return res, *([float(m) for m in re.findall(kernel + r": .* ([0-9.]+) ms", text)] for kernel in ("coef_relayout_kernel", "coef_transform_kernel"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--orientation", default="", help="comma-separated EXIF orientations 2..8 to time coef_transform_kernel on")
    ap.add_argument("--crop", default="", help="WxH+X+Y: also time the batch cut to this region, orientation 1 and 6")
    ap.add_argument("--skip-pixel-route", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    src, what = bench.make_inputs()
    jpegs = [src[i % len(src)] for i in range(a.batch)]
    print("inputs:", what, "x", a.batch)
    t = lowlevel.BatchTranscoder(device=0, num_threads=bench.usable_cpus(), gpu_huffman=True)
    targets = {"optimized": dict(optimized_huffman=True), "progressive": dict(progressive=True)}
    for name, kw in targets.items():
        for _ in range(2):  # warm: arenas sized, code objects loaded
            statuses, files = t.transcode(jpegs, **kw)
        assert statuses == [0] * a.batch
        assert files[0] == lowlevel.transcode_host(jpegs[0], **kw), "the device route must write the host route's file"

        def timed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                t.transcode(jpegs, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        seconds, ms, _ = kernel_times(timed)
        st = t.stats()
        nbytes = st["relayout_blocks"] * 128
        print(f"[{name}] hipjpegTranscodeBatch: {a.batch * a.steps / seconds:.0f} images/s ({seconds / a.steps * 1e3:.2f} ms per batch; "
              f"GPU-decoded {st['gpu_decoded_images']}, GPU-coded {st['gpu_coded_images']}, output {sum(len(f) for f in files) / 1e6:.1f} MB per batch)")
        k = sorted(ms)[len(ms) // 2]
        print(f"[{name}] coef_relayout_kernel: median {k:.4f} ms per batch (min {min(ms):.4f}, max {max(ms):.4f}, {len(ms)} launches), {nbytes / 1e6:.1f} MB read + "
              f"as many written: {2 * nbytes / k / 1e6:.0f} GB/s of traffic")
    identity_ms, identity_blocks = k, st["relayout_blocks"]
    nbytes = identity_blocks * 128
    for orientation in [int(v) for v in a.orientation.split(",") if v]:
        kw = dict(optimized_huffman=True, orientation=orientation, trim=True)
        for _ in range(2):
            statuses, files = t.transcode(jpegs, **kw)
        assert statuses == [0] * a.batch
        assert files[0] == lowlevel.transcode_host(jpegs[0], **kw), "the device route must write the host route's file"

        def turned():
            for _ in range(a.steps):
                t.transcode(jpegs, **kw)

        _, ms_identity, ms = kernel_times(turned)
        assert not ms_identity and len(ms) == a.steps
        blocks = t.stats()["relayout_blocks"]
        m = sorted(ms)[len(ms) // 2]
        print(f"[orientation {orientation}] coef_transform_kernel: median {m:.4f} ms per batch (min {min(ms):.4f}, max {max(ms):.4f}, {len(ms)} launches), "
              f"{blocks} blocks ({blocks / identity_blocks:.4f} of the untrimmed batch): {2 * blocks * 128 / m / 1e6:.0f} GB/s of traffic; "
              f"/ coef_relayout_kernel = {m / identity_ms:.3f} per batch, {m / blocks / (identity_ms / identity_blocks):.3f} per block")
    if a.crop:
        w, h, x, y = (int(v) for v in re.fullmatch(r"(\d+)x(\d+)\+(\d+)\+(\d+)", a.crop).groups())
        region = (x, y, x + w, y + h)
        for orientation in (1, 6):
            kw = dict(optimized_huffman=True, orientation=orientation, trim=True, region=region)
            for _ in range(2):
                statuses, files = t.transcode(jpegs, **kw)
            assert statuses == [0] * a.batch
            assert files[0] == lowlevel.transcode_host(jpegs[0], **kw), "the device route must write the host route's file"

            def cropped():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    t.transcode(jpegs, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            seconds, ms_identity, ms = kernel_times(cropped)
            assert not ms_identity and len(ms) == a.steps
            blocks = t.stats()["relayout_blocks"]
            m = sorted(ms)[len(ms) // 2]
            print(f"[crop {a.crop}, orientation {orientation}] coef_transform_kernel: median {m:.4f} ms per batch (min {min(ms):.4f}, max {max(ms):.4f}, "
                  f"{len(ms)} launches), {blocks} blocks carried: {2 * blocks * 128 / m / 1e6:.0f} GB/s of traffic; per block / coef_relayout_kernel per block = "
                  f"{m / blocks / (identity_ms / identity_blocks):.3f}; hipjpegTranscodeBatch {a.batch * a.steps / seconds:.0f} images/s")
        if not a.skip_pixel_route:
            dec = lowlevel.BatchDecoder(device=0, num_threads=bench.usable_cpus())
            enc = lowlevel.BatchEncoder(device=0, num_threads=bench.usable_cpus(), gpu_huffman=True)
            transforms = [(region, 1)] * a.batch
            outs = dec.allocate_outputs(jpegs, "rgb", transforms)

            def pixel_route():
                dec.decode(jpegs, fmt="rgb", outs=outs, gpu_huffman=True, transforms=transforms)
                return enc.encode(outs, "420", 90, optimized_huffman=True)

            for _ in range(2):
                pixel_route()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                pixel_route()
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            print(f"[crop {a.crop}] decode with the region -> encode (4:2:0 q90, optimized tables, both entropy stages on the GPU): "
                  f"{a.batch * a.steps / seconds:.0f} images/s")
            dec.close()
            enc.close()
    # the same byte count through the copy engine's kernel path, same run
    a_dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b_dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b_dev.copy_(a_dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * 10)]
    for i in range(10):
        ev[2 * i].record()
        b_dev.copy_(a_dev)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    c = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(10))
    print(f"device-to-device copy of {nbytes / 1e6:.1f} MB: median {c[5]:.4f} ms (min {c[0]:.4f}, max {c[-1]:.4f}): {2 * nbytes / c[5] / 1e6:.0f} GB/s of traffic; "
          f"kernel / copy = {k / c[5]:.2f}")
    t.close()
    if a.skip_pixel_route:
        return
    tool = os.path.join(os.path.dirname(N.LIB_PATH), "hipimtrans")
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "in"))
        os.mkdir(os.path.join(d, "out"))
        for i, j in enumerate(jpegs):
            with open(os.path.join(d, "in", "img%04d.jpg" % i), "wb") as f:
                f.write(bytes(j))
        for name, extra in (("optimized", ["--optimized_huffman", "true"]), ("progressive", ["--jpeg_encoding", "progressive_dct"])):
            for lossless in (False, True):
                cmd = [tool, "-i", os.path.join(d, "in"), "-o", os.path.join(d, "out"), "-b", str(a.batch), "-w", "1", "-r", str(a.steps),
                       "-t", str(bench.usable_cpus())] + extra + (["--lossless"] if lossless else ["-q", "90", "-s", "420"])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    print("hipimtrans failed:", " ".join(cmd), p.stdout[-800:], p.stderr[-800:])
                    continue
                rate = lambda stage: float(re.search(r"Avg %s time per image: ([0-9.e-]+)" % stage, p.stdout).group(1))
                if lossless:
                    print(f"[{name}] hipimtrans --lossless: {1 / rate('lossless coding'):.0f} images/s in the call, {1 / rate('transcoding'):.0f} with file reading and writing")
                else:
                    print(f"[{name}] hipimtrans decode -> encode: {1 / (rate('decoding') + rate('encoding')):.0f} images/s (decoding {1 / rate('decoding'):.0f}, "
                          f"encoding {1 / rate('encoding'):.0f}), {1 / rate('transcoding'):.0f} with file reading, parsing and writing")


if __name__ == "__main__":
    main()
