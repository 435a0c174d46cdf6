"""Coefficient tensors <-> pixels on one MI355X with the batch of DESIGN 3.7 (256 x 1920x1080 4:2:0 q90, warm), all in one run:
 (0) parity at the timed size: every to_pixels output equals the file decode, every from_pixels tensor set the file route's;
 (a) coef_to_decoder_kernel next to coef_import_kernel and coef_from_coder_kernel next to coef_export_kernel -- each pair moves the
     same blocks, the sibling is the yardstick -- as medians of the library's own event brackets (HIPJPEG_DEBUG_TIMING) over several
     launches, the four kernels taking turns.  The brackets make the calls wait, so this part runs in a child process of its own
     (--kernels) and nothing else is measured there;
 (b) device time of a whole BatchCoefficients.to_pixels batch, events on the caller's stream around the call (the stream is kept
     busy in front of the first event, so that the interval holds the batch's kernels and not the host's planning), against
     coef_import_kernel's median from (a) + the pixel kernels of the file-decoded batch timed one family at a time
     (hipjpegDecodeBatchDeviceKernel 0, 1, 2);
 (c) images/s of to_pixels, from_pixels and from_pixels -> to_pixels, tensors and outputs allocated once and one synchronisation at
     the end of the timed window, next to the routes through files: BatchCoefficients.encode + BatchDecoder.decode and
     BatchEncoder.encode + BatchCoefficients.decode.
usage: python tools/prof_coefficient_pixels.py [--batch 256] [--steps 7]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("coef_export_kernel", "coef_import_kernel", "coef_to_decoder_kernel", "coef_from_coder_kernel")
PAIRS = (("coef_to_decoder_kernel", "coef_import_kernel"), ("coef_from_coder_kernel", "coef_export_kernel"))


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return f"median {median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f}, {len(v)} launches)"


def captured_stderr(fn):
    """runs fn() with stderr captured at the file-descriptor level -> its text"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def setup(batch):
    import torch

    import bench
    from nvimagecodec_amd import lowlevel
    src, what = bench.make_inputs()
    jpegs = [src[i % len(src)] for i in range(batch)]
    threads = bench.usable_cpus()
    c = lowlevel.BatchCoefficients(device=0, num_threads=threads, gpu_huffman=True)
    dec = lowlevel.BatchDecoder(device=0, num_threads=threads)
    info = lowlevel.coefficient_info(jpegs[0])
    tensors = [c.allocate(info) for _ in jpegs]
    statuses, images = c.decode(jpegs, outs=tensors)
    assert statuses == [0] * batch
    pixels, statuses = dec.decode(jpegs, gpu_huffman=True)  # the file decode: to_pixels' reference and from_pixels' input
    torch.cuda.synchronize()
    return what, jpegs, c, dec, images, pixels


def kernels_main(a):
    """the child process: HIPJPEG_DEBUG_TIMING is set, every bracketed call waits for its kernel"""
    import torch
    what, jpegs, c, dec, images, pixels = setup(a.batch)
    outs = [torch.empty_like(p) for p in pixels]
    from_outs = [c.allocate(images[0].info) for _ in jpegs]

    def turns():
        for _ in range(a.steps):
            c.decode(jpegs, outs=[im.coefs for im in images])
            c.encode(images, optimized_huffman=True)
            c.to_pixels(images, outs=outs)
            c.from_pixels(pixels, "420", 90, outs=from_outs)

    turns()  # warm
    torch.cuda.synchronize()
    text = captured_stderr(turns)
    ms = {k: [float(m) for m in re.findall(k + r": .* ([0-9.]+) ms", text)] for k in KERNELS}
    blocks = {k: sorted({int(m) for m in re.findall(k + r": \d+ workgroups, (\d+) blocks", text)}) for k in KERNELS}
    print("KERNELS " + json.dumps(dict(ms=ms, blocks=blocks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true", help="(internal) the child process of part (a)")
    a = ap.parse_args()
    assert a.steps >= 7, "at least seven launches each"
    if a.kernels:
        return kernels_main(a)
    import torch

    from nvimagecodec_amd import lowlevel
    assert torch.cuda.is_available(), "needs a GPU"
    assert "HIPJPEG_DEBUG_TIMING" not in os.environ, "the brackets make every call wait: only the child of part (a) runs with them"

    # ---- (a) in a fresh child process, before this one opens the device
    env = dict(os.environ, HIPJPEG_DEBUG_TIMING="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels", "--batch", str(a.batch), "--steps", str(a.steps)], env=env,
                           stdout=subprocess.PIPE, text=True, check=True, timeout=600)
    k = json.loads(next(line for line in child.stdout.splitlines() if line.startswith("KERNELS "))[len("KERNELS "):])

    what, jpegs, c, dec, images, pixels = setup(a.batch)
    print("inputs:", what, "x", a.batch)
    outs = [torch.empty_like(p) for p in pixels]
    from_outs = [c.allocate(images[0].info) for _ in jpegs]

    # ---- (0) parity at the timed size, before anything is timed
    statuses, _ = c.to_pixels(images, outs=outs)
    assert statuses == [0] * a.batch
    statuses, from_images = c.from_pixels(pixels, "420", 90, outs=from_outs)
    assert statuses == [0] * a.batch
    torch.cuda.synchronize()
    assert all(torch.equal(o, p) for o, p in zip(outs, pixels)), "to_pixels must give the file decode's pixels"
    enc = lowlevel.BatchEncoder(device=0, num_threads=c_threads(), gpu_huffman=True)
    files = enc.encode(pixels, "420", 90)
    statuses, file_route = c.decode(files)
    assert statuses == [0] * a.batch
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for im, ref in zip(from_images, file_route) for x, y in zip(im.coefs, ref.coefs)), \
        "from_pixels must give the file route's tensors"
    assert all(im.info["blocks_w"] == ref.info["blocks_w"] and im.info["blocks_h"] == ref.info["blocks_h"] for im, ref in zip(from_images, file_route))
    print(f"parity: {a.batch} to_pixels outputs equal the file decode, {a.batch} from_pixels tensor sets equal the file route's")

    # ---- (a) report
    for new, sibling in PAIRS:
        assert len(k["ms"][new]) == a.steps and len(k["ms"][sibling]) == a.steps, (new, len(k["ms"][new]), len(k["ms"][sibling]))
        assert k["blocks"][new] == k["blocks"][sibling] and len(k["blocks"][new]) == 1, (k["blocks"][new], k["blocks"][sibling])
        ratio = median(k["ms"][new]) / median(k["ms"][sibling])
        print(f"{sibling}: {spread(k['ms'][sibling])}, {k['blocks'][sibling][0]} blocks")
        print(f"{new}: {spread(k['ms'][new])}, {k['blocks'][new][0]} blocks; / {sibling} = {ratio:.3f} ({'within' if ratio <= 1.10 else 'MISSES'} 1.10)")

    # ---- (b) device time of a whole to_pixels batch
    stream = torch.cuda.current_stream(0)
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")

    def device_ms(fn):
        for _ in range(160):  # keeps the stream busy (some 40 ms) while Python marshals the batch and the host plans it
            ballast.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    whole = [device_ms(lambda: c.to_pixels(images, outs=outs)) for _ in range(a.steps + 1)][1:]
    dec.host_stage(jpegs, outs, gpu_huffman=True)
    dec.transfer()
    dec.device_stage(which=3)
    torch.cuda.synchronize()
    families = {}
    for _ in range(a.steps + 1):
        for which in (0, 1, 2):
            families.setdefault(which, []).append(device_ms(lambda: dec.device_stage(which=which)))
    families = {w: v[1:] for w, v in families.items()}
    pixel_sum = sum(median(v) for v in families.values())
    yard = median(k["ms"]["coef_import_kernel"]) + pixel_sum
    ratio = median(whole) / yard
    print(f"to_pixels, whole batch on the device: {spread(whole)}")
    print("pixel kernels of the file-decoded batch: " + "; ".join(f"family {w}: {spread(v)}" for w, v in families.items()))
    print(f"coef_import_kernel {median(k['ms']['coef_import_kernel']):.4f} + pixel kernels {pixel_sum:.4f} = {yard:.4f} ms; "
          f"to_pixels / that sum = {ratio:.3f} ({'within' if ratio <= 1.10 else 'MISSES'} 1.10)")

    # ---- (c) rates
    def rate(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return a.batch * a.steps / (time.perf_counter() - t0)

    def round_trip():
        _, ims = c.from_pixels(pixels, "420", 90, outs=from_outs)
        c.to_pixels(ims, outs=outs)

    def through_files_to_pixels():
        _, written = c.encode(images, optimized_huffman=False)
        dec.decode(written, outs=outs, gpu_huffman=True)

    def through_files_from_pixels():
        c.decode(enc.encode(pixels, "420", 90), outs=from_outs)

    r = dict(to_pixels=rate(lambda: c.to_pixels(images, outs=outs)), from_pixels=rate(lambda: c.from_pixels(pixels, "420", 90, outs=from_outs)),
             round_trip=rate(round_trip), files_to_pixels=rate(through_files_to_pixels), files_from_pixels=rate(through_files_from_pixels))
    print(f"images/s: to_pixels {r['to_pixels']:.0f} (BatchCoefficients.encode + BatchDecoder.decode: {r['files_to_pixels']:.0f}); "
          f"from_pixels {r['from_pixels']:.0f} (BatchEncoder.encode + BatchCoefficients.decode: {r['files_from_pixels']:.0f}); "
          f"from_pixels -> to_pixels {r['round_trip']:.0f}")
    enc.close()
    dec.close()
    c.close()


def c_threads():
    import bench
    return bench.usable_cpus()


if __name__ == "__main__":
    main()
