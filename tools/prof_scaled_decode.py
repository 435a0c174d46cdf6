#!/usr/bin/env python3
"""Device-stage time of a scaled decode (profiles/scaled_decode/).

256 images of 1920x1080 4:2:0 q90, built as bench.py builds them, bitstreams through the GPU entropy stage.  Five batches are planned once
-- denominators 1, 2, 4, 8 and 1 again, a decoder each -- and their device stages run in turn, forwards and backwards alternately, with
HIP events before the entropy stage, between it and the pixel kernels, and behind them.  Every batch is warmed up; the two denominator-1
batches give the spread.  Prints one JSON object and, with --out, writes it to a file.

  python tools/prof_scaled_decode.py --out profiles/scaled_decode/timing.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_scaled_decode.py --reps 3 --warmup 1      (per-kernel shares)"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from nvimagecodec_amd.lowlevel import BatchDecoder
    sources, origin = bench.make_inputs()
    jpegs = [sources[i % len(sources)] for i in range(bench.BATCH)]
    decs = []
    for label, denom in (("1", 1), ("2", 2), ("4", 4), ("8", 8), ("1 again", 1)):
        d = BatchDecoder(device=0, num_threads=16)
        scales = [denom] * len(jpegs)
        outs = d.allocate_outputs(jpegs, "rgb", None, scales)
        assert all(s == 0 for s in d.host_stage(jpegs, outs, "rgb", fancy=True, gpu_huffman=True, scales=scales))
        d.transfer()
        torch.cuda.synchronize()
        assert d.stats()["gpu_entropy_images"] == len(jpegs)
        decs.append((label, d, outs))

    def step(d, ev=None):
        if ev:
            ev[0].record()
        d.device_stage(which=6)  # GPU entropy stage
        if ev:
            ev[1].record()
        for which in (0, 1, 2):  # K1 + reduced IDCT, K2, colour kernels
            d.device_stage(which=which)
        if ev:
            ev[2].record()

    for _ in range(args.warmup):
        for _, d, _ in decs:
            step(d)
    torch.cuda.synchronize()
    events = {label: [] for label, _, _ in decs}
    for r in range(args.reps):
        for label, d, _ in (decs if r % 2 == 0 else decs[::-1]):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            step(d, ev)
            events[label].append(ev)
    torch.cuda.synchronize()
    res = {"workload": "256 x 1920x1080 4:2:0 q90, " + origin, "repeats": args.reps, "warmup": args.warmup, "ms_per_batch": {}}
    for label, evs in events.items():
        ent = sorted(e[0].elapsed_time(e[1]) for e in evs)
        pix = sorted(e[1].elapsed_time(e[2]) for e in evs)
        tot = sorted(e[0].elapsed_time(e[2]) for e in evs)
        res["ms_per_batch"][label] = {"device_stage_median": round(tot[len(tot) // 2], 4), "min": round(tot[0], 4), "max": round(tot[-1], 4),
                                      "entropy_median": round(ent[len(ent) // 2], 4), "pixel_median": round(pix[len(pix) // 2], 4)}
    for label, d, outs in decs:  # the batch cycles through eight sources: image i and image i + 8 are the same picture
        h = [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() for o in outs[:16]]
        assert h[:8] == h[8:16], label
        res["ms_per_batch"][label]["first_image_sha256"] = h[0][:16]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
