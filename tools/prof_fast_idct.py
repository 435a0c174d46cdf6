"""ISLOW vs IFAST (decoder option fast_idct) on configs[1] (256 x 1080p 4:2:0 baseline -> interleaved RGB).  Dev tool, GPU only.

  prof_fast_idct.py kernels {islow|ifast} [N]   one batch prepared with that flavour, its device stage (GPU entropy stage, K1, K2) run N
                                                times (default 20) -- run under
                                                rocprofv3 --kernel-trace --stats for the K1 (idct_plane*) / K2 (luma_color*) kernel times
  prof_fast_idct.py e2e [ROUNDS] [STEPS]        end-to-end images/s with the profiler off, the two flavours alternating ROUNDS times
                                                (default 4) over STEPS pipelined batches each (default 12, three in flight, GPU entropy
                                                stage, as bench.py takes configs[1]); prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

BATCH = 256


def batch():
    src, _ = bench.make_inputs()
    return [src[i % len(src)] for i in range(BATCH)]


def kernels(flavour, n):
    import torch
    from nvimagecodec_amd.lowlevel import BatchDecoder
    jpegs = batch()
    dec = BatchDecoder(0, bench.usable_cpus())
    outs = dec.allocate_outputs(jpegs)
    dec.host_stage(jpegs, outs, gpu_huffman=True, fast_idct=flavour == "ifast")  # K1 / K2 read the blocks the GPU entropy stage writes
    dec.transfer()
    torch.cuda.synchronize()
    for _ in range(n):
        dec.device_stage()
    torch.cuda.synchronize()
    dec.close()
    print("done", flavour, n)


def e2e(rounds, steps):
    import torch
    from nvimagecodec_amd.lowlevel import BatchDecoder
    jpegs = batch()
    dec = BatchDecoder(0, bench.usable_cpus())
    ring = [dec.allocate_outputs(jpegs) for _ in range(3)]

    def run(fast, k):
        for i in range(k):
            dec.submit(jpegs, ring[i % 3], fast_idct=fast)
            if i >= 2:
                dec.wait()
        for _ in range(min(k, 2)):
            dec.wait()
        torch.cuda.synchronize()

    res = {"islow": [], "ifast": []}
    for fast in (False, True):
        run(fast, 4)  # warm-up of both flavours
    for _ in range(rounds):
        for name, fast in (("islow", False), ("ifast", True)):
            t = time.perf_counter()
            run(fast, steps)
            res[name].append(round(steps * BATCH / (time.perf_counter() - t), 1))
    dec.close()
    print(json.dumps({"workload": "configs[1]: 256 x 1920x1080 4:2:0 q90 -> I_RGB, GPU entropy stage, three batches in flight",
                      "images_per_s": res, "median": {k: sorted(v)[len(v) // 2] for k, v in res.items()}}))


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    else:
        e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 4, int(sys.argv[3]) if len(sys.argv) > 3 else 12)
