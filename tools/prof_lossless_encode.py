"""Where hipjpegEncodeLosslessBatch spends its time, against a device-to-device copy of the input and against libjpeg-turbo itself.

Two workloads, those of tools/prof_lossless_decode.py: 256 x 512x512 at P = 16, Ps = 1 and 32 x 2048x2048 at P = 12, Ps = 7, one
component, smooth content with noise.  Per workload, in a child process under its own time limit: 5 warm-up batches, then 20 measured
ones.  Of each batch: the ten stages of hipjpegEncodeLosslessBatchStageTimes (HIP events on the batch's stream: every kernel, the two
waits with the host work in them, the files' way into pinned memory), the whole call (HIP events around the call and the wait for its
last copy) and, in the same run, a device-to-device copy of the input bytes as the roofline yardstick.  Reported: median [min .. max].

The library: the compressor binding of tests/golden/make_golden_lossless_encode.py (the libjpeg-turbo that Pillow bundles) on the same
samples in 16 processes, each coding its share of the batch three times and reporting its best pass; the batch's time is the slowest
process's.  Skipped with --no-library, or where Pillow is missing (the JSON then says so).

    python tools/prof_lossless_encode.py [--out profiles/lossless/prof_lossless_encode.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "256x512x512_p16_ps1": dict(batch=256, height=512, width=512, precision=16, predictor=1),
    "32x2048x2048_p12_ps7": dict(batch=32, height=2048, width=2048, precision=12, predictor=7),
}
ROUNDS, WARMUP, PROCESSES, PASSES = 20, 5, 16, 3


def picture(w, index):
    """smooth ramp plus noise, as tests/helpers/lossless_files.py random_samples(smooth=True) makes it, over the whole range of P"""
    rng = np.random.default_rng(index)
    top = 1 << w["precision"]
    y, x = np.mgrid[0:w["height"], 0:w["width"]]
    return ((x * 3 + y * 5 + index * 7 + rng.integers(-2, 3, size=x.shape)) % top).astype(np.uint16)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def run_gpu(name):
    import torch
    from nvimagecodec_amd import _native as N
    from nvimagecodec_amd import lowlevel as LL
    w = WORKLOADS[name]
    host = np.stack([picture(w, i) for i in range(w["batch"])])
    dev = torch.from_numpy(host.view(np.int16)).cuda()
    twin = torch.empty_like(dev)
    enc = LL.BatchLosslessEncoder(device=0, num_threads=2)
    n = w["batch"]
    X = (N.LosslessEncodeInput * n)()
    P = (N.LosslessEncodeParams * n)()
    for i in range(n):
        X[i], comps = LL.lossless_encode_input(dev[i].data_ptr(), (w["height"], w["width"]), (w["width"] * 2, 2), 2, False)
        P[i] = N.LosslessEncodeParams(w["precision"], w["predictor"], 0, 0, 1)
    statuses = (ctypes.c_int * n)()
    L = N.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    stages = {k: [] for k in LL.BatchLosslessEncoder.STAGES}
    whole, copy, wall = [], [], []
    ptr, length = ctypes.c_void_p(), ctypes.c_size_t()
    file_bytes = 0
    for r in range(WARMUP + ROUNDS):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        st = L.hipjpegEncodeLosslessBatch(enc._h, X, P, n, statuses, stream)
        assert st == 0 and not any(statuses), (st, list(statuses))
        assert L.hipjpegEncodeLosslessGetBitstream(enc._h, n - 1, ctypes.byref(ptr), ctypes.byref(length)) == 0  # waits for the last copy
        b.record()
        twin.copy_(dev)
        c.record()
        torch.cuda.synchronize()
        if r < WARMUP:
            continue
        wall.append((time.perf_counter() - t0) * 1e3)
        whole.append(a.elapsed_time(b))
        copy.append(b.elapsed_time(c))
        for k, v in enc.stage_times().items():
            stages[k].append(v)
    for i in range(n):
        assert L.hipjpegEncodeLosslessGetBitstream(enc._h, i, ctypes.byref(ptr), ctypes.byref(length)) == 0
        file_bytes += length.value
    first = ctypes.string_at(ptr.value, length.value)
    assert np.array_equal(LL.decode_lossless_host(first)[:, :, 0], host[n - 1]), "the last file does not decode to its input"
    out = {"workload": w, "input_bytes": int(host.nbytes), "file_bytes": file_bytes, "stats": enc.stats(), "rounds": ROUNDS, "warmup": WARMUP,
           "stages_ms": {k: spread(v) for k, v in stages.items()}, "whole_call_ms": spread(whole), "whole_call_wall_ms": spread(wall),
           "device_to_device_copy_ms": spread(copy), "device": torch.cuda.get_device_name(0)}
    enc.close()
    print(json.dumps(out))


def library_worker(name, rank):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_lossless_encode as G
    w = WORKLOADS[name]
    mine = [picture(w, i)[:, :, None] for i in range(rank, w["batch"], PROCESSES)]
    best, size = None, 0
    for _ in range(PASSES):
        t0 = time.perf_counter()
        size = sum(len(G.compress(s, w["precision"], w["predictor"], 0, 0)) for s in mine)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    print(json.dumps({"rank": rank, "images": len(mine), "best_ms": best, "file_bytes": size}))


def run_library(name, limit):
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--library-worker", name, str(r)], stdout=subprocess.PIPE, text=True)
             for r in range(PROCESSES)]
    results = []
    for p in procs:
        out, _ = p.communicate(timeout=limit)
        assert p.returncode == 0, "a library process failed"
        results.append(json.loads(out.strip().splitlines()[-1]))
    return {"processes": PROCESSES, "passes": PASSES, "batch_ms": max(r["best_ms"] for r in results),
            "per_process_best_ms": spread([r["best_ms"] for r in results]), "file_bytes": sum(r["file_bytes"] for r in results)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lossless", "prof_lossless_encode.json"))
    ap.add_argument("--no-library", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=300)
    args = ap.parse_args()
    report = {"tool": "tools/prof_lossless_encode.py", "workloads": {}}
    try:
        from PIL import features
        report["libjpeg_turbo"] = features.version_feature("libjpeg_turbo")
    except ImportError:
        report["libjpeg_turbo"] = None
    for name in WORKLOADS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-step", name], capture_output=True, text=True, timeout=args.step_timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit("the GPU step of %s ended with %d: nothing further is started" % (name, r.returncode))
        entry = json.loads(r.stdout.strip().splitlines()[-1])
        if not args.no_library and report["libjpeg_turbo"]:
            entry["library"] = run_library(name, args.step_timeout)
            assert entry["library"]["file_bytes"] == entry["file_bytes"], "the library's files are not as long as the GPU's"
            entry["whole_call_vs_library"] = entry["library"]["batch_ms"] / entry["whole_call_ms"]["median"]
        entry["whole_call_vs_copy"] = entry["whole_call_ms"]["median"] / entry["device_to_device_copy_ms"]["median"]
        report["workloads"][name] = entry
        print(name, "whole call %.2f ms" % entry["whole_call_ms"]["median"], "copy %.3f ms" % entry["device_to_device_copy_ms"]["median"],
              "library %.1f ms" % entry["library"]["batch_ms"] if "library" in entry else "library not run", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(report, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    if "--gpu-step" in sys.argv:
        run_gpu(sys.argv[sys.argv.index("--gpu-step") + 1])
    elif "--library-worker" in sys.argv:
        i = sys.argv.index("--library-worker")
        library_worker(sys.argv[i + 1], int(sys.argv[i + 2]))
    else:
        main()
