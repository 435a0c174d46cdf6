"""Measurements of the lossless (SOF3) decoder on two workloads:

    gray16   256 pictures of 512 x 512, P = 16, Ps = 1, one component   (lossless_col0_kernel + lossless_rows_kernel)
    ps7      32 pictures of 2048 x 2048, P = 12, Ps = 7, one component   (lossless_wavefront_kernel)

For each: every kernel's time per batch from HIP events around a relaunch of that part alone (hipjpegDecodeLosslessBatchDeviceKernel),
with the stream kept busy in front so that the launch itself is not in the figure -- median, minimum and maximum of 20 rounds after
5 warm-ups; beside it, in the same run, a device-to-device copy of the same bytes (2 read + 2 written per sample); the host part of
the call (header checks + entropy stage on 16 threads, until the call returns) and the whole call until the stream is done, as
images/s; and libjpeg-turbo (the one Pillow ships, through the binding of tests/golden/make_golden_lossless.py) decoding the same
files in 16 processes.

    python tools/prof_lossless_decode.py --files DIR [--make] [--out profiles/lossless/prof_lossless_decode.json]

--gpu-entropy measures the GPU entropy stage instead: both workloads with the flag off and with the flag on, in the
same process -- host part of the call, bytes of the host-to-device copies, the entropy kernels' parts (which = 3: destuffing and
synchronisation, which = 4: the write pass) and the whole call -- into profiles/lossless/prof_lossless_gpu_entropy.json.

--make writes the workload files into DIR (a few distinct pictures per workload; the batch repeats them) and stops: the writer is
numpy and slow, so this is done once, away from the GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

WORKLOADS = {
    "gray16": dict(batch=256, distinct=8, height=512, width=512, precision=16, ps=1, which=1, kernel="lossless_col0_kernel + lossless_rows_kernel"),
    "ps7": dict(batch=32, distinct=2, height=2048, width=2048, precision=12, ps=7, which=2, kernel="lossless_wavefront_kernel"),
}
THREADS = 16
ROUNDS, WARMUPS = 20, 5


def make_files(directory):
    from helpers import lossless_files as LF
    os.makedirs(directory, exist_ok=True)
    for name, w in WORKLOADS.items():
        for k in range(w["distinct"]):
            s = LF.random_samples(1000 + k, w["height"], w["width"], 1, w["precision"])
            data = LF.write_samples(s, w["precision"], w["ps"])
            open(os.path.join(directory, f"{name}_{k}.jpg"), "wb").write(data)
            print(name, k, len(data), "bytes", flush=True)


def load_files(directory, name):
    w = WORKLOADS[name]
    distinct = [open(os.path.join(directory, f"{name}_{k}.jpg"), "rb").read() for k in range(w["distinct"])]
    return [distinct[i % len(distinct)] for i in range(w["batch"])]


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4), "rounds": len(values)}


def _library_worker(args):
    directory, name, count = args
    import make_golden_lossless as G
    dec = G.Decoder()
    files = load_files(directory, name)[:count]
    dec.decode(files[0])
    best = None
    for _ in range(3):  # the best of three passes: the first ones still warm caches and clocks
        t0 = time.perf_counter()
        for f in files:
            dec.decode(f)
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best


def library_rate(directory, name):
    """images/s of libjpeg-turbo on the batch, cut into 16 shares, one process each (its best of three passes); the slowest share
    ends the batch"""
    import multiprocessing as mp
    batch = WORKLOADS[name]["batch"]
    share = max(1, batch // THREADS)
    procs = min(THREADS, batch)
    with mp.get_context("spawn").Pool(procs) as pool:
        times = pool.map(_library_worker, [(directory, name, share)] * procs)
    return round(share * procs / max(times), 1), {"processes": procs, "images_per_process": share, "slowest_s": round(max(times), 4)}


def measure(directory, name):
    import torch
    from nvimagecodec_amd import lowlevel
    w = WORKLOADS[name]
    files = load_files(directory, name)
    dec = lowlevel.BatchLosslessDecoder(device=0, num_threads=THREADS)
    info = lowlevel.lossless_info(files[0])
    outs = [dec.allocate(info) for _ in files]
    samples = w["batch"] * w["height"] * w["width"]
    src = torch.empty(samples, dtype=torch.int16, device="cuda:0")
    dst = torch.empty_like(src)
    busy = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0")

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        busy.fill_(1)  # the stream is busy while the host queues what follows
        busy.fill_(2)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    host_s, call_s = [], []
    for r in range(WARMUPS + 6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        statuses, _ = dec.decode(files, outs=outs)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert not any(statuses)
        if r >= WARMUPS:
            host_s.append(t1 - t0)
            call_s.append(t2 - t0)
    stats = dec.stats()
    kernel, copy, upload = [], [], []
    for r in range(WARMUPS + ROUNDS):
        k = timed(lambda: dec.device_stage(w["which"]))
        c = timed(lambda: dst.copy_(src))
        u = timed(lambda: dec.device_stage(0))
        if r >= WARMUPS:
            kernel.append(k)
            copy.append(c)
            upload.append(u)
    want = outs[0].cpu().numpy()
    dec.device_stage(w["which"])
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), want)
    dec.close()
    bytes_moved = samples * 4
    result = {
        "workload": {k: w[k] for k in ("batch", "height", "width", "precision", "ps")}, "kernel": w["kernel"], "stats": stats,
        "file_bytes_per_batch": sum(len(f) for f in files),
        "kernel_ms": summary(kernel), "d2d_copy_ms": summary(copy), "upload_ms": summary(upload),
        "kernel_GBps_2_read_2_written": round(bytes_moved / statistics.median(kernel) / 1e6, 1),
        "d2d_copy_GBps": round(bytes_moved / statistics.median(copy) / 1e6, 1),
        "kernel_over_copy": round(statistics.median(kernel) / statistics.median(copy), 2),
        "host_stage_images_per_s": round(w["batch"] / statistics.median(host_s), 1), "host_threads": THREADS,
        "whole_call_images_per_s": round(w["batch"] / statistics.median(call_s), 1),
        "whole_call_ms": summary([s * 1e3 for s in call_s]), "host_stage_ms": summary([s * 1e3 for s in host_s]),
    }
    return result


def measure_gpu_entropy(directory, name):
    """flag off, then flag on, in this process: {"flag_off": ..., "flag_on": ...}; the outputs of the two must be the same bytes"""
    import torch
    from nvimagecodec_amd import lowlevel
    w = WORKLOADS[name]
    files = load_files(directory, name)
    info = lowlevel.lossless_info(files[0])
    busy = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0")

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        busy.fill_(1)
        busy.fill_(2)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    result, first = {"workload": {k: w[k] for k in ("batch", "height", "width", "precision", "ps")}, "file_bytes_per_batch": sum(len(f) for f in files)}, None
    for key, flag in (("flag_off", False), ("flag_on", True)):
        dec = lowlevel.BatchLosslessDecoder(device=0, num_threads=THREADS, gpu_entropy=flag)
        outs = [dec.allocate(info) for _ in files]
        host_s, call_s = [], []
        for r in range(WARMUPS + 6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            statuses, _ = dec.decode(files, outs=outs)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert not any(statuses)
            if r >= WARMUPS:
                host_s.append(t1 - t0)
                call_s.append(t2 - t0)
        stats = dec.stats()
        r = {"stats": stats, "h2d_bytes": stats["h2d_bytes"], "host_part_ms": summary([s * 1e3 for s in host_s]),
             "whole_call_ms": summary([s * 1e3 for s in call_s]), "whole_call_images_per_s": round(w["batch"] / statistics.median(call_s), 1)}
        if flag:
            assert stats["host_fallback_images"] == 0, stats
            sync, write = [], []
            for k in range(WARMUPS + ROUNDS):
                a = timed(lambda: dec.device_stage(3))
                b = timed(lambda: dec.device_stage(4))
                if k >= WARMUPS:
                    sync.append(a)
                    write.append(b)
            r["destuff_and_sync_ms"] = summary(sync)
            r["write_pass_ms"] = summary(write)
        got = [outs[0].cpu().numpy(), outs[-1].cpu().numpy()]
        if first is None:
            first = got
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, got)), "flag on and flag off differ"
        dec.close()
        result[key] = r
    result["flag_on_over_flag_off_whole_call"] = round(result["flag_on"]["whole_call_ms"]["median"] / result["flag_off"]["whole_call_ms"]["median"], 2)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", required=True)
    ap.add_argument("--make", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lossless", "prof_lossless_decode.json"))
    ap.add_argument("--skip-library", action="store_true")
    ap.add_argument("--gpu-entropy", action="store_true")
    args = ap.parse_args()
    if args.make:
        make_files(args.files)
        return
    if args.gpu_entropy:
        out = {"tool": "tools/prof_lossless_decode.py --gpu-entropy", "rounds": ROUNDS, "warmups": WARMUPS, "call_rounds": 6, "host_threads": THREADS}
        for name in WORKLOADS:
            out[name] = measure_gpu_entropy(args.files, name)
            print(name, json.dumps(out[name]), flush=True)
        path = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "lossless", "prof_lossless_gpu_entropy.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump(out, open(path, "w"), indent=1)
        return
    out = {"tool": "tools/prof_lossless_decode.py", "rounds": ROUNDS, "warmups": WARMUPS}
    for name in WORKLOADS:
        r = measure(args.files, name)
        if not args.skip_library:
            rate, how = library_rate(args.files, name)
            r["libjpeg_turbo_images_per_s"] = rate
            r["libjpeg_turbo"] = how
            r["whole_call_over_library"] = round(r["whole_call_images_per_s"] / rate, 2)
            r["host_stage_over_library"] = round(r["host_stage_images_per_s"] / rate, 2)
        out[name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
