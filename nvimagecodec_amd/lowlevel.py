"""Thin Python front-end of the hipjpeg C-ABI (include/hipjpeg.h).  torch is used only as the owner of device
memory and streams; every pixel is produced by the HIP kernels in libhipjpeg_ext.so."""
import ctypes

import numpy as np

from . import _native as N

_FORMATS = {"rgb": N.OUTPUT_RGBI, "bgr": N.OUTPUT_BGRI, "rgb_planar": N.OUTPUT_RGB_PLANAR, "bgr_planar": N.OUTPUT_BGR_PLANAR,
            "y": N.OUTPUT_Y, "yuv_planar": N.OUTPUT_YUV_PLANAR}


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    if hasattr(data, "data_ptr") and hasattr(data, "numpy"):  # a torch CPU tensor: its memory, no copy
        return data.numpy()
    return np.frombuffer(bytes(data), dtype=np.uint8)


def entropy_decode_host_sparse(data):
    """The host entropy stage's zero-run-compressed stream of a picture, expanded again: per component int16 [blocks_h, blocks_w, 64] in
    NATURAL (row-major) order like entropy_decode_host + the stream's size in bytes.  Raises HipJpegError(UNSUPPORTED) for frames the format
    does not cover (progressive, several scans)."""
    a = _as_u8(data)
    info = get_image_info(data)
    nblocks = [bh * bw for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
    cap = sum(nblocks) * 200 + 64
    buf = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_size_t()
    toff = (ctypes.c_uint64 * 4)()
    st = N.load().hipjpegEntropyDecodeHostSparse(a.ctypes.data, a.size, buf.ctypes.data, cap, ctypes.byref(n), toff)
    if st:
        raise N.HipJpegError(st, "hipjpegEntropyDecodeHostSparse")
    tables = buf[: sum(nblocks) * 4].view(np.uint32)
    out = []
    for c, nb in enumerate(nblocks):
        blocks = np.zeros((nb, 64), dtype=np.int16)
        for b in range(nb):
            off = int(tables[int(toff[c]) + b])
            if off == 0:
                continue
            k = int(buf[off])
            blocks[b, 0] = np.frombuffer(buf[off + 1:off + 3].tobytes(), dtype="<i2")[0]
            for e in range(k):
                r = off + 3 + 3 * e
                blocks[b, int(buf[r])] = np.frombuffer(buf[r + 1:r + 3].tobytes(), dtype="<i2")[0]
        blk = blocks.reshape(info["blocks_h"][c], info["blocks_w"][c], 8, 8)  # device layout: [column][row]
        out.append(np.ascontiguousarray(blk.transpose(0, 1, 3, 2)).reshape(info["blocks_h"][c], info["blocks_w"][c], 64))
    return out, int(n.value)


def set_twin_scratch_fill(byte):
    """hipjpegTestSetScratchFill: the byte the host twins of the GPU algorithms fill their stand-ins for device scratch with
    (process-wide, 0 = the default; test hook)."""
    st = N.load().hipjpegTestSetScratchFill(int(byte))
    if st:
        raise N.HipJpegError(st, "hipjpegTestSetScratchFill")


def get_image_info(data):
    a = _as_u8(data)
    info = N.ImageInfo()
    st = N.load().hipjpegGetImageInfo(a.ctypes.data, a.size, ctypes.byref(info))
    if st:
        raise N.HipJpegError(st, "hipjpegGetImageInfo")
    nc = info.num_components
    d = {k: getattr(info, k) for k in ("width", "height", "num_components", "sof_marker", "color_model", "subsampling",
                                        "restart_interval", "num_scans", "coef_bytes")}
    for k in ("h", "v", "blocks_w", "blocks_h", "samp_w", "samp_h"):
        d[k] = list(getattr(info, k))[:nc]
    return d


def entropy_decode_host(data):
    """Host stage only (no GPU).  Returns (coefs, qtables): per component int16 [blocks_h, blocks_w, 64] and uint16[64],
    both converted back to NATURAL (row-major) order for easy comparison with the oracle."""
    a = _as_u8(data)
    info = get_image_info(a)
    buf = np.zeros(info["coef_bytes"] // 2, dtype=np.int16)
    offs = (ctypes.c_uint64 * 4)()
    qt = np.zeros(256, dtype=np.uint16)
    st = N.load().hipjpegEntropyDecodeHost(a.ctypes.data, a.size, buf.ctypes.data, buf.nbytes, ctypes.addressof(offs), qt.ctypes.data)
    if st:
        raise N.HipJpegError(st, "hipjpegEntropyDecodeHost")
    coefs, qts = [], []
    for c in range(info["num_components"]):
        n = info["blocks_w"][c] * info["blocks_h"][c]
        blk = buf[offs[c]: offs[c] + n * 64].reshape(info["blocks_h"][c], info["blocks_w"][c], 8, 8)
        coefs.append(np.ascontiguousarray(blk.transpose(0, 1, 3, 2)).reshape(info["blocks_h"][c], info["blocks_w"][c], 64))
        qts.append(np.ascontiguousarray(qt[c * 64:(c + 1) * 64].reshape(8, 8).T).reshape(64))
    return coefs, qts


def entropy_decode_gpu_algorithm_host(data):
    """The GPU entropy decoder's multi-pass algorithm emulated on the host (no GPU).  Returns (coefs natural order, sync passes)."""
    a = _as_u8(data)
    info = get_image_info(a)
    buf = np.zeros(info["coef_bytes"] // 2, dtype=np.int16)
    offs = (ctypes.c_uint64 * 4)()
    passes = ctypes.c_int32()
    st = N.load().hipjpegEntropyDecodeGpuAlgorithmHost(a.ctypes.data, a.size, buf.ctypes.data, buf.nbytes, ctypes.addressof(offs), ctypes.byref(passes))
    if st:
        raise N.HipJpegError(st, "hipjpegEntropyDecodeGpuAlgorithmHost")
    coefs = []
    for c in range(info["num_components"]):
        n = info["blocks_w"][c] * info["blocks_h"][c]
        blk = buf[offs[c]: offs[c] + n * 64].reshape(info["blocks_h"][c], info["blocks_w"][c], 8, 8)
        coefs.append(np.ascontiguousarray(blk.transpose(0, 1, 3, 2)).reshape(info["blocks_h"][c], info["blocks_w"][c], 64))
    return coefs, passes.value


def sync_schedule_counts(data):
    """hipjpegTestSyncScheduleCounts: what the first sync launch of the GPU entropy stage decodes, counted by the host twin (no GPU),
    which also checks that both schedules end in the Jacobi fixpoint's states and records.  Returns {"single": ..., "paired": ...}, each
    {"phases": [four counts of subsequence decodes], "tail": tasks left behind correction round 2}.  Test processes only."""
    a = _as_u8(data)
    counts = (ctypes.c_uint64 * 10)()
    fn = N.load().hipjpegTestSyncScheduleCounts   # (bound here, not in load(): an A/B library of an older commit has no such hook)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    st = fn(a.ctypes.data, a.size, ctypes.addressof(counts))
    if st:
        raise N.HipJpegError(st, "hipjpegTestSyncScheduleCounts")
    return {name: {"phases": [int(v) for v in counts[5 * k:5 * k + 4]], "tail": int(counts[5 * k + 4])} for k, name in enumerate(("single", "paired"))}


def entropy_decode_gpu_interval_algorithm_host(data):
    """The interval algorithm of gpu_progressive_intervals (a lane per restart interval, then the replay) emulated on the host (no GPU).
    Returns the coefficients in natural order; HipJpegError UNSUPPORTED for anything that is not a progressive file whose scans all have
    restart intervals the kernels take."""
    a = _as_u8(data)
    info = get_image_info(a)
    buf = np.zeros(info["coef_bytes"] // 2, dtype=np.int16)
    offs = (ctypes.c_uint64 * 4)()
    st = N.load().hipjpegEntropyDecodeGpuIntervalAlgorithmHost(a.ctypes.data, a.size, buf.ctypes.data, buf.nbytes, ctypes.addressof(offs))
    if st:
        raise N.HipJpegError(st, "hipjpegEntropyDecodeGpuIntervalAlgorithmHost")
    coefs = []
    for c in range(info["num_components"]):
        n = info["blocks_w"][c] * info["blocks_h"][c]
        blk = buf[offs[c]: offs[c] + n * 64].reshape(info["blocks_h"][c], info["blocks_w"][c], 8, 8)
        coefs.append(np.ascontiguousarray(blk.transpose(0, 1, 3, 2)).reshape(info["blocks_h"][c], info["blocks_w"][c], 64))
    return coefs


def _decode_flags(fancy, gpu_huffman, fast_idct, gpu_progressive_intervals=False):
    return ((N.FLAG_FANCY_UPSAMPLING if fancy else 0) | (N.FLAG_GPU_HUFFMAN if gpu_huffman else 0) | (N.FLAG_FAST_IDCT if fast_idct else 0) |
            (N.FLAG_GPU_PROGRESSIVE_INTERVALS if gpu_progressive_intervals else 0))


def scaled_image_size(width, height, scale_denom):
    """(width, height) of a picture decoded at 1 / scale_denom (1, 2, 4, 8): hipjpegGetScaledImageSize, host only."""
    w, h = ctypes.c_int32(), ctypes.c_int32()
    st = N.load().hipjpegGetScaledImageSize(int(width), int(height), int(scale_denom), ctypes.byref(w), ctypes.byref(h))
    if st:
        raise N.HipJpegError(st, "hipjpegGetScaledImageSize")
    return w.value, h.value


def output_shapes(jpegs, fmt="rgb", transforms=None, scales=None):
    """The shapes BatchDecoder.allocate_outputs gives its tensors (host only): per image a shape, a list of plane shapes (yuv_planar),
    or None for a file whose header cannot be read or whose scale denominator is none of 1, 2, 4, 8."""
    shapes = []
    for i, j in enumerate(jpegs):
        try:
            info = get_image_info(j)
            h, w = info["height"], info["width"]
            if scales is not None and scales[i] != 1:
                w, h = scaled_image_size(w, h, scales[i])
        except N.HipJpegError:
            shapes.append(None)
            continue
        if transforms is not None and transforms[i] is not None:
            roi, orientation = transforms[i]
            if roi is not None:
                w, h = roi[2] - roi[0], roi[3] - roi[1]
            if orientation >= 5:
                w, h = h, w
        if fmt in ("rgb", "bgr"):
            shapes.append((h, w, 3))
        elif fmt in ("rgb_planar", "bgr_planar"):
            shapes.append((3, h, w))
        elif fmt == "y":
            shapes.append((h, w))
        else:  # (hipjpegOutput_t holds three planes: four-component frames have no raw planes and are declined)
            shapes.append([(info["samp_h"][c], info["samp_w"][c]) for c in range(min(info["num_components"], 3))])
    return shapes


def _set_allocators(handle, allocators):
    """hipjpegSetAllocators on a fresh handle.  `allocators`: None, an _native.Allocators structure, or an object whose
    hipjpeg_allocators() returns one (it is kept alive with the handle: the library calls its functions until hipjpegDestroy)."""
    if allocators is None:
        return None
    table = allocators.hipjpeg_allocators() if hasattr(allocators, "hipjpeg_allocators") else allocators
    st = N.load().hipjpegSetAllocators(handle, ctypes.byref(table))
    if st:
        raise N.HipJpegError(st, "hipjpegSetAllocators")
    return (allocators, table)


class BatchDecoder:
    """hipjpegCreate / hipjpegDecodeBatch* on one device.  allocators (every Batch* class here takes it): see _set_allocators."""

    def __init__(self, device=0, num_threads=0, allocators=None):
        import torch
        self._torch = torch
        self.device = int(device)
        self._h = ctypes.c_void_p()
        st = N.load().hipjpegCreate(ctypes.byref(self._h), self.device, int(num_threads))
        if st:
            raise N.HipJpegError(st, "hipjpegCreate")
        self._allocators = _set_allocators(self._h, allocators)
        self._keep = None
        self._inflight = []

    def close(self):
        if self._h:
            N.load().hipjpegDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- output allocation mirrors python/decoder.cpp:179-225 of the reference: I_RGB u8, row_stride = w*3
    def allocate_outputs(self, jpegs, fmt="rgb", transforms=None, scales=None):
        """transforms: optional list with one entry per image, None or (roi, orientation) with roi = (x0, y0, x1, y1) or
        None and orientation = EXIF 1..8; the output then has the size of the region, turned upright.
        scales: optional list with one denominator per image (1, 2, 4, 8): the picture then has hipjpegGetScaledImageSize's size, and a
        region is in its coordinates."""
        torch = self._torch
        dev = torch.device("cuda", self.device)
        outs = []
        for shape in output_shapes(jpegs, fmt, transforms, scales):
            if shape is None:
                outs.append(None)
            elif isinstance(shape, list):
                outs.append([torch.empty(s, dtype=torch.uint8, device=dev) for s in shape])
            else:
                outs.append(torch.empty(shape, dtype=torch.uint8, device=dev))
        return outs

    def _marshal(self, jpegs, outs, fmt):
        n = len(jpegs)
        # a torch CPU tensor (uint8, contiguous) is taken where it lies -- in pinned memory (tensor.pin_memory()) the library then sends its
        # bitstream to the device without a staging copy (zero-copy input); everything else goes through numpy
        arrs = [j if (hasattr(j, "data_ptr") and hasattr(j, "numel")) else _as_u8(j) for j in jpegs]
        ptrs = (ctypes.c_void_p * n)(*[(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) for a in arrs])
        lens = (ctypes.c_size_t * n)(*[(a.numel() if hasattr(a, "numel") else a.size) for a in arrs])
        O = (N.Output * n)()
        for i, o in enumerate(outs):
            if o is None:
                continue
            if fmt in ("rgb", "bgr"):
                O[i].plane[0] = o.data_ptr()
                O[i].pitch[0] = o.stride(0)
            elif fmt in ("rgb_planar", "bgr_planar"):
                for p in range(3):
                    O[i].plane[p] = o[p].data_ptr()
                    O[i].pitch[p] = o.stride(1)
            elif fmt == "y":
                O[i].plane[0] = o.data_ptr()
                O[i].pitch[0] = o.stride(0)
            else:
                for p, t in enumerate(o):
                    O[i].plane[p] = t.data_ptr()
                    O[i].pitch[p] = t.stride(0)
        statuses = (ctypes.c_int * n)()
        self._keep = (arrs, ptrs, lens, O, outs)  # keep host inputs alive until the next call
        return ptrs, lens, O, statuses

    def _stream_ptr(self, stream):
        torch = self._torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def set_transforms(self, transforms, n):
        """Geometry for the next batch (see allocate_outputs); None clears it."""
        if transforms is None:
            st = N.load().hipjpegDecodeBatchSetTransforms(self._h, None, 0)
        else:
            T = (N.Transform * n)()
            for i, t in enumerate(transforms):
                if t is None:
                    T[i].orientation = 1
                    continue
                roi, orientation = t
                if roi is not None:
                    T[i].x0, T[i].y0, T[i].x1, T[i].y1 = [int(v) for v in roi]
                T[i].orientation = int(orientation)
            st = N.load().hipjpegDecodeBatchSetTransforms(self._h, T, n)
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchSetTransforms")

    def set_scales(self, scales, n):
        """Scale denominators (1, 2, 4, 8) for the next batch, one per image; None clears them."""
        if scales is None:
            st = N.load().hipjpegDecodeBatchSetScales(self._h, None, 0)
        else:
            st = N.load().hipjpegDecodeBatchSetScales(self._h, (ctypes.c_int32 * n)(*[int(v) for v in scales]), n)
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchSetScales")

    def decode(self, jpegs, fmt="rgb", fancy=True, outs=None, stream=None, check=True, gpu_huffman=False, transforms=None, fast_idct=False,
               gpu_progressive_intervals=False, scales=None):
        """Full pipeline.  Returns (outputs, statuses).  gpu_huffman=True: entropy-decode eligible streams on the GPU.
        gpu_progressive_intervals=True (with gpu_huffman): progressive files whose scans all have restart intervals too, a lane per interval.
        fast_idct=True: the fast integer IDCT (JDCT_IFAST of libjpeg-turbo's x86-64 SIMD routine) instead of the default ISLOW one.
        transforms: per-image (roi, orientation) or None -- region of interest and EXIF orientation applied on the device.
        scales: per-image denominator 1, 2, 4 or 8 -- decode at that fraction of the size (libjpeg's scale_denom)."""
        if outs is None:
            outs = self.allocate_outputs(jpegs, fmt, transforms, scales)
        if transforms is not None:
            self.set_transforms(transforms, len(jpegs))
        if scales is not None:
            self.set_scales(scales, len(scales))
        ptrs, lens, O, statuses = self._marshal(jpegs, outs, fmt)
        flags = _decode_flags(fancy, gpu_huffman, fast_idct, gpu_progressive_intervals)
        st = N.load().hipjpegDecodeBatch(self._h, ptrs, lens, len(jpegs), O, _FORMATS[fmt], flags, statuses, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatch")
        statuses = list(statuses)
        if check:
            for i, s in enumerate(statuses):
                if s:
                    raise N.HipJpegError(s, f"image {i}")
        return outs, statuses

    # -- pipelined: submit() returns once everything is queued; wait() returns the statuses of the oldest submitted batch.
    #    At most three batches in flight (set_pipeline_depth: up to eight).  The caller keeps jpegs and outs alive until the
    #    matching wait().
    def host_fallbacks(self):
        """Images of the last settled batch that the GPU entropy stage handed back to the host entropy decoder."""
        return int(N.load().hipjpegTestHostFallbacks(self._h))

    def kernel_flavours(self):
        """(plane_units[1], luma_units[3]) of the current batch: work units of K1 and of K2 per layout (hipjpegTestKernelFlavours)."""
        import ctypes
        a, b = (ctypes.c_int32 * 1)(), (ctypes.c_int32 * 3)()
        st = N.load().hipjpegTestKernelFlavours(self._h, a, b)
        if st:
            raise N.HipJpegError(st, "hipjpegTestKernelFlavours")
        return list(a), list(b)

    def set_hybrid_huffman_threshold(self, pixels):
        """gpu_huffman=True then applies to images of more than `pixels` pixels only (nvJPEG's hybrid_huffman_threshold); 0 = all."""
        st = N.load().hipjpegSetHybridHuffmanThreshold(self._h, ctypes.c_uint64(int(pixels)))
        if st:
            raise N.HipJpegError(st, "hipjpegSetHybridHuffmanThreshold")

    def fused_units(self):
        """Work units of the current batch that went to the FUSED kernel builds (HIPJPEG_FUSED_DECODE=1)."""
        return int(N.load().hipjpegTestFusedUnits(self._h))

    def set_pipeline_depth(self, depth):
        st = N.load().hipjpegSetPipelineDepth(self._h, int(depth))
        if st:
            raise N.HipJpegError(st, "hipjpegSetPipelineDepth")

    def submit(self, jpegs, outs, fmt="rgb", fancy=True, stream=None, gpu_huffman=True, fast_idct=False, gpu_progressive_intervals=False,
               scales=None):
        if scales is not None:
            self.set_scales(scales, len(scales))
        ptrs, lens, O, statuses = self._marshal(jpegs, outs, fmt)
        flags = _decode_flags(fancy, gpu_huffman, fast_idct, gpu_progressive_intervals)
        st = N.load().hipjpegDecodeBatchSubmit(self._h, ptrs, lens, len(jpegs), O, _FORMATS[fmt], flags, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchSubmit")
        self._inflight.append((len(jpegs), (ptrs, lens, O, jpegs, outs)))

    def wait(self, check=True):
        n, _keep = self._inflight.pop(0)
        statuses = (ctypes.c_int32 * n)()
        st = N.load().hipjpegDecodeBatchWait(self._h, statuses, n)
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchWait")
        statuses = list(statuses)
        if check:
            for i, s in enumerate(statuses):
                if s:
                    raise N.HipJpegError(s, f"image {i}")
        return statuses

    # -- the three phases separately (bench.py times device_stage with coefficients resident in HBM)
    def host_stage(self, jpegs, outs, fmt="rgb", fancy=True, gpu_huffman=False, fast_idct=False, gpu_progressive_intervals=False, scales=None):
        if scales is not None:
            self.set_scales(scales, len(scales))
        ptrs, lens, O, statuses = self._marshal(jpegs, outs, fmt)
        flags = _decode_flags(fancy, gpu_huffman, fast_idct, gpu_progressive_intervals)
        st = N.load().hipjpegDecodeBatchHost(self._h, ptrs, lens, len(jpegs), O, _FORMATS[fmt], flags, statuses)
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchHost")
        return list(statuses)

    def transfer(self, stream=None):
        st = N.load().hipjpegDecodeBatchTransfer(self._h, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchTransfer")

    def device_stage(self, stream=None, which=None):
        """which=None: all kernels; 0 idct_plane, 1 luma_color, 2 generic_color, 3 GPU entropy stage and the read-back of its
        verdicts, 4 geometry pass, 6 GPU entropy stage enqueued only.  Any other value raises HipJpegError."""
        if which is None:
            st = N.load().hipjpegDecodeBatchDevice(self._h, self._stream_ptr(stream))
        else:
            st = N.load().hipjpegDecodeBatchDeviceKernel(self._h, int(which), self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeBatchDevice")

    def stats(self):
        units = (ctypes.c_int32 * 3)()
        cb, ob = ctypes.c_uint64(), ctypes.c_uint64()
        N.load().hipjpegDecodeBatchStats(self._h, ctypes.addressof(units), ctypes.byref(cb), ctypes.byref(ob))
        gi, sl, sb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
        N.load().hipjpegDecodeBatchEntropyStats(self._h, ctypes.byref(gi), ctypes.byref(sl), ctypes.byref(sb))
        h2d, sp = ctypes.c_uint64(), ctypes.c_int32()
        N.load().hipjpegDecodeBatchTransferStats(self._h, ctypes.byref(h2d), ctypes.byref(sp))
        return dict(units=list(units), coef_bytes=cb.value, output_bytes=ob.value, gpu_entropy_images=gi.value, sync_launches=sl.value,
                    stream_bytes=sb.value, zero_copy_images=int(N.load().hipjpegDecodeBatchZeroCopyImages(self._h)), h2d_bytes=h2d.value,
                    sparse_images=sp.value, interval_images=int(N.load().hipjpegDecodeBatchIntervalImages(self._h)),
                    interval_takeovers=int(N.load().hipjpegDecodeBatchIntervalTakeovers(self._h)))

    def statuses(self, n):
        st = (ctypes.c_int * n)()
        N.load().hipjpegDecodeBatchGetStatuses(self._h, st, n)
        return list(st)


# ---------------------------------------------------------------------------------------------- encode
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                    49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_IN_FORMATS = {"rgb": N.OUTPUT_RGBI, "bgr": N.OUTPUT_BGRI, "rgb_planar": N.OUTPUT_RGB_PLANAR, "bgr_planar": N.OUTPUT_BGR_PLANAR, "gray": N.OUTPUT_Y,
               "yuv_planar": N.OUTPUT_YUV_PLANAR}


def _enc_params(subsampling, quality, input_format="rgb", restart_interval=0, optimized_huffman=False, progressive=False):
    return N.EncodeParams(int(quality), N.CSS[subsampling], _IN_FORMATS[input_format], int(restart_interval), int(bool(optimized_huffman)),
                          int(bool(progressive)))


def _encode_coefficients(entry, width, height, coefs_natural, subsampling, quality, restart_interval, optimized_huffman, progressive):
    zz = [np.ascontiguousarray(c[:, :, _ZIGZAG]) for c in coefs_natural]
    ptrs = (ctypes.c_void_p * 3)(*([z.ctypes.data for z in zz] + [None] * (3 - len(zz))))
    p = _enc_params(subsampling, quality, "rgb", restart_interval, optimized_huffman, progressive)
    cap = width * height * 3 + 65536
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_size_t()
    st = getattr(N.load(), entry)(width, height, ctypes.byref(p), ptrs, out.ctypes.data, cap, ctypes.byref(n))
    if st:
        raise N.HipJpegError(st, entry)
    return out[: n.value].tobytes()


def encode_from_coefficients_host(width, height, coefs_natural, subsampling="420", quality=90, restart_interval=0, optimized_huffman=False,
                                  progressive=False):
    """Host-only entropy coding (no GPU).  coefs_natural: per component int16 [blocks_h, blocks_w, 64] in natural order over the
    MCU-padded grid (what oracle.forward returns); converted to the zigzag layout the C-ABI takes."""
    return _encode_coefficients("hipjpegEncodeFromCoefficientsHost", width, height, coefs_natural, subsampling, quality, restart_interval,
                                optimized_huffman, progressive)


def encode_from_coefficients_gpu_algorithm_host(width, height, coefs_natural, subsampling="420", quality=90, restart_interval=0,
                                                progressive=True):
    """The GPU entropy coder's progressive algorithm run on the host with the kernels' per-block code (no GPU): the file
    encode_from_coefficients_host(..., progressive=True) writes.  Raises HipJpegError (UNSUPPORTED) for baseline output and restart
    intervals, which the GPU coder's progressive path does not take without FLAG_GPU_PROGRESSIVE_RESTART."""
    return _encode_coefficients("hipjpegEncodeFromCoefficientsGpuAlgorithmHost", width, height, coefs_natural, subsampling, quality,
                                restart_interval, False, progressive)


def encode_from_coefficients_progressive_gpu_algorithm_host(width, height, coefs_natural, subsampling="420", quality=90, restart_interval=0,
                                                            progressive=True):
    """The GPU entropy coder's progressive algorithm with restart intervals (FLAG_GPU_PROGRESSIVE_RESTART) run on the host with the
    kernels' own code (no GPU): the interval-end flush of the EOB run, the segmented scan of the bit offsets, padding, restart markers
    and the byte stuffing that spares them.  Any restart_interval: the file encode_from_coefficients_host(..., progressive=True)
    writes for it.  Raises HipJpegError (UNSUPPORTED) for baseline output."""
    return _encode_coefficients("hipjpegEncodeProgressiveGpuAlgorithmHost", width, height, coefs_natural, subsampling, quality,
                                restart_interval, False, progressive)


def encode_from_coefficients_baseline_gpu_algorithm_host(width, height, coefs_natural, subsampling="420", quality=90, restart_interval=0,
                                                         optimized_huffman=False, progressive=False):
    """The GPU entropy coder's baseline algorithm run on the host with the kernels' own code (no GPU): per-block coding, the segmented
    scan of the bit offsets, padding, restart markers and the byte stuffing that spares them.  Any restart_interval, Annex-K or
    optimized tables: the file encode_from_coefficients_host writes for the same arguments.  Raises HipJpegError (UNSUPPORTED) for
    progressive output."""
    return _encode_coefficients("hipjpegEncodeBaselineGpuAlgorithmHost", width, height, coefs_natural, subsampling, quality, restart_interval,
                                optimized_huffman, progressive)


class BatchEncoder:
    """hipjpegEncodeBatch* on one device; inputs are torch CUDA uint8 tensors ([H, W, 3] interleaved, [3, H, W] planar or [H, W] gray).
    gpu_huffman: the entropy stage's default route; gpu_restart: with gpu_huffman, the GPU coder also takes baseline images with a restart
    interval (FLAG_GPU_RESTART_INTERVALS); gpu_progressive_restart: with gpu_huffman, the GPU coder also takes progressive images with
    a restart interval (FLAG_GPU_PROGRESSIVE_RESTART)."""

    def __init__(self, device=0, num_threads=0, gpu_huffman=False, gpu_restart=False, gpu_progressive_restart=False, allocators=None):
        import torch
        self._torch = torch
        self.device = int(device)
        self.gpu_huffman = bool(gpu_huffman)
        self.gpu_restart = bool(gpu_restart)
        self.gpu_progressive_restart = bool(gpu_progressive_restart)
        self._inflight = []
        self._h = ctypes.c_void_p()
        st = N.load().hipjpegCreate(ctypes.byref(self._h), self.device, int(num_threads))
        if st:
            raise N.HipJpegError(st, "hipjpegCreate")
        self._allocators = _set_allocators(self._h, allocators)
        self._keep = None
        self._n = 0

    def close(self):
        if self._h:
            N.load().hipjpegDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream_ptr(self, stream):
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def _entropy_flags(self, gpu_huffman):
        if not gpu_huffman:
            return 0
        return (N.FLAG_GPU_HUFFMAN | (N.FLAG_GPU_RESTART_INTERVALS if self.gpu_restart else 0) |
                (N.FLAG_GPU_PROGRESSIVE_RESTART if self.gpu_progressive_restart else 0))

    def _marshal(self, images, subsampling, quality, input_format, restart_interval, optimized_huffman, progressive=False):
        n = len(images)
        I = (N.EncodeInput * n)()
        P = (N.EncodeParams * n)()
        subs = subsampling if isinstance(subsampling, (list, tuple)) else [subsampling] * n
        quals = quality if isinstance(quality, (list, tuple)) else [quality] * n
        rsts = restart_interval if isinstance(restart_interval, (list, tuple)) else [restart_interval] * n
        for i, t in enumerate(images):
            fmt = input_format
            if fmt in ("rgb", "bgr"):
                h, w = t.shape[0], t.shape[1]
                I[i].plane[0] = t.data_ptr()
                I[i].pitch[0] = t.stride(0)
            elif fmt == "gray":
                h, w = t.shape
                I[i].plane[0] = t.data_ptr()
                I[i].pitch[0] = t.stride(0)
            elif fmt == "yuv_planar":  # t = [Y, Cb, Cr], the chroma planes already in the stream's sampling
                h, w = t[0].shape
                for p in range(3):
                    I[i].plane[p] = t[p].data_ptr()
                    I[i].pitch[p] = t[p].stride(0)
            else:
                h, w = t.shape[1], t.shape[2]
                for p in range(3):
                    I[i].plane[p] = t[p].data_ptr()
                    I[i].pitch[p] = t.stride(1)
            I[i].width, I[i].height = w, h
            P[i] = _enc_params(subs[i], quals[i], fmt, rsts[i], optimized_huffman, progressive)
        self._keep = (images, I, P)
        self._n = n
        return I, P

    def device_stage(self, images, subsampling="420", quality=90, input_format="rgb", restart_interval=0, optimized_huffman=False, stream=None,
                     progressive=False):
        I, P = self._marshal(images, subsampling, quality, input_format, restart_interval, optimized_huffman, progressive)
        st_arr = (ctypes.c_int * self._n)()
        st = N.load().hipjpegEncodeBatchDevice(self._h, I, P, self._n, st_arr, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeBatchDevice")
        return list(st_arr)

    # -- pipelined: submit() queues forward kernel + entropy stage + copy of the files and returns; wait() completes the
    #    oldest submitted batch and returns (statuses, bitstreams).  At most three batches in flight.
    def submit(self, images, subsampling="420", quality=90, input_format="rgb", restart_interval=0, optimized_huffman=False, stream=None,
               gpu_huffman=None, progressive=False):
        if gpu_huffman is None:
            gpu_huffman = self.gpu_huffman
        I, P = self._marshal(images, subsampling, quality, input_format, restart_interval, optimized_huffman, progressive)
        st = N.load().hipjpegEncodeBatchSubmit(self._h, I, P, self._n, self._entropy_flags(gpu_huffman), self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeBatchSubmit")
        self._inflight.append((self._n, self._keep))

    def wait(self, fetch=True):
        n, _keep = self._inflight.pop(0)
        st_arr = (ctypes.c_int * n)()
        st = N.load().hipjpegEncodeBatchWait(self._h, st_arr, n)
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeBatchWait")
        self._n = n
        return list(st_arr), (self.bitstreams() if fetch else None)

    def relaunch(self, stream=None):
        st = N.load().hipjpegEncodeBatchRelaunch(self._h, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeBatchRelaunch")

    def host_stage(self, gpu_huffman=None):
        """Entropy stage of the prepared batch.  gpu_huffman (default: the encoder's setting): code on the GPU what it can take --
        baseline output with Annex-K or optimized tables and progressive output, without a restart interval; with the encoder's
        gpu_restart=True also baseline output with a restart interval, with gpu_progressive_restart=True also progressive output
        with one -- and the rest, or everything when False, on the host thread pool."""
        if gpu_huffman is None:
            gpu_huffman = self.gpu_huffman
        st_arr = (ctypes.c_int * self._n)()
        st = N.load().hipjpegEncodeBatchEntropy(self._h, self._entropy_flags(gpu_huffman), st_arr)
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeBatchEntropy")
        return list(st_arr)

    def bitstreams(self):
        out = []
        for i in range(self._n):
            p, n = ctypes.c_void_p(), ctypes.c_size_t()
            st = N.load().hipjpegEncodeGetBitstream(self._h, i, ctypes.byref(p), ctypes.byref(n))
            out.append(ctypes.string_at(p, n.value) if st == 0 else None)
        return out

    def coefficients(self, index):
        """Quantized coefficients of image `index`, per component int16 [real_h, real_w, 64] in NATURAL order."""
        res = []
        c = 0
        while True:
            p = ctypes.c_void_p()
            grid = (ctypes.c_int32 * 4)()
            st = N.load().hipjpegEncodeGetCoefficients(self._h, index, c, ctypes.byref(p), ctypes.addressof(grid))
            if st:
                break
            bw, bh, rw, rh = list(grid)
            a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int16)), shape=(bh, bw, 64))
            nat = np.zeros((rh, rw, 64), dtype=np.int16)
            nat[:, :, _ZIGZAG] = a[:rh, :rw, :]
            res.append(nat)
            c += 1
        return res

    def encode(self, images, subsampling="420", quality=90, input_format="rgb", restart_interval=0, optimized_huffman=False, stream=None,
               progressive=False):
        st = self.device_stage(images, subsampling, quality, input_format, restart_interval, optimized_huffman, stream, progressive)
        st = self.host_stage()
        for i, s in enumerate(st):
            if s:
                raise N.HipJpegError(s, f"image {i}")
        return self.bitstreams()

    def stats(self):
        u = ctypes.c_int32()
        pb, cb = ctypes.c_uint64(), ctypes.c_uint64()
        N.load().hipjpegEncodeBatchStats(self._h, ctypes.byref(u), ctypes.byref(pb), ctypes.byref(cb))
        return dict(units=u.value, pixel_bytes=pb.value, coef_bytes=cb.value, gpu_entropy_images=int(N.load().hipjpegEncodeBatchGpuEntropyImages(self._h)))


def _orientation_field(orientation, trim, from_exif, grayscale=False, expand=False, copy_markers=False):
    """hipjpegTranscodeParams_t::orientation"""
    flags = (N.TRANSCODE_TRIM if trim else 0) | (N.TRANSCODE_GRAYSCALE if grayscale else 0) | (N.TRANSCODE_CROP_EXPAND if expand else 0) | \
        (N.TRANSCODE_COPY_MARKERS if copy_markers else 0)
    if from_exif:
        return N.TRANSCODE_ORIENTATION_FROM_EXIF | flags
    o = int(orientation)
    if not 0 <= o <= 8:
        raise ValueError("orientation must be 1..8")
    return (0 if o == 1 else o) | flags  # the field spells the identity 0


def _region(region):
    """hipjpegTranscodeRegion_t of (x0, y0, x1, y1); None = the whole picture (all zeros)"""
    return N.TranscodeRegion(*(int(v) for v in region)) if region is not None else N.TranscodeRegion(0, 0, 0, 0)


def exif_orientation(data):
    """The EXIF orientation (1..8) of a JPEG file: tag 0x0112 of IFD0 in its first APP1/Exif segment; 1 when it is missing or out of range."""
    a = _as_u8(data)
    o = ctypes.c_int32()
    st = N.load().hipjpegGetExifOrientation(a.ctypes.data, a.size, ctypes.byref(o))
    if st:
        raise N.HipJpegError(st, "hipjpegGetExifOrientation")
    return o.value


def transcode_host(data, optimized_huffman=False, progressive=False, restart_interval=0, orientation=1, trim=False, from_exif=False, region=None,
                   grayscale=False, expand=False, copy_markers=False):
    """Lossless transcode on the host (no GPU): host entropy decoder -> host coder.  The file keeps every coefficient and the
    quantization tables of the source; APPn / COM segments are copied only with copy_markers (the EXIF orientation is reset to 1 when
    the picture is turned).  Before the turn: grayscale drops the chroma components, then region=(x0, y0, x1, y1) (stored-image
    coordinates, end exclusive) cuts the picture; its origin must lie on the iMCU grid unless expand moves it left / up onto it.  orientation 1..8: the file holds the picture brought
    upright for that EXIF value (from_exif: for the source's own tag), still without requantizing; a mirror moves whole iMCUs, so the
    mirrored axes must be multiples of the iMCU size unless trim cuts them (include/hipjpeg.h).  Raises HipJpegError: UNSUPPORTED for
    sources the coder cannot take (include/hipjpeg.h lists the rules), the decoder's statuses for damaged ones."""
    a = _as_u8(data)
    p = N.TranscodeParams(int(bool(optimized_huffman)), int(bool(progressive)), int(restart_interval),
                          _orientation_field(orientation, trim, from_exif, grayscale, expand, copy_markers))
    r = _region(region)
    n = ctypes.c_size_t()
    cap = a.size * 2 + 65536
    for _ in range(2):
        out = np.empty(cap, dtype=np.uint8)
        st = N.load().hipjpegTranscodeHostRegion(a.ctypes.data, a.size, ctypes.byref(p), ctypes.byref(r) if region is not None else None,
                                                 out.ctypes.data, cap, ctypes.byref(n))
        if st != 9:  # BUFFER_TOO_SMALL: n holds the needed size
            break
        cap = n.value
    if st:
        raise N.HipJpegError(st, "hipjpegTranscodeHostRegion")
    return out[: n.value].tobytes()


class BatchTranscoder:
    """hipjpegTranscodeBatch on one device: entropy decode, coefficient relayout kernel and entropy coder in one blocking call.
    gpu_huffman: both entropy stages on the GPU for every image each of them takes; gpu_restart: with gpu_huffman, the GPU coder also
    takes baseline output with a restart interval (FLAG_GPU_RESTART_INTERVALS); gpu_progressive_intervals: with gpu_huffman, the GPU
    decoder also takes progressive sources whose scans all have restart intervals (FLAG_GPU_PROGRESSIVE_INTERVALS);
    gpu_progressive_restart: with gpu_huffman, the GPU coder also takes progressive output with a restart interval
    (FLAG_GPU_PROGRESSIVE_RESTART).  The bytes do not depend on any of them."""

    def __init__(self, device=0, num_threads=0, gpu_huffman=True, gpu_restart=False, gpu_progressive_intervals=False,
                 gpu_progressive_restart=False, allocators=None):
        import torch
        self._torch = torch
        self.device = int(device)
        self.gpu_huffman = bool(gpu_huffman)
        self.gpu_restart = bool(gpu_restart)
        self.gpu_progressive_intervals = bool(gpu_progressive_intervals)
        self.gpu_progressive_restart = bool(gpu_progressive_restart)
        self._h = ctypes.c_void_p()
        st = N.load().hipjpegCreate(ctypes.byref(self._h), self.device, int(num_threads))
        if st:
            raise N.HipJpegError(st, "hipjpegCreate")
        self._allocators = _set_allocators(self._h, allocators)

    def close(self):
        if self._h:
            N.load().hipjpegDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_hybrid_huffman_threshold(self, pixels):
        st = N.load().hipjpegSetHybridHuffmanThreshold(self._h, int(pixels))
        if st:
            raise N.HipJpegError(st, "hipjpegSetHybridHuffmanThreshold")

    def transcode(self, jpegs, optimized_huffman=False, progressive=False, restart_interval=0, stream=None, gpu_huffman=None, orientation=1,
                  trim=False, from_exif=False, region=None, grayscale=False, expand=False, copy_markers=False):
        """Returns (statuses, files): files[i] is bytes, or None where statuses[i] != 0.  optimized_huffman / progressive /
        restart_interval / orientation / grayscale / copy_markers: one value for the batch or a list with one per image.  region: None,
        one (x0, y0, x1, y1) for every image, or a list with a tuple or None per image.  orientation, trim, from_exif, region, grayscale,
        expand, copy_markers: as transcode_host."""
        n = len(jpegs)
        if gpu_huffman is None:
            gpu_huffman = self.gpu_huffman
        flags = (N.FLAG_GPU_HUFFMAN | (N.FLAG_GPU_RESTART_INTERVALS if self.gpu_restart else 0) |
                 (N.FLAG_GPU_PROGRESSIVE_INTERVALS if self.gpu_progressive_intervals else 0) |
                 (N.FLAG_GPU_PROGRESSIVE_RESTART if self.gpu_progressive_restart else 0)) if gpu_huffman else 0
        per = [v if isinstance(v, (list, tuple)) else [v] * n for v in (optimized_huffman, progressive, restart_interval, orientation, grayscale,
                                                                         copy_markers)]
        P = (N.TranscodeParams * n)()
        for i in range(n):
            P[i] = N.TranscodeParams(int(bool(per[0][i])), int(bool(per[1][i])), int(per[2][i]),
                                     _orientation_field(per[3][i], trim, from_exif, per[4][i], expand, per[5][i]))
        if region is not None:
            regions = region if isinstance(region, list) else [region] * n
            R = (N.TranscodeRegion * max(n, 1))(*[_region(r) for r in regions])
            st = N.load().hipjpegTranscodeBatchSetRegions(self._h, R, len(regions))
            if st:
                raise N.HipJpegError(st, "hipjpegTranscodeBatchSetRegions")
        arrs = [j if (hasattr(j, "data_ptr") and hasattr(j, "numel")) else _as_u8(j) for j in jpegs]
        ptrs = (ctypes.c_void_p * n)(*[(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) for a in arrs])
        lens = (ctypes.c_size_t * n)(*[(a.numel() if hasattr(a, "numel") else a.size) for a in arrs])
        statuses = (ctypes.c_int * n)()
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device)
        st = N.load().hipjpegTranscodeBatch(self._h, ptrs, lens, n, P, flags, statuses, ctypes.c_void_p(s.cuda_stream))
        if st:
            raise N.HipJpegError(st, "hipjpegTranscodeBatch")
        files = []
        for i in range(n):
            p, ln = ctypes.c_void_p(), ctypes.c_size_t()
            ok = statuses[i] == 0 and N.load().hipjpegEncodeGetBitstream(self._h, i, ctypes.byref(p), ctypes.byref(ln)) == 0
            files.append(ctypes.string_at(p, ln.value) if ok else None)
        return list(statuses), files

    def stats(self):
        d, c, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        N.load().hipjpegTranscodeBatchStats(self._h, ctypes.byref(d), ctypes.byref(c), ctypes.byref(b))
        return dict(gpu_decoded_images=d.value, gpu_coded_images=c.value, relayout_blocks=b.value,
                    interval_takeovers=int(N.load().hipjpegDecodeBatchIntervalTakeovers(self._h)))


# ---------------------------------------------------------------- coefficient tensors
def _info_dict(ci):
    nc = ci.num_components
    d = dict(width=ci.width, height=ci.height, num_components=nc, color_model=ci.color_model)
    for k in ("h", "v", "blocks_w", "blocks_h"):
        d[k] = list(getattr(ci, k))[:nc]
    d["qtables"] = [np.array(ci.qtable[c], dtype=np.uint16) for c in range(nc)]
    return d


def _info_struct(info):
    """hipjpegCoefficientInfo_t of an info dict (coefficient_info's); h / v default to 1, the colour model to gray / YCbCr"""
    ci = N.CoefficientInfo()
    nc = int(info["num_components"])
    if not 0 <= nc <= 4:
        raise ValueError("num_components must be 1..4")
    ci.width, ci.height, ci.num_components = int(info["width"]), int(info["height"]), nc
    ci.color_model = int(info.get("color_model", 0 if nc == 1 else 1))
    for c in range(nc):
        ci.h[c] = int(info["h"][c]) if "h" in info else 1
        ci.v[c] = int(info["v"][c]) if "v" in info else 1
        ci.blocks_w[c], ci.blocks_h[c] = int(info["blocks_w"][c]), int(info["blocks_h"][c])
        q = np.asarray(info["qtables"][c]).reshape(64)
        if q.min() < 0 or q.max() > 65535:
            raise ValueError("quantizers must fit uint16")
        q = np.ascontiguousarray(q, dtype=np.uint16)
        ctypes.memmove(ci.qtable[c], q.ctypes.data, 128)
    return ci


def _coding_params(optimized_huffman, progressive, restart_interval):
    return N.TranscodeParams(int(bool(optimized_huffman)), int(bool(progressive)), int(restart_interval), 0)


def coefficient_info(data):
    """Geometry and quantization tables of a JPEG file, from its header: dict(width, height, num_components, color_model, h, v,
    blocks_w, blocks_h -- the REAL block area ceil(samp / 8) per component --, qtables: uint16[64] per component, natural order)."""
    a = _as_u8(data)
    ci = N.CoefficientInfo()
    st = N.load().hipjpegGetCoefficientInfo(a.ctypes.data, a.size, ctypes.byref(ci))
    if st:
        raise N.HipJpegError(st, "hipjpegGetCoefficientInfo")
    return _info_dict(ci)


def _css(subsampling):
    """hipjpegChromaSubsampling_t of a name or a value; a name the library does not know is HIPJPEG_CSS_UNKNOWN, which it refuses"""
    if isinstance(subsampling, str):
        return N.CSS.get(subsampling, -1)
    return int(subsampling)


def encode_coefficient_info(width, height, subsampling="420", quality=90):
    """Host only (no GPU): the dict coefficient_info returns for the file BatchEncoder writes for a width x height picture with this
    subsampling and quality -- what BatchCoefficients.from_pixels fills.  Raises HipJpegError: UNSUPPORTED for an unknown subsampling
    (a name or a hipjpegChromaSubsampling_t value), INVALID_ARGUMENT for a size outside 1..65535."""
    p = N.EncodeParams(int(quality), _css(subsampling), N.OUTPUT_RGBI, 0, 0, 0)
    ci = N.CoefficientInfo()
    st = N.load().hipjpegGetEncodeCoefficientInfo(int(width), int(height), ctypes.byref(p), ctypes.byref(ci))
    if st:
        raise N.HipJpegError(st, "hipjpegGetEncodeCoefficientInfo")
    return _info_dict(ci)


def _host_planes(coefs, what):
    """hipjpegCoefficientPlanes_t over numpy arrays [blocks_h, pitch >= blocks_w, 8, 8] (or [.., 64]) int16, C-contiguous"""
    P = N.CoefficientPlanes()
    for c, a in enumerate(coefs):
        if not isinstance(a, np.ndarray) or a.dtype != np.int16 or not a.flags["C_CONTIGUOUS"] or a.ndim not in (3, 4) or a[0, 0].size != 64:
            raise TypeError(f"{what}: component {c} must be a C-contiguous int16 array [blocks_h, pitch, 8, 8]")
        P.coef[c] = a.ctypes.data
        P.pitch_blocks[c] = a.shape[1]
    return P


def decode_coefficients_host(data, out=None):
    """Host only (no GPU): (info, coefs) with coefs[c] an int16 array [blocks_h, blocks_w, 8, 8], natural order, the quantized values as
    the stream codes them.  out: arrays to fill instead (a larger second dimension is the pitch; the padding is not written)."""
    a = _as_u8(data)
    info = coefficient_info(a)
    if out is None:
        # (numpy's allocations are 16-byte aligned for anything but tiny arrays; one block is 128 bytes)
        out = [np.zeros((bh, bw, 8, 8), dtype=np.int16) for bh, bw in zip(info["blocks_h"], info["blocks_w"])]
    if len(out) != info["num_components"] or any(o.shape[0] < bh for o, bh in zip(out, info["blocks_h"])):
        raise TypeError("decode_coefficients_host: one array of at least blocks_h rows per component")
    P = _host_planes(out, "decode_coefficients_host")
    st = N.load().hipjpegDecodeCoefficientsHost(a.ctypes.data, a.size, ctypes.byref(P))
    if st:
        raise N.HipJpegError(st, "hipjpegDecodeCoefficientsHost")
    return info, out


def encode_coefficients_host(info, coefs, optimized_huffman=False, progressive=False, restart_interval=0):
    """Host only (no GPU): the JFIF file of a picture given by `info` (coefficient_info's dict; its tables may be replaced) and its
    coefficients (as decode_coefficients_host returns them; a larger second dimension is the pitch).  Raises HipJpegError: UNSUPPORTED
    for what the writer does not write (include/hipjpeg.h lists the rules), INVALID_ARGUMENT for a description that contradicts itself."""
    ci = _info_struct(info)
    if len(coefs) < ci.num_components:
        raise TypeError("encode_coefficients_host: one array per component")
    P = _host_planes(coefs[: ci.num_components], "encode_coefficients_host")
    p = _coding_params(optimized_huffman, progressive, restart_interval)
    n = ctypes.c_size_t()
    cap = sum(int(a.nbytes) for a in coefs) * 2 + 65536
    for _ in range(2):
        out = np.empty(cap, dtype=np.uint8)
        st = N.load().hipjpegEncodeCoefficientsHost(ctypes.byref(ci), ctypes.byref(P), ctypes.byref(p), out.ctypes.data, cap, ctypes.byref(n))
        if st != 9:  # BUFFER_TOO_SMALL: n holds the needed size
            break
        cap = n.value
    if st:
        raise N.HipJpegError(st, "hipjpegEncodeCoefficientsHost")
    return out[: n.value].tobytes()


class CoefficientImage:
    """A picture as its quantized DCT coefficients on the device: info (coefficient_info's dict) and coefs, one torch CUDA int16 tensor
    [blocks_h, blocks_w, 8, 8] per component (natural order inside a block)."""

    def __init__(self, info, coefs):
        self.info = info
        self.coefs = coefs


class BatchCoefficients:
    """hipjpegDecodeCoefficientsBatch / hipjpegEncodeCoefficientsBatch on one device: JPEG files to coefficient tensors and back, the
    tensors never leaving the device.  gpu_huffman: the entropy stage on the GPU for every image it takes; gpu_restart: with gpu_huffman,
    the GPU coder also takes baseline output with a restart interval; gpu_progressive_intervals: with gpu_huffman, the GPU decoder also
    takes progressive files whose scans all have restart intervals; gpu_progressive_restart: with gpu_huffman, the GPU coder also takes
    progressive output with a restart interval.  Neither the tensors nor the bytes depend on any of them."""

    def __init__(self, device=0, num_threads=0, gpu_huffman=True, gpu_restart=False, gpu_progressive_intervals=False,
                 gpu_progressive_restart=False, allocators=None):
        import torch
        self._torch = torch
        self.device = int(device)
        self.gpu_huffman = bool(gpu_huffman)
        self.gpu_restart = bool(gpu_restart)
        self.gpu_progressive_intervals = bool(gpu_progressive_intervals)
        self.gpu_progressive_restart = bool(gpu_progressive_restart)
        self._h = ctypes.c_void_p()
        st = N.load().hipjpegCreate(ctypes.byref(self._h), self.device, int(num_threads))
        if st:
            raise N.HipJpegError(st, "hipjpegCreate")
        self._allocators = _set_allocators(self._h, allocators)

    def close(self):
        if self._h:
            N.load().hipjpegDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_hybrid_huffman_threshold(self, pixels):
        st = N.load().hipjpegSetHybridHuffmanThreshold(self._h, int(pixels))
        if st:
            raise N.HipJpegError(st, "hipjpegSetHybridHuffmanThreshold")

    def _flags(self):
        return (N.FLAG_GPU_HUFFMAN | (N.FLAG_GPU_RESTART_INTERVALS if self.gpu_restart else 0) |
                (N.FLAG_GPU_PROGRESSIVE_INTERVALS if self.gpu_progressive_intervals else 0) |
                (N.FLAG_GPU_PROGRESSIVE_RESTART if self.gpu_progressive_restart else 0)) if self.gpu_huffman else 0

    def _stream_ptr(self, stream):
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def _planes(self, coefs, blocks_h, blocks_w, what):
        """hipjpegCoefficientPlanes_t over torch tensors [>= blocks_h, pitch >= blocks_w, 8, 8]: on this device, int16, the last three
        dimensions contiguous (the first may have any stride that is a whole number of rows)"""
        torch = self._torch
        P = N.CoefficientPlanes()
        if len(coefs) != len(blocks_h):
            raise TypeError(f"{what}: one tensor per component")
        for c, t in enumerate(coefs):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device.index != self.device:
                raise TypeError(f"{what}: component {c} must be a tensor on cuda:{self.device}")
            if t.dtype != torch.int16 or t.dim() != 4 or tuple(t.shape[2:]) != (8, 8):
                raise TypeError(f"{what}: component {c} must be int16 [blocks_h, blocks_w, 8, 8]")
            if t.stride(3) != 1 or t.stride(2) != 8 or t.stride(1) != 64 or t.stride(0) % 64 != 0 or t.stride(0) < 64 * blocks_w[c]:
                raise TypeError(f"{what}: component {c}: the last three dimensions must be contiguous and a row must hold blocks_w blocks")
            if t.shape[0] < blocks_h[c] or t.shape[1] < blocks_w[c]:
                raise TypeError(f"{what}: component {c} is smaller than the picture's {blocks_h[c]} x {blocks_w[c]} blocks")
            P.coef[c] = t.data_ptr()
            P.pitch_blocks[c] = t.stride(0) // 64
        return P

    def allocate(self, info):
        dev = self._torch.device("cuda", self.device)
        return [self._torch.empty((bh, bw, 8, 8), dtype=self._torch.int16, device=dev) for bh, bw in zip(info["blocks_h"], info["blocks_w"])]

    def decode(self, jpegs, stream=None, outs=None):
        """Returns (statuses, images): images[i] is a CoefficientImage, or None where statuses[i] != 0.  The export kernel is queued on
        `stream` (default: the current one); work queued on that stream afterwards sees the tensors.  outs: per image None or a list of
        caller tensors to fill (a larger second dimension, or a larger row stride, is the pitch; the padding is not written)."""
        n = len(jpegs)
        arrs = [j if (hasattr(j, "data_ptr") and hasattr(j, "numel")) else _as_u8(j) for j in jpegs]
        ptrs = (ctypes.c_void_p * n)(*[(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) for a in arrs])
        lens = (ctypes.c_size_t * n)(*[(a.numel() if hasattr(a, "numel") else a.size) for a in arrs])
        P = (N.CoefficientPlanes * max(n, 1))()
        infos, tensors = [], []
        for i, a in enumerate(arrs):
            try:
                info = coefficient_info(a)
            except N.HipJpegError:
                infos.append(None)  # the batch call reports why; its planes stay null and are never looked at
                tensors.append(None)
                continue
            t = outs[i] if outs is not None and outs[i] is not None else self.allocate(info)
            P[i] = self._planes(t, info["blocks_h"], info["blocks_w"], f"decode: image {i}")
            infos.append(info)
            tensors.append(t)
        statuses = (ctypes.c_int * n)()
        st = N.load().hipjpegDecodeCoefficientsBatch(self._h, ptrs, lens, n, P, self._flags(), statuses, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeCoefficientsBatch")
        images = [CoefficientImage(infos[i], tensors[i]) if statuses[i] == 0 else None for i in range(n)]
        return list(statuses), images

    def encode(self, images, optimized_huffman=False, progressive=False, restart_interval=0, stream=None):
        """images: CoefficientImage (or (info, coefs)) per picture.  Returns (statuses, files): files[i] is bytes, or None where
        statuses[i] != 0.  optimized_huffman / progressive / restart_interval: one value for the batch or a list with one per image.  The
        import kernel is queued on `stream` (default: the current one), behind whatever produced the tensors there."""
        n = len(images)
        per = [v if isinstance(v, (list, tuple)) else [v] * n for v in (optimized_huffman, progressive, restart_interval)]
        I = (N.CoefficientInfo * max(n, 1))()
        P = (N.CoefficientPlanes * max(n, 1))()
        T = (N.TranscodeParams * max(n, 1))()
        for i, im in enumerate(images):
            info, coefs = (im.info, im.coefs) if isinstance(im, CoefficientImage) else im
            I[i] = _info_struct(info)
            nc = I[i].num_components
            P[i] = self._planes(list(coefs)[:nc], list(I[i].blocks_h)[:nc], list(I[i].blocks_w)[:nc], f"encode: image {i}")
            T[i] = _coding_params(per[0][i], per[1][i], per[2][i])
        statuses = (ctypes.c_int * n)()
        st = N.load().hipjpegEncodeCoefficientsBatch(self._h, I, P, T, n, self._flags(), statuses, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeCoefficientsBatch")
        files = []
        for i in range(n):
            p, ln = ctypes.c_void_p(), ctypes.c_size_t()
            ok = statuses[i] == 0 and N.load().hipjpegEncodeGetBitstream(self._h, i, ctypes.byref(p), ctypes.byref(ln)) == 0
            files.append(ctypes.string_at(p, ln.value) if ok else None)
        return list(statuses), files

    def _pixel_outputs(self, info, fmt, transform):
        """what BatchDecoder.allocate_outputs allocates for a file of this geometry"""
        torch = self._torch
        dev = torch.device("cuda", self.device)
        h, w = info["height"], info["width"]
        if transform is not None:
            roi, orientation = transform
            if roi is not None:
                w, h = roi[2] - roi[0], roi[3] - roi[1]
            if orientation >= 5:
                w, h = h, w
        if fmt in ("rgb", "bgr"):
            return torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        if fmt in ("rgb_planar", "bgr_planar"):
            return torch.empty((3, h, w), dtype=torch.uint8, device=dev)
        if fmt == "y":
            return torch.empty((h, w), dtype=torch.uint8, device=dev)
        nc = min(info["num_components"], 3)
        hs, vs = info.get("h", [1] * nc), info.get("v", [1] * nc)
        hmax, vmax = max(hs[:nc]), max(vs[:nc])
        return [torch.empty(((info["height"] * vs[c] + vmax - 1) // vmax, (info["width"] * hs[c] + hmax - 1) // hmax), dtype=torch.uint8, device=dev)
                for c in range(nc)]

    def to_pixels(self, images, fmt="rgb", fancy=True, fast_idct=False, outs=None, transforms=None, stream=None):
        """images: CoefficientImage (or (info, coefs)) per picture.  Returns (statuses, outs): the pixels BatchDecoder.decode gives for
        a file with these coefficients and tables, with no entropy stage and no file in between.  outs: the caller's outputs, or None to
        have them allocated as BatchDecoder.allocate_outputs does for such a file (format, transforms).  transforms: per image None or
        (roi, orientation).  Everything is queued on `stream` (default: the current one), behind whatever produced the tensors there;
        nothing blocks, and the statuses are final."""
        n = len(images)
        I = (N.CoefficientInfo * max(n, 1))()
        P = (N.CoefficientPlanes * max(n, 1))()
        O = (N.Output * max(n, 1))()
        infos = []
        for i, im in enumerate(images):
            info, coefs = (im.info, im.coefs) if isinstance(im, CoefficientImage) else im
            I[i] = _info_struct(info)
            nc = I[i].num_components
            P[i] = self._planes(list(coefs)[:nc], list(I[i].blocks_h)[:nc], list(I[i].blocks_w)[:nc], f"to_pixels: image {i}")
            infos.append(info)
        if outs is None:
            outs = [self._pixel_outputs(info, fmt, transforms[i] if transforms is not None else None) for i, info in enumerate(infos)]
        for i, o in enumerate(outs):
            if o is None:
                continue
            if fmt in ("rgb", "bgr", "y"):
                O[i].plane[0], O[i].pitch[0] = o.data_ptr(), o.stride(0)
            elif fmt in ("rgb_planar", "bgr_planar"):
                for p in range(3):
                    O[i].plane[p], O[i].pitch[p] = o[p].data_ptr(), o.stride(1)
            else:
                for p, t in enumerate(o):
                    O[i].plane[p], O[i].pitch[p] = t.data_ptr(), t.stride(0)
        if transforms is not None:
            T = (N.Transform * max(n, 1))()
            for i, t in enumerate(transforms):
                T[i].orientation = 1
                if t is not None:
                    roi, orientation = t
                    if roi is not None:
                        T[i].x0, T[i].y0, T[i].x1, T[i].y1 = [int(v) for v in roi]
                    T[i].orientation = int(orientation)
            st = N.load().hipjpegDecodeBatchSetTransforms(self._h, T, n)
            if st:
                raise N.HipJpegError(st, "hipjpegDecodeBatchSetTransforms")
        statuses = (ctypes.c_int * n)()
        st = N.load().hipjpegCoefficientsToPixelsBatch(self._h, I, P, n, O, _FORMATS[fmt], _decode_flags(fancy, False, fast_idct), statuses,
                                                       self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegCoefficientsToPixelsBatch")
        return list(statuses), outs

    def from_pixels(self, images, subsampling="420", quality=90, input_format="rgb", outs=None, stream=None):
        """images: torch CUDA uint8 tensors as BatchEncoder takes them ([H, W, 3] interleaved, [3, H, W] planar, [H, W] gray, or
        [Y, Cb, Cr] for "yuv_planar").  subsampling / quality: one value for the batch or a list with one per image.  Returns (statuses,
        images): images[i] is a CoefficientImage holding what BatchCoefficients.decode reads from the file BatchEncoder writes for the
        same pixels and parameters, or None where statuses[i] != 0.  outs: per image None or a list of caller tensors to fill (as in
        decode).  Everything is queued on `stream` (default: the current one); nothing blocks."""
        n = len(images)
        subs = subsampling if isinstance(subsampling, (list, tuple)) else [subsampling] * n
        quals = quality if isinstance(quality, (list, tuple)) else [quality] * n
        I = (N.EncodeInput * max(n, 1))()
        E = (N.EncodeParams * max(n, 1))()
        P = (N.CoefficientPlanes * max(n, 1))()
        infos, tensors = [], []
        for i, t in enumerate(images):
            if input_format in ("rgb", "bgr"):
                h, w = t.shape[0], t.shape[1]
                I[i].plane[0], I[i].pitch[0] = t.data_ptr(), t.stride(0)
            elif input_format == "gray":
                h, w = t.shape
                I[i].plane[0], I[i].pitch[0] = t.data_ptr(), t.stride(0)
            elif input_format == "yuv_planar":
                h, w = t[0].shape
                for p in range(3):
                    I[i].plane[p], I[i].pitch[p] = t[p].data_ptr(), t[p].stride(0)
            else:
                h, w = t.shape[1], t.shape[2]
                for p in range(3):
                    I[i].plane[p], I[i].pitch[p] = t[p].data_ptr(), t.stride(1)
            I[i].width, I[i].height = w, h
            E[i] = N.EncodeParams(int(quals[i]), _css(subs[i]), _IN_FORMATS[input_format], 0, 0, 0)
            try:
                info = encode_coefficient_info(w, h, subs[i], quals[i])
            except N.HipJpegError:
                infos.append(None)  # the batch call reports why; its planes stay null and are never looked at
                tensors.append(None)
                continue
            o = outs[i] if outs is not None and outs[i] is not None else self.allocate(info)
            if any(x is None for x in o):  # (a caller's list with a hole: the library refuses the image)
                for c, x in enumerate(o):
                    if x is not None:
                        P[i].coef[c], P[i].pitch_blocks[c] = x.data_ptr(), x.stride(0) // 64
            else:
                P[i] = self._planes(o, info["blocks_h"], info["blocks_w"], f"from_pixels: image {i}")
            infos.append(info)
            tensors.append(o)
        statuses = (ctypes.c_int * n)()
        st = N.load().hipjpegPixelsToCoefficientsBatch(self._h, I, E, n, P, statuses, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegPixelsToCoefficientsBatch")
        return list(statuses), [CoefficientImage(infos[i], tensors[i]) if statuses[i] == 0 else None for i in range(n)]

    def stats(self):
        d, c, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        N.load().hipjpegCoefficientsBatchStats(self._h, ctypes.byref(d), ctypes.byref(c), ctypes.byref(b))
        return dict(gpu_decoded_images=d.value, gpu_coded_images=c.value, moved_blocks=b.value,
                    interval_takeovers=int(N.load().hipjpegDecodeBatchIntervalTakeovers(self._h)))


# ---------------------------------------------------------------------------------------------- lossless JPEG (SOF3)
def lossless_kernel_shape():
    """hipjpegLosslessKernelShape: the seams of the two reconstruction kernels, as a dict"""
    k = N.LosslessKernelShape()
    st = N.load().hipjpegLosslessKernelShape(ctypes.byref(k))
    if st:
        raise N.HipJpegError(st, "hipjpegLosslessKernelShape")
    return {n: getattr(k, n) for n, _ in N.LosslessKernelShape._fields_}


def lossless_info(data):
    """hipjpegGetLosslessInfo as a dict: width, height, num_components, precision, predictor, point_transform, restart_rows,
    component_id.  Raises HipJpegError (UNSUPPORTED: not a lossless frame, or one outside the rules; BAD_JPEG; TRUNCATED)."""
    arr = _as_u8(data)
    li = N.LosslessInfo()
    st = N.load().hipjpegGetLosslessInfo(arr.ctypes.data, arr.size, ctypes.byref(li))
    if st:
        raise N.HipJpegError(st, "hipjpegGetLosslessInfo")
    d = {n: getattr(li, n) for n in ("width", "height", "num_components", "precision", "predictor", "point_transform", "restart_rows")}
    d["component_id"] = list(li.component_id)[:li.num_components]
    return d


def _lossless_host_output(info, dtype, planar):
    h, w, n = info["height"], info["width"], info["num_components"]
    out = np.zeros((n, h, w) if planar else (h, w, n), dtype=dtype)
    o = N.LosslessOutput()
    o.sample_bytes = out.itemsize
    o.planar = 1 if planar else 0
    for c in range(n if planar else 1):
        o.plane[c] = out.ctypes.data + (c * h * w * out.itemsize if planar else 0)
        o.pitch[c] = w * out.itemsize * (1 if planar else n)
    return out, o


def decode_lossless_host(data, dtype=np.uint16, planar=False, algorithm=None):
    """hipjpegDecodeLosslessHost (algorithm=None) or hipjpegLosslessReconstructAlgorithmHost (algorithm = 0: the planner's kernel,
    1: the rows kernel's schedule, 2: the wavefront kernel's): an H x W x N array (N x H x W when planar) of uint16, or of uint8 for
    files of precision <= 8."""
    arr = _as_u8(data)
    info = lossless_info(arr)
    out, o = _lossless_host_output(info, np.dtype(dtype), planar)
    L = N.load()
    if algorithm is None:
        st, what = L.hipjpegDecodeLosslessHost(arr.ctypes.data, arr.size, ctypes.byref(o)), "hipjpegDecodeLosslessHost"
    else:
        st, what = (L.hipjpegLosslessReconstructAlgorithmHost(arr.ctypes.data, arr.size, ctypes.byref(o), int(algorithm)),
                    "hipjpegLosslessReconstructAlgorithmHost")
    if st:
        raise N.HipJpegError(st, what)
    return out


def lossless_entropy_shape():
    """hipjpegLosslessEntropyShape: the seams of the GPU entropy stage of the lossless decoder, as a dict"""
    k = N.LosslessEntropyShape()
    st = N.load().hipjpegLosslessEntropyShape(ctypes.byref(k))
    if st:
        raise N.HipJpegError(st, "hipjpegLosslessEntropyShape")
    return {n: getattr(k, n) for n, _ in N.LosslessEntropyShape._fields_}


def _lossless_difference_planes(data):
    arr = _as_u8(data)
    info = lossless_info(arr)
    planes = np.zeros((info["num_components"], info["height"], info["width"]), dtype=np.uint16)
    ptrs = (ctypes.c_void_p * 4)(*[planes[c].ctypes.data for c in range(info["num_components"])])
    return arr, planes, ptrs, info["width"]


def lossless_entropy_algorithm_host(data):
    """hipjpegLosslessEntropyAlgorithmHost: the GPU entropy stage's schedule run on the CPU.  -> (status, N x H x W uint16 differences,
    converged); the status and, where the walk did not vouch for the image, the differences are the host stage's, as in the batch call.
    Raises HipJpegError where the file is no lossless frame the decoder takes."""
    arr, planes, ptrs, pitch = _lossless_difference_planes(data)
    converged = ctypes.c_int32(-1)
    st = N.load().hipjpegLosslessEntropyAlgorithmHost(arr.ctypes.data, arr.size, ptrs, pitch, ctypes.byref(converged))
    return st, planes, bool(converged.value)


def lossless_entropy_host(data):
    """hipjpegLosslessEntropyHost: the host entropy stage alone.  -> (status, N x H x W uint16 differences)"""
    arr, planes, ptrs, pitch = _lossless_difference_planes(data)
    st = N.load().hipjpegLosslessEntropyHost(arr.ctypes.data, arr.size, ptrs, pitch)
    return st, planes


def plugin_lossless_entropy_stats():
    """hipjpegPluginLosslessEntropyStats: what the plugin decoders of this process sent through the GPU entropy stage so far"""
    g, f = ctypes.c_int64(), ctypes.c_int64()
    st = N.load().hipjpegPluginLosslessEntropyStats(ctypes.byref(g), ctypes.byref(f))
    if st:
        raise N.HipJpegError(st, "hipjpegPluginLosslessEntropyStats")
    return {"gpu_images": g.value, "host_fallback_images": f.value}


class BatchLosslessDecoder:
    """hipjpegDecodeLosslessBatch on one device: lossless JPEG files (SOF3, 2..16 bit, predictors 1..7) to torch tensors of the stored
    samples, uint16 (or uint8 for files of precision <= 8), H x W x N or N x H x W.  The entropy stage runs on host threads; prediction
    runs on the GPU.  gpu_entropy=True: hipjpegDecodeLosslessBatchFlags with HIPJPEG_FLAG_GPU_HUFFMAN, the entropy stage on the GPU too."""

    def __init__(self, device=0, num_threads=0, gpu_entropy=False, allocators=None):
        import torch
        self._torch = torch
        self.device = int(device)
        self.gpu_entropy = bool(gpu_entropy)
        self._h = ctypes.c_void_p()
        st = N.load().hipjpegCreate(ctypes.byref(self._h), self.device, int(num_threads))
        if st:
            raise N.HipJpegError(st, "hipjpegCreate")
        self._allocators = _set_allocators(self._h, allocators)

    def close(self):
        if self._h:
            N.load().hipjpegDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream_ptr(self, stream):
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def allocate(self, info, dtype=None, planar=False):
        torch = self._torch
        dtype = dtype or torch.uint16
        h, w, n = info["height"], info["width"], info["num_components"]
        return torch.empty((n, h, w) if planar else (h, w, n), dtype=dtype, device=torch.device("cuda", self.device))

    def output(self, tensor, info, planar=False):
        """hipjpegLosslessOutput_t over a tensor on this device: uint16 or uint8, [H, W, N] (or [N, H, W] when planar) with the last
        dimension(s) of a row contiguous; the row stride is the pitch, and the tensor may start at any byte."""
        torch = self._torch
        if not isinstance(tensor, torch.Tensor) or tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise TypeError(f"lossless output must be a tensor on cuda:{self.device}")
        if tensor.dtype not in (torch.uint16, torch.uint8) or tensor.dim() != 3:
            raise TypeError("lossless output must be a uint16 or uint8 tensor of three dimensions")
        h, w, n = info["height"], info["width"], info["num_components"]
        size = tensor.element_size()
        o = N.LosslessOutput()
        o.sample_bytes = size
        o.planar = 1 if planar else 0
        if planar:
            if tuple(tensor.shape) != (n, h, w) or tensor.stride(2) != 1 or tensor.stride(1) < w:
                raise TypeError(f"planar lossless output must be [{n}, {h}, {w}] with contiguous rows")
            for c in range(n):
                o.plane[c] = tensor.data_ptr() + c * tensor.stride(0) * size
                o.pitch[c] = tensor.stride(1) * size
        else:
            if tuple(tensor.shape) != (h, w, n) or tensor.stride(2) != 1 or tensor.stride(1) != n or tensor.stride(0) < w * n:
                raise TypeError(f"interleaved lossless output must be [{h}, {w}, {n}] with contiguous rows")
            o.plane[0] = tensor.data_ptr()
            o.pitch[0] = tensor.stride(0) * size
        return o

    def decode(self, jpegs, dtype=None, planar=False, outs=None, raw_outputs=None, stream=None):
        """Returns (statuses, tensors): tensors[i] is None where statuses[i] != 0 and no tensor was given.  Queued on `stream` (default:
        the current one).  outs: per image None or a tensor to fill (see output()); raw_outputs: per image None or a ready
        N.LosslessOutput (any pitch, any byte offset) that takes the place of a tensor."""
        n = len(jpegs)
        arrs = [_as_u8(j) for j in jpegs]
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
        O = (N.LosslessOutput * max(n, 1))()
        tensors = []
        for i, a in enumerate(arrs):
            if raw_outputs is not None and raw_outputs[i] is not None:
                O[i] = raw_outputs[i]
                tensors.append(None)
                continue
            try:
                info = lossless_info(a)
            except N.HipJpegError:
                tensors.append(None)  # the batch call reports why; the output stays null and is never looked at
                continue
            t = outs[i] if outs is not None and outs[i] is not None else self.allocate(info, dtype, planar)
            O[i] = self.output(t, info, planar)
            tensors.append(t)
        statuses = (ctypes.c_int * n)()
        if self.gpu_entropy:
            st, what = (N.load().hipjpegDecodeLosslessBatchFlags(self._h, ptrs, lens, n, O, statuses, N.FLAG_GPU_HUFFMAN, self._stream_ptr(stream)),
                        "hipjpegDecodeLosslessBatchFlags")
        else:
            st, what = N.load().hipjpegDecodeLosslessBatch(self._h, ptrs, lens, n, O, statuses, self._stream_ptr(stream)), "hipjpegDecodeLosslessBatch"
        if st:
            raise N.HipJpegError(st, what)
        given = outs if outs is not None else [None] * n
        return list(statuses), [tensors[i] if statuses[i] == 0 or given[i] is not None else None for i in range(n)]

    def device_stage(self, which, stream=None):
        """hipjpegDecodeLosslessBatchDeviceKernel: one part of the last decode() again (0 upload, 1 rows kernels, 2 wavefront kernel; behind a
        decode() with gpu_entropy in which no image went to the host stage also 3 destuffing and synchronisation, 4 the write pass)"""
        st = N.load().hipjpegDecodeLosslessBatchDeviceKernel(self._h, int(which), self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeLosslessBatchDeviceKernel")

    def stats(self):
        k = (ctypes.c_int32 * 2)()
        b = ctypes.c_uint64()
        st = N.load().hipjpegDecodeLosslessBatchStats(self._h, k, ctypes.byref(b))
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeLosslessBatchStats")
        e = [ctypes.c_int32() for _ in range(3)]
        st = N.load().hipjpegDecodeLosslessBatchEntropyStats(self._h, *[ctypes.byref(x) for x in e])
        if st:
            raise N.HipJpegError(st, "hipjpegDecodeLosslessBatchEntropyStats")
        return {"rows_images": k[0], "wavefront_images": k[1], "h2d_bytes": b.value, "gpu_images": e[0].value,
                "host_fallback_images": e[1].value, "ripple_launches": e[2].value}


# ------------------------------------------------------------------------------------------------------------- lossless encoding
def lossless_encode_shape():
    """hipjpegLosslessEncodeShape: the seams of the lossless coder's kernels, as a dict"""
    k = N.LosslessEncodeShape()
    st = N.load().hipjpegLosslessEncodeShape(ctypes.byref(k))
    if st:
        raise N.HipJpegError(st, "hipjpegLosslessEncodeShape")
    return {n: getattr(k, n) for n, _ in N.LosslessEncodeShape._fields_}


def lossless_encode_fits_gpu(samples, intervals):
    """hipjpegLosslessEncodeFitsGpu: whether the kernels' uint32 bit offsets hold a scan of that many samples and restart intervals"""
    return bool(N.load().hipjpegLosslessEncodeFitsGpu(int(samples), int(intervals)))


def _lossless_encode_params(precision, predictor, point_transform, restart_rows, num_components):
    return N.LosslessEncodeParams(int(precision), int(predictor), int(point_transform), int(restart_rows), int(num_components))


def lossless_encode_input(base, shape, strides, itemsize, planar):
    """hipjpegLosslessEncodeInput_t over samples at address `base`: shape / strides (in bytes) of an H x W x N picture, or N x H x W when
    planar (H x W: one component).  The samples of a row must be contiguous; the row stride is the pitch.  -> (structure, N)"""
    shape, strides = tuple(shape), tuple(strides)
    if len(shape) == 2:
        shape, strides = (shape + (1,), strides + (itemsize,)) if not planar else ((1,) + shape, (0,) + strides)
    if len(shape) != 3:
        raise TypeError("a lossless picture has two or three dimensions")
    x = N.LosslessEncodeInput()
    x.sample_bytes = itemsize
    x.planar = 1 if planar else 0
    if planar:
        n, h, w = shape
        if w > 1 and strides[2] != itemsize:
            raise TypeError("the samples of a row must be contiguous")
        for c in range(min(n, 4)):
            x.plane[c] = base + c * strides[0]
            x.pitch[c] = strides[1] if h > 1 else w * itemsize
    else:
        h, w, n = shape
        if (n > 1 and strides[2] != itemsize) or (w > 1 and strides[1] != n * itemsize):
            raise TypeError("the samples of a row must be contiguous")
        x.plane[0] = base
        x.pitch[0] = strides[0] if h > 1 else w * n * itemsize
    x.width, x.height = w, h
    return x, n


def _encode_lossless_host(entry, samples, precision, predictor, point_transform, restart_rows, planar):
    a = np.asarray(samples)
    if a.dtype not in (np.uint8, np.uint16):
        raise TypeError("lossless samples are uint8 or uint16")
    x, n = lossless_encode_input(a.ctypes.data, a.shape, a.strides, a.itemsize, planar)
    p = _lossless_encode_params(precision, predictor, point_transform, restart_rows, n)
    fn = getattr(N.load(), entry)
    need = ctypes.c_size_t(0)
    st = fn(ctypes.byref(x), ctypes.byref(p), None, 0, ctypes.byref(need))
    if st != 9:  # BUFFER_TOO_SMALL names the length
        raise N.HipJpegError(st, entry)
    out = np.empty(need.value, dtype=np.uint8)
    st = fn(ctypes.byref(x), ctypes.byref(p), out.ctypes.data, out.size, ctypes.byref(need))
    if st:
        raise N.HipJpegError(st, entry)
    return out[:need.value].tobytes()


def encode_lossless_host(samples, precision, predictor=1, point_transform=0, restart_rows=0, planar=False):
    """hipjpegEncodeLosslessHost: uint8 / uint16 samples H x W x N (N x H x W when planar, H x W for one component; the row stride is the
    pitch) to the bytes of the lossless JPEG file libjpeg-turbo writes from them."""
    return _encode_lossless_host("hipjpegEncodeLosslessHost", samples, precision, predictor, point_transform, restart_rows, planar)


def encode_lossless_gpu_algorithm_host(samples, precision, predictor=1, point_transform=0, restart_rows=0, planar=False):
    """hipjpegEncodeLosslessGpuAlgorithmHost: the same file by the kernels' schedule run on the CPU"""
    return _encode_lossless_host("hipjpegEncodeLosslessGpuAlgorithmHost", samples, precision, predictor, point_transform, restart_rows, planar)


class BatchLosslessEncoder:
    """hipjpegEncodeLosslessBatch on one device: torch tensors of stored samples (uint8 / uint16, H x W x N, or N x H x W when planar; any
    row stride) to lossless JPEG files, byte for byte libjpeg-turbo's.  Everything runs in kernels; the files land in pinned host memory."""

    def __init__(self, device=0, num_threads=0, allocators=None):
        import torch
        self._torch = torch
        self.device = int(device)
        self._h = ctypes.c_void_p()
        st = N.load().hipjpegCreate(ctypes.byref(self._h), self.device, int(num_threads))
        if st:
            raise N.HipJpegError(st, "hipjpegCreate")
        self._allocators = _set_allocators(self._h, allocators)

    def close(self):
        if self._h:
            N.load().hipjpegDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream_ptr(self, stream):
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def _per_image(self, value, n):
        return list(value) if isinstance(value, (list, tuple)) else [value] * n

    def encode(self, images, precision, predictor=1, point_transform=0, restart_rows=0, planar=False, stream=None):
        """-> (statuses, files): files[i] is the bytes of image i's file, None where statuses[i] != 0.  precision, predictor,
        point_transform, restart_rows and planar may each be one value or a list with one per image."""
        torch = self._torch
        n = len(images)
        per = [self._per_image(v, n) for v in (precision, predictor, point_transform, restart_rows, planar)]
        X = (N.LosslessEncodeInput * max(n, 1))()
        P = (N.LosslessEncodeParams * max(n, 1))()
        for i, t in enumerate(images):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device.index != self.device:
                raise TypeError(f"lossless input must be a tensor on cuda:{self.device}")
            if t.dtype not in (torch.uint16, torch.uint8):
                raise TypeError("lossless input must be a uint16 or uint8 tensor")
            size = t.element_size()
            X[i], comps = lossless_encode_input(t.data_ptr(), t.shape, [s * size for s in t.stride()], size, per[4][i])
            P[i] = _lossless_encode_params(per[0][i], per[1][i], per[2][i], per[3][i], comps)
        return self._encode(X, P, n, stream)

    def _encode(self, X, P, n, stream=None):
        """hipjpegEncodeLosslessBatch over n ready descriptors, then every file"""
        statuses = (ctypes.c_int * max(n, 1))()
        st = N.load().hipjpegEncodeLosslessBatch(self._h, X, P, n, statuses, self._stream_ptr(stream))
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeLosslessBatch")
        files = []
        for i in range(n):
            if statuses[i]:
                files.append(None)
                continue
            ptr, length = ctypes.c_void_p(), ctypes.c_size_t()
            st = N.load().hipjpegEncodeLosslessGetBitstream(self._h, i, ctypes.byref(ptr), ctypes.byref(length))
            if st:
                raise N.HipJpegError(st, "hipjpegEncodeLosslessGetBitstream")
            files.append(ctypes.string_at(ptr.value, length.value))
        return list(statuses)[:n], files

    def stats(self):
        g, w, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
        st = N.load().hipjpegEncodeLosslessBatchStats(self._h, ctypes.byref(g), ctypes.byref(w), ctypes.byref(b))
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeLosslessBatchStats")
        return {"gpu_images": g.value, "waits": w.value, "bit_buffer_bytes": b.value}

    STAGES = ("upload_stats", "counts_wait_tables", "codes_length", "scan", "totals_wait_layout", "upload_zero", "write", "count_layout", "expand",
              "copies")

    def stage_times(self):
        """hipjpegEncodeLosslessBatchStageTimes: the stages of the last encode() in milliseconds, by HIP events, as a dict"""
        ms = (ctypes.c_float * 10)()
        st = N.load().hipjpegEncodeLosslessBatchStageTimes(self._h, ms)
        if st:
            raise N.HipJpegError(st, "hipjpegEncodeLosslessBatchStageTimes")
        return dict(zip(self.STAGES, list(ms)))
