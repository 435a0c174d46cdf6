"""Allocators that hand the library memory which is NOT zero (tests/test_gpu_poisoned_arenas.py).

Every handle stages its batches in grow-only arenas (csrc/staging.h) that are never cleared as a whole; docs/arena_regions.md lists, region
by region, who writes what before whom.  A fresh hipMalloc commonly returns cleared memory, so a kernel that reads a byte its batch did
not write would go unnoticed on a fresh handle -- and would see the previous batch's tables on a used one.  PoisonAllocators fills every
allocation with one byte before the library sees it, and can fill every live device allocation again between two batches (refill()).

    fill 0x00   the control: what fresh memory usually holds; proves that the harness itself changes nothing
    fill 0x5A   the project's poison byte (gpu_huffman_host.cpp)
    fill 0xFF   all ones: kRecInvalid as a record mark, kLlInvalidPacked as a lossless state, -1 as an index or a count

No further byte: the regions that hold marks, indices or positions (the audit's rows for records, first_block, walkers, block_pos,
tail counts, unit_out) are 16-, 32- or 64-bit words.  A uniform byte b gives the words b * 0x0101..01: as a 16-bit record mark only b = 0
is below kRecOverflow (a record that reads as usable, naming no block -- the control is the plausible value there); as an index or a bit
position both 0x5A5A5A5A and 0xFFFFFFFF lie far outside every arena and every stream of the small test pictures, one in the positive
and one in the negative range of a signed reader.  Another byte would be a third value of the second kind.

Two configurations (hipjpegSetAllocators / the plugin's execution parameters):
    pinned=False   device allocator only: the library keeps its own pinned memory, into which kernels store verdicts and coded files
                   directly;
    pinned=True    device and pinned allocator: the library does not know the device mapping of the caller's pinned memory and takes
                   its "assemble in HBM, copy down" routes.
"""
import ctypes as C


def _hip():
    lib = C.CDLL("libamdhip64.so")  # (the runtime the process already holds: torch's, loaded before the library)
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    lib.hipHostFree.argtypes = [C.c_void_p]
    return lib


class PoisonAllocators:
    """calls: allocations made (device + pinned); live / live_pinned: {pointer: size} of what has not been handed back."""

    def __init__(self, byte, pinned=False):
        from nvimagecodec_amd import _native as N
        assert 0 <= byte <= 255
        self.byte, self.pinned = int(byte), bool(pinned)
        self.calls = self.device_calls = self.pinned_calls = 0
        self.live, self.live_pinned = {}, {}
        self.errors = []
        self._hip = _hip()
        # ctypes callbacks must outlive every handle that holds them: they are members
        self._cb = (N.AllocatorMalloc(self._device_malloc), N.AllocatorFree(self._device_free),
                    N.AllocatorMalloc(self._pinned_malloc), N.AllocatorFree(self._pinned_free))
        self._N = N

    # ---- the four functions (ctx, ptr, size, stream); 0 = success
    def _device_malloc(self, ctx, out, size, stream):
        p = C.c_void_p()
        if self._hip.hipMalloc(C.byref(p), size) != 0 or not p.value:
            self.errors.append(("hipMalloc", size))
            return 1
        # the library's streams are non-blocking: they do not order against the null stream, so the fill must be complete on return
        if self._hip.hipMemset(p, self.byte, size) != 0 or self._hip.hipDeviceSynchronize() != 0:
            self.errors.append(("hipMemset", size))
            self._hip.hipFree(p)
            return 1
        self.calls += 1
        self.device_calls += 1
        self.live[p.value] = size
        out[0] = p.value
        return 0

    def _device_free(self, ctx, p, size, stream):
        if self.live.pop(p, None) != size:
            self.errors.append(("device_free of a pointer / size never handed out", p, size))
        return self._hip.hipFree(p)

    def _pinned_malloc(self, ctx, out, size, stream):
        p = C.c_void_p()
        if self._hip.hipHostMalloc(C.byref(p), size, 0) != 0 or not p.value:
            self.errors.append(("hipHostMalloc", size))
            return 1
        C.memset(p, self.byte, size)
        self.calls += 1
        self.pinned_calls += 1
        self.live_pinned[p.value] = size
        out[0] = p.value
        return 0

    def _pinned_free(self, ctx, p, size, stream):
        if self.live_pinned.pop(p, None) != size:
            self.errors.append(("pinned_free of a pointer / size never handed out", p, size))
        return self._hip.hipHostFree(p)

    # ---- what the tests use
    def hipjpeg_allocators(self):
        """hipjpegAllocators_t for hipjpegSetAllocators (lowlevel.Batch*(allocators=self))"""
        a = self._N.Allocators()
        a.device_malloc, a.device_free = self._cb[0], self._cb[1]
        if self.pinned:
            a.pinned_malloc, a.pinned_free = self._cb[2], self._cb[3]
        return a

    def plugin_allocators(self):
        """(nvimgcodecDeviceAllocator_t, nvimgcodecPinnedAllocator_t or None) for nvimgcodecExecutionParams_t; same functions"""
        from nvimagecodec_amd import abi as A
        cast = lambda f, t: C.cast(f, t)
        da = A.init(A.DeviceAllocator, A.ST_DEVICE_ALLOCATOR, device_malloc=cast(self._cb[0], A.DeviceMalloc), device_free=cast(self._cb[1], A.DeviceFree))
        pa = None
        if self.pinned:
            pa = A.init(A.PinnedAllocator, A.ST_PINNED_ALLOCATOR, pinned_malloc=cast(self._cb[2], A.DeviceMalloc), pinned_free=cast(self._cb[3], A.DeviceFree))
        return da, pa

    def refill(self):
        """The fill again over every live device allocation.  Only on an idle handle, after a synchronise: nothing of the library's may
        be in flight.  (Pinned memory is left alone: the library's host side keeps tables there between the calls of one batch.)"""
        assert self._hip.hipDeviceSynchronize() == 0
        for p, size in self.live.items():
            assert self._hip.hipMemset(C.c_void_p(p), self.byte, size) == 0
        assert self._hip.hipDeviceSynchronize() == 0

    def all_freed(self):
        return not self.live and not self.live_pinned and not self.errors
