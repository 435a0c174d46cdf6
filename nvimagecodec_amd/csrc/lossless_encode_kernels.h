// lossless_encode_kernels.h -- launches of the lossless coder's kernels (lossless_encode_kernels.hip); the arithmetic and the shape
// are in lossless_encode_core.h.  The samples never leave HBM:
//   stats    per row piece: difference and category of every sample, 17 counters per workgroup in LDS, one global atomic each
//   -- the host reads the counts, builds each picture's table and SOI .. SOS --
//   length   one lane per group of kLencGroup samples of the scan: what the group does to the bit offset (a packed HencSpan)
//   scan     per picture: exclusive segmented scan of the spans -> bit offset of every group, total bits
//   -- the host reads the totals and lays out the bit buffers --
//   write    one lane per group: the bits at the group's offset, assembled per workgroup in an LDS window, whole words out, the two
//            end words OR-ed; padding, RSTn and the marker bitmap by the lane whose group holds an interval's last sample
// Stuffing and file assembly are gpu_huffman_encode.hip's count / layout / expand kernels over HencImage descriptors that the planner
// fills (bit buffer, marker bitmap, header).
#pragma once
#include <hip/hip_runtime_api.h>

#include "gpu_huffman_encode.h"
#include "lossless_encode_core.h"

namespace hipjpeg {

struct LencUnit {
    uint32_t image, first;  // a workgroup of the length / write kernels: descriptor, its first group
};

// counts: written through LencImage::counts, zeroed by the caller on the same stream
hipError_t launch_lenc_stats(const LencImage* images, int nimages, hipStream_t stream);
hipError_t launch_lenc_length(const LencImage* images, const LencUnit* units, int nunits, uint32_t* spans, hipStream_t stream);
hipError_t launch_lenc_scan(const LencImage* images, int nimages, const uint32_t* spans, uint32_t* offsets, uint32_t* totals, hipStream_t stream);
// out[LencImage::index]: raw (zeroed, with the bitmap behind it) and raw_bytes
hipError_t launch_lenc_write(const LencImage* images, const LencUnit* units, int nunits, const HencImage* out, const uint32_t* offsets,
                             hipStream_t stream);

}  // namespace hipjpeg
