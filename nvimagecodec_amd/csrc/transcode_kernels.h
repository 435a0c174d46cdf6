// transcode_kernels.h -- host-callable launcher of the lossless transcode's kernel (transcode_kernels.hip); stream = hipStream_t as void*.
#pragma once
#include <cstdint>

#include "device_layout.h"
#include "encode_layout.h"

namespace hipjpeg {

constexpr int kRelayoutBlocksPerUnit = 256;  // one workgroup: two rounds of four passes of 32 blocks, eight lanes per block

// One workgroup's worth of work: kRelayoutBlocksPerUnit consecutive blocks (raster order over the REAL block area, real_w x real_h of
// the EncodeImage) of one component of one image; the same index addresses DecodeImage[] and EncodeImage[].
struct RelayoutUnit {
    uint32_t image, comp, first_block, pad;
};

// Copies the real blocks of every unit from the decoder's layout (DecodeImage: column-major blocks over the frame's grid, DC at
// dc[b * dc_stride]) to the coder's (EncodeImage::coef: zigzag-order blocks over the coder's grid).  out_of_range[image] gets bit 0 set
// when a DC value leaves [-1024, 1023] or an AC value [-1023, 1023]; the caller clears the words first.
int launch_coef_relayout(const DecodeImage* src, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream);

}  // namespace hipjpeg
