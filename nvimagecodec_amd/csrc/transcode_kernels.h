// transcode_kernels.h -- host-callable launchers of the lossless transcode's kernels (transcode_kernels.hip); stream = hipStream_t as void*.
#pragma once
#include <cstdint>

#include "device_layout.h"
#include "encode_layout.h"

namespace hipjpeg {

constexpr int kRelayoutBlocksPerUnit = 256;  // one workgroup: two rounds of four passes of 32 blocks, eight lanes per block

// One workgroup's worth of work: kRelayoutBlocksPerUnit consecutive blocks (raster order over the REAL block area, real_w x real_h of
// the EncodeImage) of one component of one image; the same index addresses DecodeImage[] and EncodeImage[].
// `pad`: 0 for coef_relayout_kernel; for coef_transform_kernel the picture's turn (transcode_core.h kTurn*: bit 0 transpose, bit 1
// mirror x, bit 2 mirror y of the output) and, from bit 3 and bit 16 on, 13 bits each: the block column and row of the decoder's grid at which
// this component of a cropped picture begins (kOrigin* below; 0, 0 for a picture that is not cropped).
struct RelayoutUnit {
    uint32_t image, comp, first_block, pad;
};
// the origin inside `pad`: block coordinates of a 65535-sample axis stay below 8192
constexpr unsigned kOriginShiftX = 3, kOriginShiftY = 16, kOriginMask = 0x1FFFu;

// Copies the real blocks of every unit from the decoder's layout (DecodeImage: column-major blocks over the frame's grid, DC at
// dc[b * dc_stride]) to the coder's (EncodeImage::coef: zigzag-order blocks over the coder's grid).  out_of_range[image] gets bit 0 set
// when a DC value leaves [-1024, 1023] or an AC value [-1023, 1023]; the caller clears the words first.
int launch_coef_relayout(const DecodeImage* src, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream);
// The same for turned pictures: the units walk the OUTPUT's real blocks (EncodeImage describes the output), each block comes from the
// source block the unit's turn and origin name, transposed and with the mirrors' sign changes.  The range flags are set from the source's values.
int launch_coef_transform(const DecodeImage* src, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream);

}  // namespace hipjpeg
