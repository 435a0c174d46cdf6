// coefficient_kernels.h -- host-callable launchers of the coefficient-tensor kernels (coefficient_kernels.hip); stream = hipStream_t as void*.
#pragma once
#include <cstdint>

#include "device_layout.h"
#include "encode_layout.h"
#include "transcode_kernels.h"

namespace hipjpeg {

// One component of one picture in the caller's memory (include/hipjpeg.h hipjpegCoefficientPlanes_t): int16[64] blocks in natural order,
// block (by, bx) of the real_w x real_h area at coef + (by * pitch + bx) * 64.  The table holds four records per image, component c of
// image i at [i * 4 + c].  One 16-byte-aligned record per component and nothing narrower than a dword in it: a kernel that takes its
// component number at run time computes ONE aligned base and reads the members at constant offsets (device_layout.h DecodeComponent).
struct alignas(16) CoefPlane {
    int16_t* coef;
    uint32_t pitch, real_w, real_h, pad;
};
static_assert(sizeof(CoefPlane) == 32, "four records per image, 16-byte aligned");

// The units are RelayoutUnit as for the transcode kernels: kRelayoutBlocksPerUnit consecutive blocks, in raster order over the real area
// (CoefPlane::real_w x real_h), of one component of one image; `pad` is 0.
// Export: the decoder's layout (DecodeImage: column-major blocks over the frame's MCU-padded grid, DC at dc[b * dc_stride]) to the
// caller's planes.  Components 0..3.
int launch_coef_export(const DecodeImage* src, const CoefPlane* planes, const RelayoutUnit* units, int nunits, void* stream);
// Import: the caller's planes to the coder's layout (EncodeImage::coef: zigzag-order blocks over the coder's grid, real blocks only).
// Components 0..2.  out_of_range[image] gets bit 0 set when a DC value leaves [-1024, 1023] or an AC value [-1023, 1023]; the caller
// clears the words first.
int launch_coef_import(const CoefPlane* planes, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream);
// To the decoder (hipjpegCoefficientsToPixelsBatch): the caller's planes to the decoder's layout with the DC value inside the block
// (DecodeComponent::coef, dc == coef, dc_stride == 64, as for host-decoded pictures).  Components 0..3.  Here -- and only here -- a unit's
// first_block counts over the component's MCU-PADDED grid (DecodeComponent::blocks_w x blocks_h): the kernel writes every block of the
// grid, zeros outside the real area, because K1 reads the whole grid and the arena holds what an earlier batch left there.  No range
// guard: any int16 is a coefficient the decoder has arithmetic for.
int launch_coef_to_decoder(const CoefPlane* planes, const DecodeImage* dst, const RelayoutUnit* units, int nunits, void* stream);
// From the coder (hipjpegPixelsToCoefficientsBatch): the coder's layout (EncodeImage::coef, as the forward kernels leave it) to the
// caller's planes, real blocks only.  Components 0..2.
int launch_coef_from_coder(const EncodeImage* src, const CoefPlane* planes, const RelayoutUnit* units, int nunits, void* stream);

}  // namespace hipjpeg
