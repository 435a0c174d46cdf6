// decode_kernels.h -- host-callable launchers of the decode kernels (implemented in decode_kernels.hip; those of the kernels that read
// finished planes -- K3, CMYK, scaled colour, geometry -- in plane_color_kernels.hip).
// `stream` is a hipStream_t passed as void* so that plain C++ translation units need no HIP headers.
#pragma once
#include "device_layout.h"

namespace hipjpeg {

// K1: IDCT of component blocks into u8 planes.  One WorkUnit = 128 blocks.  (Rounds 1-2 had three builds of K1 and K2 for three
// pass-1 arithmetics chosen per image; since round 3 the transform is the SIMD routine's int16 arithmetic for every image.)
// fast_idct: the JDCT_IFAST flavour of K1 / K2 (jsimd_idct_ifast_sse2 restated); the descriptors' qpk must then hold the IFAST multiplier
// tables (DecodeComponent::qpk).  The FUSED builds have no such flavour.
int launch_idct_plane(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream, bool fast_idct = false);
// K2: fused luma IDCT + chroma upsample (factors hs x vs, 0 = no chroma) + colour conversion + store.
// layout: which instantiation of the fused luma kernel (decode_kernels.hip luma_color_body): 0 = generic (format flags read at run
// time), 1 = COMMON (YCbCr source, interleaved RGB / BGR, fancy upsampling), 2 = COMMON with planar RGB / BGR output
constexpr int kNumLumaLayouts = 3;
int launch_luma_color(int layout, int hs, int vs, const DecodeImage* images, const WorkUnit* units, int nunits, void* stream, bool fast_idct = false);
// FUSED builds of K1 / K2 for images of the GPU entropy stage (baseline): the blocks are Huffman-decoded inside the kernel, into the LDS
// slots the IDCT reads, from the start positions the position pass recorded (HuffImage::block_pos) -- no coefficient block is written
// to or read from HBM.  himages = the batch's HuffImage array (DecodeImage::huff_index points into it), pool_bytes = dynamic LDS for
// the largest lookup-table pool of the batch.  Same work units as the plain builds.
struct HuffImage;
int launch_idct_plane_fused(const DecodeImage* images, const WorkUnit* units, int nunits, HuffImage* himages, unsigned pool_bytes, void* stream);
int launch_luma_color_fused(int layout, int hs, int vs, const DecodeImage* images, const WorkUnit* units, int nunits, HuffImage* himages, unsigned pool_bytes,
                            void* stream);
// K3: per-pixel colour stage from planes (replication upsampling) for uncommon sampling layouts.
int launch_generic_color(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream);
// Four-component frames (CMYK / YCCK): upsampling + the reference's CMYK -> RGB step, one WorkUnit per pixel row.
int launch_cmyk_color(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream);
// Scaled decode (DecodeImage::scale_k != 0), kernels of their own beside K1 / K2 / K3:
// the reduced IDCTs of libjpeg-turbo (jsimd_idct_4x4_sse2, jsimd_idct_2x2_sse2, jpeg_idct_1x1 restated) of a component whose
// DecodeComponent::scaled is 4, 2 or 1, into its plane; one WorkUnit = 128 blocks, as for K1.  Components with scaled == 8 take K1.
int launch_idct_reduced_plane(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream);
// ... and from the planes to the output: jdsample.c's upsampler choice on the scaled groups, YCbCr / RGB / gray, any format but the raw
// planes; one WorkUnit = kScaledRowsPerUnit pixel rows of the scaled picture (block_base = the first).
int launch_scaled_color(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream);
// Geometry pass (region of interest + EXIF orientation): WorkUnit{image = TransformImage index, block_base = first output row}.
int launch_transform(const TransformImage* images, const WorkUnit* units, int nunits, void* stream);

}  // namespace hipjpeg
