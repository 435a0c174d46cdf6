// transcode_core.h -- lossless transcode (hipjpegTranscode*): which sources the coder can take, the picture as the coder sees it,
// and the host-only route (host entropy decoder -> relayout -> host coder).  The device route (hipjpeg_api.cpp) plans a DecodeBatch
// for coefficients only, lets coef_relayout_kernel (transcode_kernels.hip) fill an EncodeBatch's coefficient area and goes on through
// the unchanged entropy stage of the encoder.
//
// Lossless turns (hipjpegTranscodeParams_t::orientation; transupp.c's identities).  With u the horizontal and v the vertical frequency
// of natural position v * 8 + u: a horizontal mirror reverses the block columns and negates odd u, a vertical mirror reverses the block
// rows and negates odd v, a transpose sends block (by, bx) to (bx, by) and coefficient (u, v) to (v, u).  Every orientation is "transpose
// or not", then "mirror x or not" and "mirror y or not" in the OUTPUT's frame (kTurn* bits): 6 = transpose | mirror x, 8 = transpose |
// mirror y, 7 = all three.  The host route below applies them in plain C++ and is the definition coef_transform_kernel reproduces.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/hipjpeg.h"
#include "entropy_encode.h"
#include "jpeg_syntax.h"

namespace hipjpeg {

// jchuff.c's limits for 8-bit data (MAX_COEF_BITS 10): with DC in this range no DC difference exceeds category 11
constexpr int kTranscodeDcMin = -1024, kTranscodeDcMax = 1023, kTranscodeAcMax = 1023;

// A source picture as encode_jfif / the GPU coder take it: geometry and the source's own quantization tables (natural order).
struct TranscodePicture {
    EncodeGeometry geom;
    uint16_t qlum[64], qchr[64];
};

// How the output's blocks come from the source's (uniform per image; RelayoutUnit::pad carries it to the kernel)
constexpr unsigned kTurnTranspose = 1u, kTurnMirrorX = 2u, kTurnMirrorY = 4u;

// The header rules of include/hipjpeg.h (frame type, components, colour model, sampling, tables): SUCCESS and *p, or UNSUPPORTED.
hipjpegStatus_t transcode_picture(const FrameInfo& f, TranscodePicture* p);
// INVALID_ARGUMENT for a restart interval outside 0..65535 or an orientation field with an orientation of 1 or above 8, an orientation next
// to HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF, or a bit that is neither flag.
hipjpegStatus_t transcode_params_ok(const hipjpegTranscodeParams_t& p);
// The orientation 1..8 the (valid) parameters ask for, the source's own EXIF tag where they say so.
int transcode_orientation(const hipjpegTranscodeParams_t& p, const uint8_t* data, size_t size);
// The picture `src` (of transcode_picture) brought upright for `orientation`, and the kTurn* bits that say where its blocks come from.
// Applies the iMCU rule for mirrored axes (perfect, or trimmed when `trim`) and the sampling rule for transposing turns: SUCCESS or
// UNSUPPORTED.  Orientation 1 returns `src` and 0.
hipjpegStatus_t transcode_turn(const TranscodePicture& src, int orientation, bool trim, TranscodePicture* dst, unsigned* turn);
EntropyEncodeOptions transcode_options(const hipjpegTranscodeParams_t& p);
// Host route.  Appends the file to `out`; nothing is appended unless the status is SUCCESS.
hipjpegStatus_t transcode_host(const uint8_t* data, size_t size, const hipjpegTranscodeParams_t& params, std::vector<uint8_t>* out);

}  // namespace hipjpeg
