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
//
// Before the turn come, in this order, the drop of the chroma components (transcode_picture's grayscale mode) and the crop
// (transcode_crop: a block origin per component, added to the source block's coordinates after the mirrors and the transpose are undone).
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
// ... and where in the source's grid they start: per component the block origin of a cropped picture (behind the turn in `pad`:
// transcode_kernels.h kOrigin*)
struct TranscodeOrigin {
    int ox[3] = {0, 0, 0}, oy[3] = {0, 0, 0};
    bool any() const { return (ox[0] | oy[0] | ox[1] | oy[1] | ox[2] | oy[2]) != 0; }
};
constexpr uint32_t kTranscodeFlags = HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF | HIPJPEG_TRANSCODE_TRIM | HIPJPEG_TRANSCODE_GRAYSCALE |
                                     HIPJPEG_TRANSCODE_CROP_EXPAND | HIPJPEG_TRANSCODE_COPY_MARKERS;

// The header rules of include/hipjpeg.h (frame type, components, colour model, sampling, tables): SUCCESS and *p, or UNSUPPORTED.
// `grayscale` (HIPJPEG_TRANSCODE_GRAYSCALE): the one-component picture of a YCbCr source's luma; the chroma-only rules are waived.
hipjpegStatus_t transcode_picture(const FrameInfo& f, bool grayscale, TranscodePicture* p);
// INVALID_ARGUMENT for a restart interval outside 0..65535 or an orientation field with an orientation of 1 or above 8, an orientation next
// to HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF, or a bit that is none of the flags.
hipjpegStatus_t transcode_params_ok(const hipjpegTranscodeParams_t& p);
// The picture `src` (of transcode_picture) cut to `region` (nullptr or all zeros: the whole picture, `src` itself) and the block origins
// its components are read from.  INVALID_ARGUMENT for a region outside the picture or empty, UNSUPPORTED for an origin off the iMCU grid
// unless `expand` moves it left / up onto it.
hipjpegStatus_t transcode_crop(const TranscodePicture& src, const hipjpegTranscodeRegion_t* region, bool expand, TranscodePicture* dst,
                               TranscodeOrigin* origin);
// The source's APPn / COM segments as the output carries them (empty without HIPJPEG_TRANSCODE_COPY_MARKERS), the EXIF orientation reset
// when `orientation` (of transcode_orientation) is a turn.
void transcode_markers(const hipjpegTranscodeParams_t& p, int orientation, const uint8_t* data, size_t size, std::vector<uint8_t>* markers);
// The orientation 1..8 the (valid) parameters ask for, the source's own EXIF tag where they say so.
int transcode_orientation(const hipjpegTranscodeParams_t& p, const uint8_t* data, size_t size);
// The picture `src` (of transcode_picture) brought upright for `orientation`, and the kTurn* bits that say where its blocks come from.
// Applies the iMCU rule for mirrored axes (perfect, or trimmed when `trim`) and the sampling rule for transposing turns: SUCCESS or
// UNSUPPORTED.  Orientation 1 returns `src` and 0.
hipjpegStatus_t transcode_turn(const TranscodePicture& src, int orientation, bool trim, TranscodePicture* dst, unsigned* turn);
EntropyEncodeOptions transcode_options(const hipjpegTranscodeParams_t& p);

// Coefficients in the public layout of include/hipjpeg.h (hipjpegCoefficientPlanes_t): int16[64] blocks in natural order (row * 8 +
// column), raster order over the component's real block area blocks_w x blocks_h = ceil(samp / 8), block (by, bx) at
// coef + (by * pitch + bx) * 64.  The host route below goes through it, so that a transcode IS a read followed by a write.
struct NaturalPlanes {
    int16_t* coef[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t pitch[4] = {0, 0, 0, 0};
    int blocks_w[4] = {0, 0, 0, 0}, blocks_h[4] = {0, 0, 0, 0};
};
// The real block area of every component of `f` (pointers and pitches are left for the caller).
void natural_area(const FrameInfo& f, NaturalPlanes* p);
// Read: the host entropy decoder's output (column-major blocks over the MCU-padded grid) re-laid into `dst`.  The decoder's status for a
// damaged stream, and then nothing is written.
hipjpegStatus_t decode_natural(const uint8_t* data, size_t size, const FrameInfo& f, const NaturalPlanes& dst);
// Write: the picture `pic` whose blocks come from `src` by `origin` and `turn` (all zero: its own places), natural order to zigzag over the
// coder's grid with the range check (UNSUPPORTED), then the unchanged host coder.  Appends the file to `out`.
hipjpegStatus_t encode_natural(const TranscodePicture& pic, const NaturalPlanes& src, const TranscodeOrigin& origin, unsigned turn,
                               const EntropyEncodeOptions& opt, std::vector<uint8_t>* out);
// Host route.  Appends the file to `out`; nothing is appended unless the status is SUCCESS.
hipjpegStatus_t transcode_host(const uint8_t* data, size_t size, const hipjpegTranscodeParams_t& params, const hipjpegTranscodeRegion_t* region,
                               std::vector<uint8_t>* out);

}  // namespace hipjpeg
