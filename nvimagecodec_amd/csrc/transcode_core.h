// transcode_core.h -- lossless transcode (hipjpegTranscode*): which sources the coder can take, the picture as the coder sees it,
// and the host-only route (host entropy decoder -> relayout -> host coder).  The device route (hipjpeg_api.cpp) plans a DecodeBatch
// for coefficients only, lets coef_relayout_kernel (transcode_kernels.hip) fill an EncodeBatch's coefficient area and goes on through
// the unchanged entropy stage of the encoder.
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

// The header rules of include/hipjpeg.h (frame type, components, colour model, sampling, tables): SUCCESS and *p, or UNSUPPORTED.
hipjpegStatus_t transcode_picture(const FrameInfo& f, TranscodePicture* p);
// INVALID_ARGUMENT for a restart interval outside 0..65535 or a reserved field that is not 0.
hipjpegStatus_t transcode_params_ok(const hipjpegTranscodeParams_t& p);
EntropyEncodeOptions transcode_options(const hipjpegTranscodeParams_t& p);
// Host route.  Appends the file to `out`; nothing is appended unless the status is SUCCESS.
hipjpegStatus_t transcode_host(const uint8_t* data, size_t size, const hipjpegTranscodeParams_t& params, std::vector<uint8_t>* out);

}  // namespace hipjpeg
