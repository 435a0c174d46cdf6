// lossless_encode_host.h -- host side of the lossless coder (lossless_encode_host.cpp): argument rules, descriptors, the table and the
// headers libjpeg-turbo writes, the plain host coder and the kernels' schedule run on the host.
#pragma once
#include <vector>

#include "../../include/hipjpeg.h"
#include "lossless_encode_core.h"

namespace hipjpeg {

// The argument rules of hipjpeg.h; on success `im` describes the picture at the input's addresses (first_group, index, counts and
// codes are the planner's to fill).
hipjpegStatus_t lossless_encode_describe(const hipjpegLosslessEncodeInput_t& in, const hipjpegLosslessEncodeParams_t& p, LencImage* im);

inline uint32_t lenc_intervals(const LencImage& im) { return (im.height + im.interval_rows - 1) / im.interval_rows; }

// From the category counts of all components: the table as code | size << 16 per category, and SOI .. SOS as the library writes them.
void lossless_encode_headers(const LencImage& im, const hipjpegLosslessEncodeParams_t& p, const uint32_t counts[kLencSymbols],
                             uint32_t codes[kLencSymbols], std::vector<uint8_t>* header);

// Appends a complete file to `out` (descriptor addresses are host addresses).
void lossless_encode_plain(const LencImage& im, const hipjpegLosslessEncodeParams_t& p, std::vector<uint8_t>* out);
void lossless_encode_gpu_algorithm(const LencImage& im, const hipjpegLosslessEncodeParams_t& p, std::vector<uint8_t>* out);

}  // namespace hipjpeg
