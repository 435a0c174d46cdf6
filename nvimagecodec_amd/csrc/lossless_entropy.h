// lossless_entropy.h -- host entropy stage of the lossless (SOF3) decoder: the rules a frame must meet, and the Huffman symbols of
// its one scan decoded into uint16 DIFFERENCE planes, one per component.  No prediction happens here: that is the reconstruction
// kernels' work (lossless_kernels.hip) or, on the host, lossless_core.cpp's.
#pragma once
#include <cstddef>
#include <cstdint>

#include "jpeg_syntax.h"

namespace hipjpeg {

struct LosslessFrame {
    int width = 0, height = 0, ncomp = 0, precision = 0;
    int comp_id[4] = {0, 0, 0, 0};
    int ps = 0, pt = 0;
    int restart_rows = 0;     // rows per restart interval; 0 = the file has none
    int scan_comp[4] = {0, 0, 0, 0};  // frame component coded at each position of a pixel
    HuffSpec table[4];        // the table of each such position
    size_t data_begin = 0, data_end = 0;
    int interval_rows() const { return restart_rows ? restart_rows : height; }
    int init() const { return 1 << (precision - pt - 1); }
};

// Parses `data` as a lossless frame and applies the rules (hipjpeg.h, hipjpegGetLosslessInfo): SUCCESS, UNSUPPORTED for a valid file
// outside them, BAD_JPEG for a malformed one, TRUNCATED when a marker segment is cut.
hipjpegStatus_t lossless_frame(const uint8_t* data, size_t size, LosslessFrame* out);

// Differences of component c go to planes[c], `pitch` samples per row.  SSSS = 0..15 as usual; SSSS = 16 is 32768 with no extra bits.
// TRUNCATED: the data ends before the last sample; CORRUPT: a code no table holds, a restart marker missing, early or out of turn.
hipjpegStatus_t lossless_entropy_decode(const uint8_t* data, const LosslessFrame& f, uint16_t* const planes[4], size_t pitch);

}  // namespace hipjpeg
