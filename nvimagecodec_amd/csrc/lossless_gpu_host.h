// lossless_gpu_host.h -- host side of the lossless decoder's GPU entropy stage: the marker scan that cuts a scan into segments, the
// lookup tables, and the twin that runs the kernels' schedule (lossless_entropy_kernels.hip) lane by lane on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lossless_entropy.h"
#include "lossless_gpu_core.h"

namespace hipjpeg {

struct LlRawSegment {
    size_t begin, end;  // bytes of the file: one restart interval without its marker
};

// The intervals of the frame's scan, found with a byte scan: markers RST0..7 in turn, fill bytes allowed in front of them, as
// lossless_entropy_decode takes them.  No Huffman work.  false: the image is one for the host stage, which names what is wrong or
// decodes what the GPU stage does not take -- a marker missing, early, out of turn or of another kind, an empty interval, a table of
// more than kLlSpecSymbols symbols, or a scan of 2^29 bytes or more (bit positions are 32-bit in the kernels; the bound is on the
// stuffed bytes, which are no fewer than the destuffed ones).
bool lossless_gpu_segments(const uint8_t* data, const LosslessFrame& f, std::vector<LlRawSegment>* out);

// specs: room for 4 * kLlSpecWords words (the tables as they travel: lossless_gpu_core.h).  Returns the number of tables: 1 where every
// position of a pixel names the same one.
uint32_t lossless_gpu_tables(const LosslessFrame& f, uint32_t* specs);

// rows x width x ncomp of interval k, and its first row
inline uint32_t lossless_gpu_first_row(const LosslessFrame& f, size_t k) { return (uint32_t)(k * (size_t)f.interval_rows()); }
inline uint64_t lossless_gpu_samples(const LosslessFrame& f, size_t k)
{
    const int row0 = (int)lossless_gpu_first_row(f, k);
    const int rows = row0 + f.interval_rows() < f.height ? f.interval_rows() : f.height - row0;
    return (uint64_t)rows * (uint64_t)f.width * (uint64_t)f.ncomp;
}

// The kernels' schedule on the CPU: destuff, pass 0, rounds, ripple launches, checks, sums, stores.  Differences of frame component c
// to planes[c], `pitch` samples per row.  *verdict: the kLl* bits the write pass would leave (0: the planes are final).  false: the
// image is one for the host stage from the start (lossless_gpu_segments), nothing ran.
bool lossless_gpu_algorithm_host(const uint8_t* data, const LosslessFrame& f, uint16_t* const planes[4], size_t pitch, uint32_t* verdict);

}  // namespace hipjpeg
