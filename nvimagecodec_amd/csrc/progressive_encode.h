// progressive_encode.h -- progressive (SOF2) output on the GPU entropy coder: the host coder's jpeg_simple_progression script with
// per-scan optimal tables, byte-identical to entropy_encode.cpp encode_progressive, with or without restart intervals.
// The per-block routines live in progressive_encode_core.h; the kernels in progressive_encode.hip.  Per batch:
//   summary  one lane per block of every scan: symbol counts of its own symbols, and the block's summary (content, tail, b)
//   runs     one wave per AC scan: the EOB-run recurrence over the summaries -> flushes, their EOBn counts, the run pieces
//   -- the counts of every scan come back in one copy; jpeg_gen_optimal_table and the DHT / SOS bytes on the host --
//   length   one lane per block: own bits, and the flushes' bits; henc_scan (gpu_huffman_encode.hip) turns them into offsets
//   -- the totals come back; one segment (tables + SOS + stuffed data) per scan, the frame header in front of the first --
//   write    one lane per block: what the block owns, at its offset; then gpu_huffman_encode.hip's count / layout / expand
//            stuff and assemble the segments of every file back to back
#pragma once
#include <cstdint>
#include <vector>

#include "entropy_encode.h"
#include "gpu_huffman_encode.h"
#include "progressive_encode_core.h"

namespace hipjpeg {

// The scans of one image (simple_progression order), first blocks counted from `first_block` on, 64-aligned; hist / codes left null.
// Returns the number of per-block entries they take.
// restart_interval (MCUs, 0: none) fills PencScan::rst_blocks.
size_t penc_describe(const EncodeGeometry& g, const int16_t* const coef[3], size_t first_block, std::vector<PencScan>* scans,
                     int restart_interval = 0);

// The GPU coder's algorithm on the host, block by block with the kernels' routines: the whole file, as encode_jfif writes it with
// progressive output and the given restart interval (0: none): the interval-end flushes, the segmented offsets, padding, markers and
// the stuffing that spares them are the kernels' steps, none exists on the device alone.
void encode_progressive_gpu_algorithm(const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], const int16_t* const coef[3],
                                      int restart_interval, std::vector<uint8_t>* out);

// stream = hipStream_t as void*; all launches are asynchronous.  units: 256 blocks each, HencUnit::image = scan index.
// restart = true: the scans may have restart intervals (PencScan::rst_blocks) and the kernels' flavour with the interval arithmetic
// runs; the default launches the kernels of a batch without restart intervals (as launch_henc_*).
int launch_penc_summary(const PencScan* scans, const HencUnit* units, int nunits, uint8_t* sum, void* stream, bool restart = false);
// one wave per scan of ac_scans
int launch_penc_runs(const PencScan* scans, const uint32_t* ac_scans, int nac, const uint8_t* sum, uint32_t* pre, uint32_t* post, uint32_t* piece,
                     uint32_t* flusher, uint16_t* rel, void* stream, bool restart = false);
int launch_penc_length(const PencScan* scans, const HencUnit* units, int nunits, const uint32_t* pre, const uint32_t* post, uint16_t* own,
                       uint16_t* bits, void* stream, bool restart = false);
// segs[scan].raw: the scan's zeroed bit buffer; with restart intervals the marker bitmap behind it (henc_map_offset(raw_bytes))
int launch_penc_write(const PencScan* scans, const HencImage* segs, const HencUnit* units, int nunits, const PencBlockArrays& a, void* stream,
                      bool restart = false);

}  // namespace hipjpeg
