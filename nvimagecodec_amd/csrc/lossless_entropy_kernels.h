// lossless_entropy_kernels.h -- launches of the lossless decoder's GPU entropy stage (lossless_entropy_kernels.hip); the algorithm and
// the descriptors are in lossless_gpu_core.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include "lossless_gpu_core.h"

namespace hipjpeg {

// The device arrays of one batch.  Batch-wide indices: subsequences through LlSegment::first_subseq, chunks through first_chunk.
struct LlArrays {
    const LlImage* images;
    const LlSegment* segments;
    const LlUnit* chunk_units;  // {segment, chunk inside it}
    const LlUnit* units;        // {segment, first subsequence}: the units of a segment lie together, in order
    int num_chunk_units, num_units;
    uint32_t* drops;      // per chunk: stuffed bytes in it
    uint32_t* seg_bits;   // per segment: bits of its destuffed stream (the last chunk's workgroup writes it)
    uint64_t* start;      // per subsequence: the state its last parse started from, where that parse ended, and its samples
    uint64_t* end;
    uint32_t* count;
    uint64_t* unit_out;   // 2 x num_units: the end state of a unit's last subsequence, as launch L left it, at [(L & 1) * num_units + unit]
    uint32_t* unit_count; // per unit: samples of its subsequences
    uint32_t* verdicts;   // per image: kLl* bits, or-ed by the write pass; cleared by the caller
    uint32_t* moved;      // kLlMaxRipple + 1 words: workgroups that had work in launch L; cleared by the caller
};

// destuff (count, compact), pass 0 and the ripple launches
hipError_t launch_lossless_entropy_sync(const LlArrays& a, hipStream_t stream);
// checks, per-segment sums, stores
hipError_t launch_lossless_entropy_write(const LlArrays& a, hipStream_t stream);

}  // namespace hipjpeg
