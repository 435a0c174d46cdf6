// lossless_host.h -- host side of the lossless decoder (lossless_core.cpp): output rules, plane descriptors, reconstruction on the CPU.
#pragma once
#include "lossless_core.h"
#include "lossless_entropy.h"

namespace hipjpeg {

// INVALID_ARGUMENT: sample size other than 1 or 2, a missing plane, a pitch that does not hold a row; UNSUPPORTED: uint8 samples asked
// of a frame whose precision is above 8.
hipjpegStatus_t lossless_output_ok(const LosslessFrame& f, const hipjpegLosslessOutput_t& o);

// The descriptors of the frame's components: differences at diff[c] (lossless_diff_pitch samples per row), scratch at scratch[c].
void lossless_planes(const LosslessFrame& f, const hipjpegLosslessOutput_t& o, const uint64_t diff[4], const uint64_t scratch[4], LosslessPlane out[4]);

// One plane in host memory (descriptor addresses are host addresses; scratch is not used): the rules applied sample by sample, and the
// two kernels' schedules.
void lossless_reconstruct_plain(const LosslessPlane& p);
void lossless_rows_schedule(const LosslessPlane& p);
void lossless_wavefront_schedule(const LosslessPlane& p);

// schedule: -1 plain, 0 the planner's kernel, 1 rows, 2 wavefront
hipjpegStatus_t lossless_decode_host(const uint8_t* data, size_t length, const hipjpegLosslessOutput_t& output, int schedule);

}  // namespace hipjpeg
