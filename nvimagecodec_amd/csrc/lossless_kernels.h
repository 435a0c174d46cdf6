// lossless_kernels.h -- launches of the lossless reconstruction kernels (lossless_kernels.hip); descriptors in lossless_core.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include "lossless_core.h"

namespace hipjpeg {

// Ps = 1: running sums of the column-0 differences (one wave per plane), then one workgroup per row.  max_height: of these planes.
hipError_t launch_lossless_rows(const LosslessPlane* planes, int num_planes, int max_height, hipStream_t stream);
// any Ps: one wave per plane
hipError_t launch_lossless_wavefront(const LosslessPlane* planes, int num_planes, hipStream_t stream);

}  // namespace hipjpeg
