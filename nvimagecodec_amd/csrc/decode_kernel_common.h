// decode_kernel_common.h -- what decode_kernels.hip (the kernels that take coefficient blocks) and plane_color_kernels.hip (the kernels
// that read finished planes) both need.  Device code only.
#pragma once
#include "kernel_common.h"

#include "decode_kernels.h"
#include "device_layout.h"

namespace hipjpeg {

constexpr int kThreads = 256;

__device__ __forceinline__ unsigned pack4(int a, int b, int c, int d) { return (unsigned)a | ((unsigned)b << 8) | ((unsigned)c << 16) | ((unsigned)d << 24); }

}  // namespace hipjpeg
