// kernel_common.h -- what several of the .hip files need word for word: address-space qualifiers, vector and pointer aliases, the
// wave-level LDS hand-off and the transcode range test.  Device code only; every .hip includes it right behind <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hipjpeg {

// Explicitly GLOBAL pointers for the hot loads and stores: through the generic pointers of the descriptors hipcc emits FLAT
// instructions (64-bit address arithmetic per access, and they count against the LDS counter as well).
#define HJ_GLOBAL __attribute__((address_space(1)))
#define HJ_LDS __attribute__((address_space(3)))

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // plain vector type: usable behind address-space pointers
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

using lds_char = __attribute__((address_space(3))) char;
using lds_u16 = __attribute__((address_space(3))) unsigned short;
using lds_u32x4 = __attribute__((address_space(3))) u32x4;
// the descriptors' pointers come out of memory as generic ones: say that they point into global memory, so that the loads and stores
// are global_* instructions (flat ones also count as LDS operations and would tie the two waits together)
using gbl_u32x4 = __attribute__((address_space(1))) u32x4;
using gbl_i16 = __attribute__((address_space(1))) int16_t;

// LDS operations of one wave execute in order; only the compiler has to be kept from reordering across the hand-off
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// is either half of a dword, as int16, outside [-1023, 1023]?  (no branches: bitwise ors)
__device__ __forceinline__ unsigned pair_outside(unsigned w)
{
    const int a = (int)(short)(w & 0xFFFFu), b = (int)w >> 16;
    return (unsigned)(a < -1023) | (unsigned)(a > 1023) | (unsigned)(b < -1023) | (unsigned)(b > 1023);
}

}  // namespace hipjpeg
