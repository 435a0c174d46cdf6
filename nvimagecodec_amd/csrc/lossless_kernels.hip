// lossless_kernels.hip -- reconstruction of lossless JPEG pictures from their difference planes (rules and arithmetic: lossless_core.h).
//
//   lossless_col0_kernel + lossless_rows_kernel   Ps = 1.  Inside a restart interval column 0 is a vertical running sum of the
//       column-0 differences and every row a horizontal running sum that starts from it, all mod 2^16.  The first kernel (one wave per
//       plane) leaves the running column-0 sums of the whole plane in scratch; a row's base is then init + S[row] - S[row in front
//       of its interval].  The second gives a workgroup one row: each lane loads 16 bytes (eight differences) per chunk, sums them,
//       the wave scans the lane totals with shuffles, the four wave totals meet in the LDS, and the chunk's total is carried to the
//       next chunk of the row.
//   lossless_wavefront_kernel   Ps = 1..7.  One wave per plane walks bands of 64 rows.  Lane r owns row r of the band and runs one
//       column behind lane r - 1: at every step its b is what lane r - 1 produced the step before (one shuffle) and its c the b it
//       held before that.  Differences come through the LDS in tiles of 64 x 64, loaded 16 bytes per lane; the state replaces them
//       in place and a finished tile leaves for the caller's buffer row by row, 64 consecutive samples per store.  Row 0 of a tile
//       slot holds the state of the row above the band, which the band before left in scratch.
//
// Both apply the point transform and the 8-bit truncation on the way out and write the caller's layout; nothing is read back from it.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "lossless_kernels.h"

namespace hipjpeg {

namespace {

using gbl_u8 = __attribute__((address_space(1))) uint8_t;
using gbl_u16 = __attribute__((address_space(1))) uint16_t;
using gbl_u32x2 = __attribute__((address_space(1))) u32x2;

// one sample at any address: a halfword where it is aligned, bytes where it is not
__device__ __forceinline__ void store_sample(uint64_t addr, uint32_t v, uint32_t out_bytes)
{
    if (out_bytes == 1) {
        *reinterpret_cast<gbl_u8*>(addr) = (uint8_t)v;
    } else if ((addr & 1) == 0) {
        *reinterpret_cast<gbl_u16*>(addr) = (uint16_t)v;
    } else {
        reinterpret_cast<gbl_u8*>(addr)[0] = (uint8_t)v;
        reinterpret_cast<gbl_u8*>(addr)[1] = (uint8_t)(v >> 8);
    }
}

// inclusive sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_up(v, d);
        if (lane >= d) v += n;
    }
    return v;
}

// The 64 steps of step group g of lossless_wavefront_kernel for predictor PS: lane r is at column g * 64 + k - r in step k.
template <int PS>
__device__ __forceinline__ void wavefront_steps(uint16_t (&tile)[2][kLosslessBandRows + 1][kLosslessTileCols], uint32_t g, int lane, int width, bool live,
                                                bool first_row, int init, int& a, int& b, int& c)
{
    for (int k = 0; k < kLosslessTileCols; k++) {
        const int j = (int)(g * kLosslessTileCols) + k - lane;  // this lane's column at this step
        int above_now = __shfl_up(a, 1);                         // what the lane above produced one step ago: its column j
        const bool in_row = j >= 0 && j < width;
        const uint32_t slot = ((uint32_t)j >> 6) & 1, at = (uint32_t)j & 63;
        if (lane == 0 && in_row) above_now = tile[slot][0][at];
        c = b;
        b = above_now;
        if (live && in_row) {
            const uint32_t d = tile[slot][lane + 1][at];
            a = (int)lossless_state(lossless_predict_at(PS, first_row, (uint32_t)j, init, a, b, c), d);
            tile[slot][lane + 1][at] = (uint16_t)a;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(64) void lossless_col0_kernel(const LosslessPlane* __restrict__ planes)
{
    const LosslessPlane& p = planes[blockIdx.x];
    const int lane = threadIdx.x;
    const gbl_u16* diff = reinterpret_cast<const gbl_u16*>(p.diff);
    gbl_u16* sums = reinterpret_cast<gbl_u16*>(p.scratch);
    const uint32_t height = p.height, pitch = p.diff_pitch;
    uint32_t carry = 0;
    for (uint32_t row0 = 0; row0 < height; row0 += 64) {
        const uint32_t row = row0 + lane;
        uint32_t v = row < height ? diff[(size_t)row * pitch] : 0u;
        v = (wave_inclusive_sum(v, lane) + carry) & 0xFFFFu;
        if (row < height) sums[row] = (uint16_t)v;
        carry = __shfl(v, 63);
    }
}

__global__ __launch_bounds__(kLosslessRowThreads) void lossless_rows_kernel(const LosslessPlane* __restrict__ planes)
{
    __shared__ uint32_t wave_total[2][kLosslessRowThreads / 64];
    const LosslessPlane& p = planes[blockIdx.y];
    const uint32_t row = blockIdx.x;
    if (row >= p.height) return;  // the grid is as tall as the tallest plane of the launch
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t width = p.width, pt = p.pt, out_bytes = p.out_bytes, out_step = p.out_step;
    const gbl_u16* sums = reinterpret_cast<const gbl_u16*>(p.scratch);
    const uint32_t first = row - row % p.restart_rows;
    uint32_t carry = lossless_row_base(p.init, sums[row], first ? sums[first - 1] : 0u);  // the state of column 0
    const gbl_u16* diff = reinterpret_cast<const gbl_u16*>(p.diff) + (size_t)row * p.diff_pitch;
    const uint64_t out_row = p.out + (uint64_t)row * p.out_pitch;
    int parity = 0;
    for (uint32_t chunk0 = 0; chunk0 < width; chunk0 += kLosslessChunkSamples, parity ^= 1) {
        const uint32_t col = chunk0 + threadIdx.x * kLosslessLaneSamples;
        // rows of a difference plane are padded to whole 16-byte pieces: the load stays inside the row's own storage
        u32x4 raw = {0u, 0u, 0u, 0u};
        if (col < width) raw = *reinterpret_cast<const gbl_u32x4*>(diff + col);
        uint32_t v[kLosslessLaneSamples];
#pragma unroll
        for (int i = 0; i < kLosslessLaneSamples; i++) {
            const uint32_t d = (raw[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
            // column 0 is the base itself; samples behind the row's end count nothing
            v[i] = (col + i < width && col + i != 0) ? d : 0u;
            if (i) v[i] += v[i - 1];
        }
        const uint32_t total = v[kLosslessLaneSamples - 1];
        const uint32_t inclusive = wave_inclusive_sum(total, lane);
        if (lane == 63) wave_total[parity][wave] = inclusive;
        __syncthreads();  // the other slot is written next time round: one barrier per chunk
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kLosslessRowThreads / 64; w++) {
            const uint32_t t = wave_total[parity][w];
            if (w < wave) before += t;
            all += t;
        }
        const uint32_t offset = carry + before + inclusive - total;
        carry = (carry + all) & 0xFFFFu;
        if (col >= width) continue;
        uint32_t s[kLosslessLaneSamples];
#pragma unroll
        for (int i = 0; i < kLosslessLaneSamples; i++) s[i] = lossless_sample((offset + v[i]) & 0xFFFFu, pt, out_bytes);
        const uint64_t addr = out_row + (uint64_t)col * out_step;
        const bool whole = col + kLosslessLaneSamples <= width && out_step == out_bytes;
        if (whole && out_bytes == 2 && (addr & 15) == 0) {
            u32x4 o;
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = s[2 * i] | (s[2 * i + 1] << 16);
            *reinterpret_cast<gbl_u32x4*>(addr) = o;
        } else if (whole && out_bytes == 1 && (addr & 7) == 0) {
            u32x2 o;
#pragma unroll
            for (int i = 0; i < 2; i++) o[i] = s[4 * i] | (s[4 * i + 1] << 8) | (s[4 * i + 2] << 16) | (s[4 * i + 3] << 24);
            *reinterpret_cast<gbl_u32x2*>(addr) = o;
        } else {
#pragma unroll
            for (int i = 0; i < kLosslessLaneSamples; i++)
                if (col + i < width) store_sample(addr + (uint64_t)i * out_step, s[i], out_bytes);
        }
    }
}

__global__ __launch_bounds__(64) void lossless_wavefront_kernel(const LosslessPlane* __restrict__ planes)
{
    // two tile slots; row 0 of a slot: the state of the row above the band, rows 1..64: the band's differences, then its state
    __shared__ __attribute__((aligned(16))) uint16_t tile[2][kLosslessBandRows + 1][kLosslessTileCols];
    static_assert(kLosslessBandRows == 64 && kLosslessTileCols == 64, "one lane per row, one lane per column of a tile row");
    const LosslessPlane& p = planes[blockIdx.x];
    const int lane = threadIdx.x;
    const uint32_t width = p.width, height = p.height, pitch = p.diff_pitch, ps = p.ps, pt = p.pt, out_bytes = p.out_bytes;
    const uint32_t out_step = p.out_step, out_pitch = p.out_pitch, restart_rows = p.restart_rows;
    const int init = (int)p.init;
    const gbl_u16* diff = reinterpret_cast<const gbl_u16*>(p.diff);
    gbl_u16* above = reinterpret_cast<gbl_u16*>(p.scratch);
    const uint32_t ntiles = (width + kLosslessTileCols - 1) / kLosslessTileCols;
    for (uint32_t band0 = 0; band0 < height; band0 += kLosslessBandRows) {
        const uint32_t row = band0 + lane;
        const bool live = row < height;
        const bool first_row = live && row % restart_rows == 0;
        const bool carries = band0 + kLosslessBandRows < height;  // another band follows: it needs this band's last row
        int a = 0, b = 0, c = 0;
        for (uint32_t g = 0; g <= ntiles + 1; g++) {
            if (g >= 2) {
                // tile g - 2 is finished in every row: out it goes
                const uint32_t slot = g & 1, col = (g - 2) * kLosslessTileCols + lane;
                if (col < width) {
                    const uint32_t rows = height - band0 < kLosslessBandRows ? height - band0 : kLosslessBandRows;
                    uint64_t addr = p.out + (uint64_t)band0 * out_pitch + (uint64_t)col * out_step;
                    for (uint32_t r = 0; r < rows; r++, addr += out_pitch)
                        store_sample(addr, lossless_sample(tile[slot][r + 1][lane], pt, out_bytes), out_bytes);
                    if (carries) above[col] = tile[slot][kLosslessBandRows][lane];
                }
            }
            wave_lds_fence();
            if (g < ntiles) {
                const uint32_t slot = g & 1, piece = (lane & 7) * 8, col = g * kLosslessTileCols + piece;
                // rows of a difference plane (and the scratch row) are padded to whole 16-byte pieces
#pragma unroll
                for (int pass = 0; pass < kLosslessBandRows / 8; pass++) {
                    const uint32_t r = pass * 8 + (lane >> 3);
                    u32x4 raw = {0u, 0u, 0u, 0u};
                    if (band0 + r < height && col < width) raw = *reinterpret_cast<const gbl_u32x4*>(diff + (size_t)(band0 + r) * pitch + col);
                    *reinterpret_cast<u32x4*>(&tile[slot][r + 1][piece]) = raw;
                }
                if (lane < 8) {
                    u32x4 raw = {0u, 0u, 0u, 0u};
                    if (band0 > 0 && col < width) raw = *reinterpret_cast<const gbl_u32x4*>(above + col);
                    *reinterpret_cast<u32x4*>(&tile[slot][0][piece]) = raw;
                }
            }
            wave_lds_fence();
            if (g > ntiles) continue;
            // (one copy of the steps per predictor: a lone wave is bound by the instructions it issues, and the choice is not one of them)
            switch (ps) {
            case 1: wavefront_steps<1>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            case 2: wavefront_steps<2>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            case 3: wavefront_steps<3>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            case 4: wavefront_steps<4>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            case 5: wavefront_steps<5>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            case 6: wavefront_steps<6>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            default: wavefront_steps<7>(tile, g, lane, (int)width, live, first_row, init, a, b, c); break;
            }
            wave_lds_fence();
        }
        // the next band reads the row this one left in scratch
        __threadfence();
    }
}

hipError_t launch_lossless_rows(const LosslessPlane* planes, int num_planes, int max_height, hipStream_t stream)
{
    for (int at = 0; at < num_planes; at += 65535) {
        const int n = num_planes - at < 65535 ? num_planes - at : 65535;
        hipLaunchKernelGGL(lossless_col0_kernel, dim3((unsigned)n), dim3(64), 0, stream, planes + at);
        hipLaunchKernelGGL(lossless_rows_kernel, dim3((unsigned)max_height, (unsigned)n), dim3(kLosslessRowThreads), 0, stream, planes + at);
    }
    return hipGetLastError();
}

hipError_t launch_lossless_wavefront(const LosslessPlane* planes, int num_planes, hipStream_t stream)
{
    if (num_planes > 0) hipLaunchKernelGGL(lossless_wavefront_kernel, dim3((unsigned)num_planes), dim3(64), 0, stream, planes);
    return hipGetLastError();
}

}  // namespace hipjpeg
