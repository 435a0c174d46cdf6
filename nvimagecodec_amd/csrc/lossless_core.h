// lossless_core.h -- the arithmetic of lossless JPEG reconstruction (T.81 Annex H as libjpeg-turbo's jdlossls.c runs it), shared
// by the reconstruction kernels (lossless_kernels.hip), their schedule run on the host (lossless_core.cpp) and the plain host decoder.
//
// One 16-bit state value per component and position: x = (prediction + difference) & 0xFFFF.  With a = left, b = above,
// c = above-left, all taken from the STATE, in plain int with an arithmetic shift:
//
//     Ps 1: a   2: b   3: c   4: a + b - c   5: a + ((b - c) >> 1)   6: b + ((a - c) >> 1)   7: (a + b) >> 1
//
// The first sample of the picture and of every restart interval is predicted as 1 << (P - Pt - 1); the rest of that row uses a
// whatever Ps says; column 0 of every other row uses b.  A restart interval is a whole number of rows.  The sample that leaves is
// the low 16 bits of x << Pt, or the low 8 bits when P <= 8: no clamp anywhere.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HJ_LL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HJ_LL_HD inline
#endif

namespace hipjpeg {

// ---- the kernels' shape (hipjpegLosslessKernelShape)
constexpr int kLosslessBandRows = 64;        // lossless_wavefront_kernel: rows of a band, one per lane
constexpr int kLosslessTileCols = 64;        // ... and columns of the tiles that travel through the LDS
constexpr int kLosslessLaneSamples = 8;      // lossless_rows_kernel: samples per lane and load (16 bytes)
constexpr int kLosslessRowThreads = 256;     // ... lanes of its workgroup
constexpr int kLosslessChunkSamples = kLosslessRowThreads * kLosslessLaneSamples;  // samples of a row chunk (one carried sum each)
constexpr int kLosslessRowsMinWidth = 64;    // Ps = 1 pictures narrower than this take the wavefront kernel
constexpr int kLosslessPitchSamples = 8;     // rows of a difference plane start on multiples of this (16 bytes)

// One component of one picture, as a kernel sees it.  32- and 64-bit members only (tests/test_code_object_hazards.py).
struct alignas(16) LosslessPlane {
    uint64_t diff;      // uint16 differences, row-major, diff_pitch samples per row, 16-byte aligned
    uint64_t out;       // sample (0, 0) of this component in the caller's buffer
    uint64_t scratch;   // rows kernel: uint16 running sum of the column-0 differences per row; wavefront kernel: uint16 state of the
                        // row above the band (width samples)
    uint32_t width, height;
    uint32_t diff_pitch;    // samples
    uint32_t out_pitch;     // bytes from a row to the next
    uint32_t out_step;      // bytes from a sample to the next of the same component
    uint32_t out_bytes;     // 1 or 2
    uint32_t ps, pt;
    uint32_t init;          // 1 << (P - Pt - 1)
    uint32_t restart_rows;  // rows per restart interval; `height` when the file has none
    uint32_t pad0, pad1;
};
static_assert(sizeof(LosslessPlane) == 80, "descriptor layout");

HJ_LL_HD int lossless_predict(int ps, int a, int b, int c)
{
    switch (ps) {
    case 1: return a;
    case 2: return b;
    case 3: return c;
    case 4: return a + b - c;
    case 5: return a + ((b - c) >> 1);
    case 6: return b + ((a - c) >> 1);
    default: return (a + b) >> 1;
    }
}

// the prediction at (row, col); first_row: the row opens a restart interval (or the picture)
HJ_LL_HD int lossless_predict_at(int ps, bool first_row, uint32_t col, int init, int a, int b, int c)
{
    if (first_row) return col == 0 ? init : a;
    if (col == 0) return b;
    return lossless_predict(ps, a, b, c);
}

HJ_LL_HD uint32_t lossless_state(int prediction, uint32_t difference) { return ((uint32_t)prediction + difference) & 0xFFFFu; }

// the value stored for state x: out_bytes = 1 keeps the low 8 bits (P <= 8), 2 the low 16
HJ_LL_HD uint32_t lossless_sample(uint32_t x, uint32_t pt, uint32_t out_bytes) { return (x << pt) & (out_bytes == 1 ? 0xFFu : 0xFFFFu); }

// rows kernel: the base of row `row` (its column-0 state) from the running column-0 sums S (S[r] = d[0][0] + ... + d[r][0] mod 2^16):
// init + S[row] - S[first row of the interval - 1]
HJ_LL_HD uint32_t lossless_row_base(uint32_t init, uint32_t s_row, uint32_t s_before_interval) { return (init + s_row - s_before_interval) & 0xFFFFu; }

// the planner's choice: true = lossless_col0_kernel + lossless_rows_kernel, false = lossless_wavefront_kernel
HJ_LL_HD bool lossless_takes_rows_kernel(uint32_t ps, uint32_t width) { return ps == 1 && width >= (uint32_t)kLosslessRowsMinWidth; }

HJ_LL_HD uint32_t lossless_diff_pitch(uint32_t width) { return (width + kLosslessPitchSamples - 1) / kLosslessPitchSamples * kLosslessPitchSamples; }

}  // namespace hipjpeg
