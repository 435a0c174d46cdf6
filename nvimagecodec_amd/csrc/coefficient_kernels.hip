// coefficient_kernels.hip -- coef_export_kernel, coef_import_kernel, coef_to_decoder_kernel and coef_from_coder_kernel: quantized
// coefficient blocks between the library's two private HBM layouts and the public one of include/hipjpeg.h
// (hipjpegDecodeCoefficientsBatch / hipjpegEncodeCoefficientsBatch; hipjpegCoefficientsToPixelsBatch / hipjpegPixelsToCoefficientsBatch).
//
//   decoder side (device_layout.h)  int16[64] per block, position col * 8 + row, blocks in raster order over the frame's MCU-padded
//                                   grid; the DC value at dc[b * dc_stride] -- a compact plane for GPU-decoded pictures (position 0
//                                   of the block then holds zero), the block itself for host-decoded ones
//   public (coefficient_kernels.h)  int16[64] per block, position row * 8 + col, raster order over the REAL block area with the
//                                   caller's pitch
//   coder side (encode_layout.h)    int16[64] per block in zigzag order, raster order over the coder's own MCU-padded grid; only the
//                                   real_w x real_h blocks that carry samples are defined
//
// Both are bandwidth kernels of coef_relayout_kernel's build (transcode_kernels.hip): eight lanes per block, one 16-byte load per lane,
// the block parked in a 144-byte LDS slot of the lanes' own wave, a gather with loop-invariant offsets, one 16-byte store per lane; four
// passes travel together, so that four loads and then four stores per lane are in flight; 256 real blocks per workgroup; no branch
// around the loads (lanes past the end read the component's last real block again and store nothing).
//
// Export: lane j loads column j of the decoder's block and stores natural row j -- an 8 x 8 int16 transpose through the slot: row j is
// the halves at byte j * 2 of the eight parked columns, 16 bytes apart.
// Import: lane j loads natural row j and stores 16-byte piece j of the zigzag-ordered block.  A natural row-major block is the decoder's
// block transposed, so the gather offsets are those coef_transform_kernel uses for a transposing turn: zigzag[k] * 2.  The range guard of
// the transcode kernels runs in the same pass: the DC value is the low half of the first dword of row 0 here as it is of column 0 there.
// To the decoder: export's transpose in the other direction (a transpose is its own inverse: the same gather), over the MCU-padded grid
// of the destination, whose blocks then lie back to back; blocks outside the real area are stored as zeros (their lanes load the nearest
// real block, no branch, and drop it).  From the coder: lane j loads piece j of the zigzag-ordered block and stores natural row j, the
// gather offsets being the inverse of import's: position-in-zigzag[natural index] * 2.
#include <hip/hip_runtime.h>

#include "coefficient_kernels.h"
#include "kernel_common.h"

namespace hipjpeg {

namespace {
constexpr int kThreads = 256;
constexpr int kBlocksPerPass = kThreads / 8;
constexpr int kPasses = kRelayoutBlocksPerUnit / kBlocksPerPass;
constexpr int kDepth = 4;  // passes that travel together: their loads are in flight at the same time, then their stores
constexpr int kRounds = kPasses / kDepth;
constexpr int kSlotStride = 144;  // 128 B block + 16 B pad: the 16-byte writes of a wave's eight blocks start on different banks
static_assert(kPasses % kDepth == 0, "whole rounds");

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// byte offsets (inside a row-major int16 block) of the eight coefficients that make up 16-byte piece `piece` of the zigzag-ordered
// block, two per dword
struct PieceOffsets {
    unsigned w[8][4];
};
constexpr PieceOffsets make_piece_offsets_natural()
{
    PieceOffsets t{};
    for (int piece = 0; piece < 8; piece++)
        for (int i = 0; i < 8; i++) {
            const unsigned off = (unsigned)(kZigzag[piece * 8 + i] * 2);
            t.w[piece][i >> 1] |= (i & 1) ? off << 16 : off;
        }
    return t;
}
__device__ const PieceOffsets kPieceOffsetsNatural = make_piece_offsets_natural();
// the inverse: byte offsets (inside a zigzag-ordered int16 block) of the eight coefficients of natural row `piece`
constexpr PieceOffsets make_row_offsets_zigzag()
{
    PieceOffsets t{};
    int where[64] = {};
    for (int k = 0; k < 64; k++) where[kZigzag[k]] = k;
    for (int row = 0; row < 8; row++)
        for (int i = 0; i < 8; i++) {
            const unsigned off = (unsigned)(where[row * 8 + i] * 2);
            t.w[row][i >> 1] |= (i & 1) ? off << 16 : off;
        }
    return t;
}
__device__ const PieceOffsets kRowOffsetsZigzag = make_row_offsets_zigzag();

struct Fetched {
    u32x4 v;
    int dc;
    unsigned by, bx;
    bool live;  // (the same for the eight lanes of a block)
};
}  // namespace

__global__ __launch_bounds__(kThreads) void coef_export_kernel(const DecodeImage* __restrict__ src, const CoefPlane* __restrict__ planes,
                                                              const RelayoutUnit* __restrict__ units)
{
    __shared__ __attribute__((aligned(16))) char slots[kDepth * kBlocksPerPass * kSlotStride];
    const RelayoutUnit u = units[blockIdx.x];
    const DecodeComponent& sc = src[u.image].comp[u.comp];  // comp 0..3 (uniform): one aligned record, members at constant offsets
    const CoefPlane& dp = planes[u.image * 4u + u.comp];    // the same
    const unsigned real_w = dp.real_w, nreal = dp.real_w * dp.real_h, dst_w = dp.pitch;
    gbl_i16* out = (gbl_i16*)dp.coef;
    const unsigned src_w = sc.blocks_w;
    const gbl_i16* in = (const gbl_i16*)sc.coef;
    const gbl_i16* dcs = (const gbl_i16*)sc.dc;
    const unsigned dc_stride = sc.dc_stride;

    const unsigned piece = threadIdx.x & 7u, slot_index = threadIdx.x >> 3;
    lds_char* slot = (lds_char*)slots + slot_index * kSlotStride;
    // all eight lanes of a block read its DC value, one address
    auto fetch = [&](int pass) {
        Fetched f;
        const unsigned r = u.first_block + (unsigned)pass * kBlocksPerPass + slot_index;
        f.live = r < nreal;
        const unsigned rr = f.live ? r : nreal - 1u;
        f.by = rr / real_w;
        f.bx = rr - f.by * real_w;
        const size_t sb = (size_t)f.by * src_w + f.bx;
        f.v = *reinterpret_cast<const gbl_u32x4*>(in + sb * 64 + piece * 8);
        f.dc = dcs[sb * dc_stride];  // column 0 starts with the DC value: wherever the decoder keeps it
        return f;
    };
    for (int round = 0; round < kRounds; round++) {
        Fetched f[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++) f[j] = fetch(round * kDepth + j);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            // (lanes that are not live carry a real block a second time: parking it again does no harm)
            u32x4 v = f[j].v;
            if (piece == 0) v.x = (v.x & 0xFFFF0000u) | ((unsigned)f[j].dc & 0xFFFFu);
            *reinterpret_cast<lds_u32x4*>(slot + j * (kBlocksPerPass * kSlotStride) + piece * 16) = v;
        }
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (!f[j].live) continue;
            // natural row `piece`: element t is row `piece` of column t
            const lds_char* mine = slot + j * (kBlocksPerPass * kSlotStride) + piece * 2;
            unsigned h[8];
#pragma unroll
            for (int t = 0; t < 8; t++) h[t] = *reinterpret_cast<const lds_u16*>(mine + t * 16);
            const u32x4 z = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            *reinterpret_cast<gbl_u32x4*>(out + ((size_t)f[j].by * dst_w + f[j].bx) * 64 + piece * 8) = z;
        }
        wave_lds_fence();  // the next round rewrites the slots
    }
}

__global__ __launch_bounds__(kThreads) void coef_import_kernel(const CoefPlane* __restrict__ planes, const EncodeImage* __restrict__ dst,
                                                              const RelayoutUnit* __restrict__ units, uint32_t* __restrict__ out_of_range)
{
    __shared__ __attribute__((aligned(16))) char slots[kDepth * kBlocksPerPass * kSlotStride];
    const RelayoutUnit u = units[blockIdx.x];
    const int c = (int)u.comp;  // 0, 1, 2 (uniform)
    const CoefPlane& sp = planes[u.image * 4u + u.comp];
    const EncodeImage& im = dst[u.image];
    const unsigned real_w = sp.real_w, nreal = sp.real_w * sp.real_h, src_w = sp.pitch;
    const unsigned dst_w = c == 0 ? im.blocks_w[0] : c == 1 ? im.blocks_w[1] : im.blocks_w[2];
    gbl_i16* out = (gbl_i16*)(c == 0 ? im.coef[0] : c == 1 ? im.coef[1] : im.coef[2]);
    const gbl_i16* in = (const gbl_i16*)sp.coef;

    const unsigned piece = threadIdx.x & 7u, slot_index = threadIdx.x >> 3;
    lds_char* slot = (lds_char*)slots + slot_index * kSlotStride;
    const uint4 zoff = *reinterpret_cast<const uint4*>(&kPieceOffsetsNatural.w[piece][0]);
    const unsigned o[4] = {zoff.x, zoff.y, zoff.z, zoff.w};
    auto fetch = [&](int pass) {
        Fetched f;
        const unsigned r = u.first_block + (unsigned)pass * kBlocksPerPass + slot_index;
        f.live = r < nreal;
        const unsigned rr = f.live ? r : nreal - 1u;
        f.by = rr / real_w;
        f.bx = rr - f.by * real_w;
        f.v = *reinterpret_cast<const gbl_u32x4*>(in + ((size_t)f.by * src_w + f.bx) * 64 + piece * 8);
        f.dc = 0;
        return f;
    };
    unsigned bad = 0;
    for (int round = 0; round < kRounds; round++) {
        Fetched f[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++) f[j] = fetch(round * kDepth + j);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            // (lanes that are not live carry a real block a second time: checking and parking it again does no harm)
            const u32x4 v = f[j].v;
            const bool first = piece == 0;
            // the DC value may be -1024; it is the low half of row 0's first dword
            const int low = (int)(short)(v.x & 0xFFFFu);
            bad |= pair_outside(first ? (v.x & 0xFFFF0000u) : v.x) | (unsigned)(first & ((low < -1024) | (low > 1023)));
            bad |= pair_outside(v.y) | pair_outside(v.z) | pair_outside(v.w);
            *reinterpret_cast<lds_u32x4*>(slot + j * (kBlocksPerPass * kSlotStride) + piece * 16) = v;
        }
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (!f[j].live) continue;
            const lds_char* mine = slot + j * (kBlocksPerPass * kSlotStride);
            unsigned h[8];
#pragma unroll
            for (int t = 0; t < 8; t++) h[t] = *reinterpret_cast<const lds_u16*>(mine + ((t & 1) ? (o[t >> 1] >> 16) : (o[t >> 1] & 0xFFFFu)));
            const u32x4 z = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            *reinterpret_cast<gbl_u32x4*>(out + ((size_t)f[j].by * dst_w + f[j].bx) * 64 + piece * 8) = z;
        }
        wave_lds_fence();  // the next round rewrites the slots
    }
    // one flag word per image, at most one atomic per wave
    if (__ballot(bad != 0u) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&out_of_range[u.image], 1u);
}

__global__ __launch_bounds__(kThreads) void coef_to_decoder_kernel(const CoefPlane* __restrict__ planes, const DecodeImage* __restrict__ dst,
                                                                  const RelayoutUnit* __restrict__ units)
{
    __shared__ __attribute__((aligned(16))) char slots[kDepth * kBlocksPerPass * kSlotStride];
    const RelayoutUnit u = units[blockIdx.x];
    const CoefPlane& sp = planes[u.image * 4u + u.comp];     // comp 0..3 (uniform): one aligned record, members at constant offsets
    const DecodeComponent& dc = dst[u.image].comp[u.comp];  // the same
    const unsigned real_w = sp.real_w, real_h = sp.real_h, src_w = sp.pitch;
    const unsigned grid_w = dc.blocks_w, ngrid = (unsigned)dc.blocks_w * dc.blocks_h;
    const gbl_i16* in = (const gbl_i16*)sp.coef;
    gbl_i16* out = (gbl_i16*)dc.coef;

    const unsigned piece = threadIdx.x & 7u, slot_index = threadIdx.x >> 3;
    lds_char* slot = (lds_char*)slots + slot_index * kSlotStride;
    // f.by, f.bx: the block's place in the padded grid; f.dc: 1 = it carries samples (the same for the eight lanes of a block)
    auto fetch = [&](int pass) {
        Fetched f;
        const unsigned r = u.first_block + (unsigned)pass * kBlocksPerPass + slot_index;
        f.live = r < ngrid;
        const unsigned rr = f.live ? r : ngrid - 1u;
        f.by = rr / grid_w;
        f.bx = rr - f.by * grid_w;
        f.dc = (int)((f.by < real_h) & (f.bx < real_w));
        // (padding reads the nearest real block: an address that is always the component's own)
        const unsigned sy = f.by < real_h ? f.by : real_h - 1u, sx = f.bx < real_w ? f.bx : real_w - 1u;
        f.v = *reinterpret_cast<const gbl_u32x4*>(in + ((size_t)sy * src_w + sx) * 64 + piece * 8);
        return f;
    };
    for (int round = 0; round < kRounds; round++) {
        Fetched f[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++) f[j] = fetch(round * kDepth + j);
#pragma unroll
        for (int j = 0; j < kDepth; j++) *reinterpret_cast<lds_u32x4*>(slot + j * (kBlocksPerPass * kSlotStride) + piece * 16) = f[j].v;
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (!f[j].live) continue;
            // the decoder's column `piece`: element t is column `piece` of natural row t
            const lds_char* mine = slot + j * (kBlocksPerPass * kSlotStride) + piece * 2;
            unsigned h[8];
#pragma unroll
            for (int t = 0; t < 8; t++) h[t] = *reinterpret_cast<const lds_u16*>(mine + t * 16);
            const unsigned keep = f[j].dc ? 0xFFFFFFFFu : 0u;  // padding of the grid: zeros
            const u32x4 z = {(h[0] | (h[1] << 16)) & keep, (h[2] | (h[3] << 16)) & keep, (h[4] | (h[5] << 16)) & keep, (h[6] | (h[7] << 16)) & keep};
            *reinterpret_cast<gbl_u32x4*>(out + ((size_t)f[j].by * grid_w + f[j].bx) * 64 + piece * 8) = z;
        }
        wave_lds_fence();  // the next round rewrites the slots
    }
}

__global__ __launch_bounds__(kThreads) void coef_from_coder_kernel(const EncodeImage* __restrict__ src, const CoefPlane* __restrict__ planes,
                                                                  const RelayoutUnit* __restrict__ units)
{
    __shared__ __attribute__((aligned(16))) char slots[kDepth * kBlocksPerPass * kSlotStride];
    const RelayoutUnit u = units[blockIdx.x];
    const int c = (int)u.comp;  // 0, 1, 2 (uniform)
    const CoefPlane& dp = planes[u.image * 4u + u.comp];
    const EncodeImage& im = src[u.image];
    const unsigned real_w = dp.real_w, nreal = dp.real_w * dp.real_h, dst_w = dp.pitch;
    const unsigned src_w = c == 0 ? im.blocks_w[0] : c == 1 ? im.blocks_w[1] : im.blocks_w[2];
    const gbl_i16* in = (const gbl_i16*)(c == 0 ? im.coef[0] : c == 1 ? im.coef[1] : im.coef[2]);
    gbl_i16* out = (gbl_i16*)dp.coef;

    const unsigned piece = threadIdx.x & 7u, slot_index = threadIdx.x >> 3;
    lds_char* slot = (lds_char*)slots + slot_index * kSlotStride;
    const uint4 zoff = *reinterpret_cast<const uint4*>(&kRowOffsetsZigzag.w[piece][0]);
    const unsigned o[4] = {zoff.x, zoff.y, zoff.z, zoff.w};
    auto fetch = [&](int pass) {
        Fetched f;
        const unsigned r = u.first_block + (unsigned)pass * kBlocksPerPass + slot_index;
        f.live = r < nreal;
        const unsigned rr = f.live ? r : nreal - 1u;
        f.by = rr / real_w;
        f.bx = rr - f.by * real_w;
        f.v = *reinterpret_cast<const gbl_u32x4*>(in + ((size_t)f.by * src_w + f.bx) * 64 + piece * 8);
        f.dc = 0;
        return f;
    };
    for (int round = 0; round < kRounds; round++) {
        Fetched f[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++) f[j] = fetch(round * kDepth + j);
#pragma unroll
        for (int j = 0; j < kDepth; j++) *reinterpret_cast<lds_u32x4*>(slot + j * (kBlocksPerPass * kSlotStride) + piece * 16) = f[j].v;
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (!f[j].live) continue;
            const lds_char* mine = slot + j * (kBlocksPerPass * kSlotStride);
            unsigned h[8];
#pragma unroll
            for (int t = 0; t < 8; t++) h[t] = *reinterpret_cast<const lds_u16*>(mine + ((t & 1) ? (o[t >> 1] >> 16) : (o[t >> 1] & 0xFFFFu)));
            const u32x4 z = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            *reinterpret_cast<gbl_u32x4*>(out + ((size_t)f[j].by * dst_w + f[j].bx) * 64 + piece * 8) = z;
        }
        wave_lds_fence();  // the next round rewrites the slots
    }
}

int launch_coef_export(const DecodeImage* src, const CoefPlane* planes, const RelayoutUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(coef_export_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, src, planes, units);
    return (int)hipGetLastError();
}

int launch_coef_import(const CoefPlane* planes, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(coef_import_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, planes, dst, units, out_of_range);
    return (int)hipGetLastError();
}

int launch_coef_to_decoder(const CoefPlane* planes, const DecodeImage* dst, const RelayoutUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(coef_to_decoder_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, planes, dst, units);
    return (int)hipGetLastError();
}

int launch_coef_from_coder(const EncodeImage* src, const CoefPlane* planes, const RelayoutUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(coef_from_coder_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, src, planes, units);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
