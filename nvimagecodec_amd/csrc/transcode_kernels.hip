// transcode_kernels.hip -- coef_relayout_kernel and coef_transform_kernel: quantized coefficient blocks from the entropy decoder's HBM layout to the entropy
// coder's, the one device step of a lossless transcode (hipjpegTranscodeBatch).
//
//   decoder side (device_layout.h)  int16[64] per block, position col * 8 + row, blocks in raster order over the frame's MCU-padded
//                                   grid; the DC value at dc[b * dc_stride] -- a compact plane for GPU-decoded pictures (position 0
//                                   of the block then holds zero), the block itself for host-decoded ones
//   coder side (encode_layout.h)    int16[64] per block in zigzag order, raster order over the coder's own MCU-padded grid; only the
//                                   real_w x real_h blocks that carry samples are defined
//
// Eight lanes per block.  Lane j loads column j of the block (one 16-byte chunk), the block is parked in an LDS slot of the lanes'
// wave (four blocks per lane group at a time, so that four loads and then four stores per lane are in flight), lane j gathers the eight positions that make up 16-byte piece j of the zigzag-ordered block -- always the same eight, so the
// LDS offsets are loop invariants -- and stores 16 bytes: a wave reads and writes whole 128-byte lines, eight blocks at a time.  The
// slots are 144 bytes apart (128 B block + 16 B pad), as in forward_pair_kernel's copy-out: the 16-byte column writes of a wave's
// eight blocks then start on different banks.
//
// The range guard of the transcode runs in the same pass: every lane compares the values it carries with jchuff.c's limits for 8-bit
// data, one ballot per wave at the end, at most one atomicOr per wave into the image's flag word.
//
// coef_transform_kernel is the same pass for pictures that are turned on the way (transcode_core.h: transpose, mirror x, mirror y of the
// OUTPUT, RelayoutUnit::pad, uniform per workgroup).  It walks the output's real blocks in raster order, so the stores fill whole lines as
// before, and computes the source block of each; every source block is still one aligned 128-byte read.  The block's own transpose costs
// nothing: the decoder's block is column-major, so gathering with row-major offsets (a second offsets table) IS the transpose.  A mirror
// negates the coefficients of odd horizontal / vertical frequency: per piece an 8-bit mask, applied while the halves are packed.
// A picture cropped at an origin other than (0, 0) takes this kernel too, turned or not (turn 0 is the plain copy): the origin of the
// unit's component rides behind the turn in RelayoutUnit::pad.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "transcode_kernels.h"

namespace hipjpeg {

namespace {
constexpr int kThreads = 256;
constexpr int kBlocksPerPass = kThreads / 8;
constexpr int kPasses = kRelayoutBlocksPerUnit / kBlocksPerPass;
constexpr int kDepth = 4;  // passes that travel together: their loads are in flight at the same time, then their stores
constexpr int kRounds = kPasses / kDepth;
constexpr int kSlotStride = 144;
static_assert(kPasses % kDepth == 0, "whole rounds");

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// byte offsets (inside a column-major int16 block) of the eight coefficients that make up 16-byte piece `piece` of the zigzag-ordered
// block, two per dword
struct PieceOffsets {
    unsigned w[8][4];
};
constexpr PieceOffsets make_piece_offsets()
{
    PieceOffsets t{};
    for (int piece = 0; piece < 8; piece++)
        for (int i = 0; i < 8; i++) {
            const int nat = kZigzag[piece * 8 + i];
            const unsigned off = (unsigned)(((nat & 7) * 8 + (nat >> 3)) * 2);
            t.w[piece][i >> 1] |= (i & 1) ? off << 16 : off;
        }
    return t;
}
__device__ const PieceOffsets kPieceOffsets = make_piece_offsets();

// the same for a block that is to come out transposed: natural position v * 8 + u of the output is position v * 8 + u of the
// decoder's memory (column v, row u: the source's coefficient (u, v))
constexpr PieceOffsets make_piece_offsets_transposed()
{
    PieceOffsets t{};
    for (int piece = 0; piece < 8; piece++)
        for (int i = 0; i < 8; i++) {
            const unsigned off = (unsigned)(kZigzag[piece * 8 + i] * 2);
            t.w[piece][i >> 1] |= (i & 1) ? off << 16 : off;
        }
    return t;
}
__device__ const PieceOffsets kPieceOffsetsTransposed = make_piece_offsets_transposed();

// per piece: bit i set when coefficient i of the piece has odd horizontal (odd_u) / vertical (odd_v) frequency in the output block
struct PieceMasks {
    unsigned odd_u[8], odd_v[8];
};
constexpr PieceMasks make_piece_masks()
{
    PieceMasks t{};
    for (int piece = 0; piece < 8; piece++)
        for (int i = 0; i < 8; i++) {
            const int nat = kZigzag[piece * 8 + i];
            t.odd_u[piece] |= (unsigned)(nat & 1) << i;
            t.odd_v[piece] |= (unsigned)((nat >> 3) & 1) << i;
        }
    return t;
}
__device__ const PieceMasks kPieceMasks = make_piece_masks();

}  // namespace

__global__ __launch_bounds__(kThreads) void coef_relayout_kernel(const DecodeImage* __restrict__ src, const EncodeImage* __restrict__ dst,
                                                                const RelayoutUnit* __restrict__ units, uint32_t* __restrict__ out_of_range)
{
    __shared__ __attribute__((aligned(16))) char slots[kDepth * kBlocksPerPass * kSlotStride];
    const RelayoutUnit u = units[blockIdx.x];
    const int c = (int)u.comp;  // 0, 1, 2 (uniform)
    const DecodeComponent& sc = src[u.image].comp[c];
    const EncodeImage& im = dst[u.image];
    const unsigned real_w = c == 0 ? im.real_w[0] : c == 1 ? im.real_w[1] : im.real_w[2];
    const unsigned real_h = c == 0 ? im.real_h[0] : c == 1 ? im.real_h[1] : im.real_h[2];
    const unsigned dst_w = c == 0 ? im.blocks_w[0] : c == 1 ? im.blocks_w[1] : im.blocks_w[2];
    gbl_i16* out = (gbl_i16*)(c == 0 ? im.coef[0] : c == 1 ? im.coef[1] : im.coef[2]);
    const unsigned src_w = sc.blocks_w, nreal = real_w * real_h;
    const gbl_i16* in = (const gbl_i16*)sc.coef;
    const gbl_i16* dcs = (const gbl_i16*)sc.dc;
    const unsigned dc_stride = sc.dc_stride;

    const unsigned piece = threadIdx.x & 7u, slot_index = threadIdx.x >> 3;
    lds_char* slot = (lds_char*)slots + slot_index * kSlotStride;
    const uint4 zoff = *reinterpret_cast<const uint4*>(&kPieceOffsets.w[piece][0]);
    const unsigned o[4] = {zoff.x, zoff.y, zoff.z, zoff.w};
    // One pass = 32 blocks, one round = kDepth passes: a wave has kDepth 16-byte loads per lane in flight, parks the blocks in kDepth
    // slots per block position, gathers them and has kDepth 16-byte stores in flight -- 4 KB per wave each way, which is what keeps
    // HBM busy from the seven waves per SIMD the registers allow.
    struct Fetched {
        u32x4 v;
        int dc;
        unsigned by, bx;
        bool live;  // (the same for the eight lanes of a block)
    };
    // No branch around the loads (the compiler would wait for each at the end of its branch): lanes past the unit's last block read
    // the component's last real block again and store nothing; all eight lanes of a block read its DC value, one address.
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
    unsigned bad = 0;
    for (int round = 0; round < kRounds; round++) {
        Fetched f[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++) f[j] = fetch(round * kDepth + j);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            // (lanes that are not live carry a real block a second time: checking and parking it again does no harm)
            u32x4 v = f[j].v;
            const bool first = piece == 0;
            if (first) v.x = (v.x & 0xFFFF0000u) | ((unsigned)f[j].dc & 0xFFFFu);
            // the DC value may be -1024; it is the low half of column 0's first dword
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

// The turned sibling of coef_relayout_kernel (same slots, same rounds, same guard; see the head of the file).
__global__ __launch_bounds__(kThreads) void coef_transform_kernel(const DecodeImage* __restrict__ src, const EncodeImage* __restrict__ dst,
                                                                 const RelayoutUnit* __restrict__ units, uint32_t* __restrict__ out_of_range)
{
    __shared__ __attribute__((aligned(16))) char slots[kDepth * kBlocksPerPass * kSlotStride];
    const RelayoutUnit u = units[blockIdx.x];
    const int c = (int)u.comp;  // 0, 1, 2 (uniform)
    const DecodeComponent& sc = src[u.image].comp[c];
    const EncodeImage& im = dst[u.image];
    const unsigned real_w = c == 0 ? im.real_w[0] : c == 1 ? im.real_w[1] : im.real_w[2];
    const unsigned real_h = c == 0 ? im.real_h[0] : c == 1 ? im.real_h[1] : im.real_h[2];
    const unsigned dst_w = c == 0 ? im.blocks_w[0] : c == 1 ? im.blocks_w[1] : im.blocks_w[2];
    gbl_i16* out = (gbl_i16*)(c == 0 ? im.coef[0] : c == 1 ? im.coef[1] : im.coef[2]);
    const unsigned src_w = sc.blocks_w, nreal = real_w * real_h;
    const unsigned dc_stride = sc.dc_stride;
    // the turn (uniform): bit 0 transpose, bit 1 mirror x, bit 2 mirror y of the output
    const bool transpose = (u.pad & 1u) != 0u, mirror_x = (u.pad & 2u) != 0u, mirror_y = (u.pad & 4u) != 0u;
    // the crop (uniform): block (oy, ox) of the decoder's grid is where this component of the picture begins.  The origin is added after
    // the mirrors and the transpose are undone, i.e. to every source block alike: it moves the two base pointers, once per workgroup on
    // the scalar unit, and the per-block address arithmetic stays what it is for an uncropped picture.
    const unsigned ox = (u.pad >> kOriginShiftX) & kOriginMask, oy = (u.pad >> kOriginShiftY) & kOriginMask;
    const size_t first = (size_t)oy * src_w + ox;
    const gbl_i16* in = (const gbl_i16*)sc.coef + first * 64;
    const gbl_i16* dcs = (const gbl_i16*)sc.dc + first * dc_stride;

    const unsigned piece = threadIdx.x & 7u, slot_index = threadIdx.x >> 3;
    lds_char* slot = (lds_char*)slots + slot_index * kSlotStride;
    const PieceOffsets& table = transpose ? kPieceOffsetsTransposed : kPieceOffsets;
    const uint4 zoff = *reinterpret_cast<const uint4*>(&table.w[piece][0]);
    const unsigned o[4] = {zoff.x, zoff.y, zoff.z, zoff.w};
    // negated twice is not negated: the masks of the two mirrors combine by xor
    const unsigned negate = (mirror_x ? kPieceMasks.odd_u[piece] : 0u) ^ (mirror_y ? kPieceMasks.odd_v[piece] : 0u);
    struct Fetched {
        u32x4 v;
        int dc;
        unsigned by, bx;  // of the output
        bool live;        // (the same for the eight lanes of a block)
    };
    // As in coef_relayout_kernel no branch surrounds the loads; lanes past the unit's last block read the source of the component's
    // last output block again.  The source block: undo the output's mirrors over its real area, then the transpose -- the real area
    // of the (cropped, trimmed) source is the output's with the axes swapped, and transcode_crop keeps origin + real area inside the
    // source's own real area, so every index stays inside the decoder's grid.
    auto fetch = [&](int pass) {
        Fetched f;
        const unsigned r = u.first_block + (unsigned)pass * kBlocksPerPass + slot_index;
        f.live = r < nreal;
        const unsigned rr = f.live ? r : nreal - 1u;
        f.by = rr / real_w;
        f.bx = rr - f.by * real_w;
        const unsigned ty = mirror_y ? real_h - 1u - f.by : f.by, tx = mirror_x ? real_w - 1u - f.bx : f.bx;
        const size_t sb = transpose ? (size_t)tx * src_w + ty : (size_t)ty * src_w + tx;
        f.v = *reinterpret_cast<const gbl_u32x4*>(in + sb * 64 + piece * 8);
        f.dc = dcs[sb * dc_stride];
        return f;
    };
    unsigned bad = 0;
    for (int round = 0; round < kRounds; round++) {
        Fetched f[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++) f[j] = fetch(round * kDepth + j);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            u32x4 v = f[j].v;
            const bool first = piece == 0;
            if (first) v.x = (v.x & 0xFFFF0000u) | ((unsigned)f[j].dc & 0xFFFFu);
            // the guard looks at the source's values (the limits of the AC values are symmetric, the DC value is never negated)
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
            for (int t = 0; t < 8; t++) {
                const unsigned x = *reinterpret_cast<const lds_u16*>(mine + ((t & 1) ? (o[t >> 1] >> 16) : (o[t >> 1] & 0xFFFFu)));
                const unsigned sign = 0u - ((negate >> t) & 1u);  // all ones: two's complement negation of the half, no branch
                h[t] = ((x ^ sign) - sign) & 0xFFFFu;
            }
            const u32x4 z = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            *reinterpret_cast<gbl_u32x4*>(out + ((size_t)f[j].by * dst_w + f[j].bx) * 64 + piece * 8) = z;
        }
        wave_lds_fence();  // the next round rewrites the slots
    }
    if (__ballot(bad != 0u) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&out_of_range[u.image], 1u);
}

int launch_coef_relayout(const DecodeImage* src, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(coef_relayout_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, src, dst, units, out_of_range);
    return (int)hipGetLastError();
}

int launch_coef_transform(const DecodeImage* src, const EncodeImage* dst, const RelayoutUnit* units, int nunits, uint32_t* out_of_range, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(coef_transform_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, src, dst, units, out_of_range);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
