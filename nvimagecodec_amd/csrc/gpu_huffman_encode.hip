// gpu_huffman_encode.hip -- gfx950 kernels of the GPU entropy coder (see gpu_huffman_encode.h for the pipeline).
// Arithmetic follows entropy_encode.cpp (the host coder, itself pinned byte-for-byte to libjpeg-turbo's output by the encode
// goldens): jchuff.c encode_one_block for the symbols, jccoefct.c compress_data for the dummy blocks of the MCU padding.
#include <hip/hip_runtime.h>

#include "gpu_huffman_encode.h"
#include "huffman_encode_core.h"
#include "kernel_common.h"

namespace hipjpeg {

namespace {

constexpr int kThreads = 256;

struct LdsTables {
    uint16_t dc_code[2][16];
    uint16_t ac_code[2][256];
    uint8_t dc_size[2][16];
    uint8_t ac_size[2][256];
};
static_assert(sizeof(LdsTables) == sizeof(StandardCodeTables), "same layout as the host struct");

__device__ __forceinline__ void load_tables(LdsTables* dst, const StandardCodeTables* src)
{
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(LdsTables) / 4); i += kThreads) d[i] = s[i];
}

// Word sink of the write kernel's emitter.  The workgroup's 256 blocks cover one contiguous bit range of the image's bit buffer; that
// range is assembled in LDS (zeroed, bits OR-ed in with ds_or -- LDS atomics are cheap) and then copied out as whole words,
// coalesced.  Only the first and the last word of the range can be shared with a neighbouring workgroup: those two go out
// with a global atomic OR (the bit buffer starts out zeroed).  A range that does not fit the window (very high bit rates)
// falls back to OR-ing every word into the global buffer directly.
constexpr int kWindowWords = 4096;  // 16 KB: 256 blocks x 64 bytes on average

struct WindowWords {
    uint32_t* gwords;         // the image's bit buffer
    HJ_LDS uint32_t* window;  // LDS window (LDS address 0 is a valid place for it: never test this pointer)
    bool use_window;          // false: write through to gwords
    uint32_t window_word0;    // index (in gwords) of window[0]
    __device__ __forceinline__ void or_word(uint32_t widx, uint32_t w) const  // w: bits in stream order, most significant first
    {
        if (use_window)
            __hip_atomic_fetch_or(&window[widx - window_word0], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            atomicOr(&gwords[widx], __builtin_bswap32(w));
    }
};
using Emitter = HencEmitter<WindowWords>;

struct LdsCount {
    HJ_LDS uint32_t (*hist)[256];  // [0] DC categories, [1] AC run/size symbols
    __device__ __forceinline__ void add(int dcac, int sym) const
    {
        __hip_atomic_fetch_add(&hist[dcac][sym], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// A block's 64 coefficients as loaded (8 x 16 bytes) -> two per dword
#define HJ_BLOCK_WORDS(q)                                                                                                                            \
    {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w,                   \
     q[4].x, q[4].y, q[4].z, q[4].w, q[5].x, q[5].y, q[5].z, q[5].w, q[6].x, q[6].y, q[6].z, q[6].w, q[7].x, q[7].y, q[7].z, q[7].w}

template <bool WRITE>
__device__ __forceinline__ uint32_t code_block(const uint4 (&q)[8], bool real, int diff, const HJ_LDS LdsTables* T, int ti, Emitter* em)
{
    const uint32_t w[32] = HJ_BLOCK_WORDS(q);
    return henc_code_block<WRITE>(w, real, diff, T, ti, em);
}

// Loads what code_block needs for block s.  RST: the launch has images with restart intervals (huffman_encode_core.h).
template <bool RST>
__device__ __forceinline__ void fetch_block(const HencImage& im, uint32_t s, uint4 (&q)[8], bool* real, int* diff, int* ti)
{
    const HencBlockRef r = henc_locate<RST>(im, s);
    *ti = r.c == 0 ? 0 : 1;
    *real = r.bx < im.real_w[r.c] && r.by < im.real_h[r.c];
    int dc;
    if (*real) {
        const uint4* p = reinterpret_cast<const uint4*>(im.coef[r.c] + ((size_t)r.by * im.blocks_w[r.c] + r.bx) * 64);
#pragma unroll
        for (int i = 0; i < 8; i++) q[i] = p[i];
        dc = (int)(short)(q[0].x & 0xFFFF);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) q[i] = make_uint4(0u, 0u, 0u, 0u);
        dc = henc_dc_value(im, r.c, r.bx, r.by);
    }
    const int pred = r.has_prev ? henc_dc_value(im, r.c, r.pbx, r.pby) : 0;
    *diff = dc - pred;
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void henc_hist_kernel(const HencImage* __restrict__ images, const HencUnit* __restrict__ units)
{
    __shared__ uint32_t hist[2][2][256];
    const HencUnit u = units[blockIdx.x];
    const HencImage& im = images[u.image];
    if (!im.hist) return;  // uniform: this image is coded with the standard tables
    for (int i = threadIdx.x; i < 1024; i += kThreads) (&hist[0][0][0])[i] = 0;
    __syncthreads();
    const uint32_t s = u.first + threadIdx.x;
    if (s < im.total_blocks) {
        uint4 q[8];
        bool real;
        int diff, ti;
        fetch_block<RST>(im, s, q, &real, &diff, &ti);
        const uint32_t w[32] = HJ_BLOCK_WORDS(q);
        henc_count_block(w, real, diff, LdsCount{(HJ_LDS uint32_t(*)[256])hist[ti]});
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += kThreads) {
        const uint32_t v = (&hist[0][0][0])[i];
        if (v) atomicAdd(&im.hist[i], v);
    }
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void henc_length_kernel(const HencImage* __restrict__ images, const HencUnit* __restrict__ units,
                                                               const StandardCodeTables* __restrict__ tables, uint16_t* __restrict__ block_bits)
{
    __shared__ LdsTables T;
    const HencUnit u = units[blockIdx.x];
    const HencImage& im = images[u.image];
    load_tables(&T, im.tables ? im.tables : tables);
    __syncthreads();
    const uint32_t s = u.first + threadIdx.x;
    if (s >= im.total_blocks) return;
    uint4 q[8];
    bool real;
    int diff, ti;
    fetch_block<RST>(im, s, q, &real, &diff, &ti);
    block_bits[im.first_block + s] = (uint16_t)code_block<false>(q, real, diff, (const HJ_LDS LdsTables*)&T, ti, nullptr);
}

// One workgroup per image: block_off = exclusive prefix sum of block_bits; total_bits[image] = the sum.
__global__ __launch_bounds__(kThreads) void henc_scan_kernel(const HencImage* __restrict__ images, const uint16_t* __restrict__ block_bits,
                                                             uint32_t* __restrict__ block_off, uint32_t* __restrict__ total_bits)
{
    __shared__ uint32_t s_sum[kThreads];
    const HencImage& im = images[blockIdx.x];
    const uint16_t* bits = block_bits + im.first_block;
    uint32_t* off = block_off + im.first_block;
    const uint32_t n = im.total_blocks;
    const uint32_t per = (n + kThreads - 1) / kThreads;
    const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    constexpr int kBatch = 8;  // independent loads in flight per lane
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i += kBatch) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) d[k] = i + k < hi ? bits[i + k] : 0u;
#pragma unroll
        for (int k = 0; k < kBatch; k++) sum += d[k];
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const uint32_t v = threadIdx.x >= (unsigned)d ? s_sum[threadIdx.x - d] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? s_sum[threadIdx.x - 1] : 0;
    for (uint32_t i = lo; i < hi; i += kBatch) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) d[k] = i + k < hi ? bits[i + k] : 0u;
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            if (i + k < hi) off[i + k] = run;
            run += d[k];
        }
    }
    if (threadIdx.x == kThreads - 1) total_bits[blockIdx.x] = s_sum[kThreads - 1];
}

// The same for a launch with restart intervals: a segmented scan.  Behind the last block of every interval but the image's last the
// running offset is rounded up to a byte and the marker's 16 bits are added (HencSpan, huffman_encode_core.h); a lane's range and
// the ranges in front of it compose with henc_span_join, which is associative but not commutative: left operand first.
__global__ __launch_bounds__(kThreads) void henc_scan_rst_kernel(const HencImage* __restrict__ images, const uint16_t* __restrict__ block_bits,
                                                                 uint32_t* __restrict__ block_off, uint32_t* __restrict__ total_bits)
{
    __shared__ uint32_t s_a[kThreads], s_b[kThreads], s_cut[kThreads];
    const HencImage& im = images[blockIdx.x];
    const uint16_t* bits = block_bits + im.first_block;
    uint32_t* off = block_off + im.first_block;
    const uint32_t n = im.total_blocks;
    const uint32_t per = (n + kThreads - 1) / kThreads;
    const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    constexpr int kBatch = 8;  // independent loads in flight per lane
    // blocks left in the interval that block lo lies in; the image's last block ends none (henc_ends_interval)
    const uint32_t rst = im.rst_blocks;
    const uint32_t left0 = rst ? rst - lo % rst : 0xFFFFFFFFu;
    HencSpan sp{0u, 0u, 0u};
    uint32_t left = left0;
    for (uint32_t i = lo; i < hi; i += kBatch) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) d[k] = i + k < hi ? bits[i + k] : 0u;
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            if (i + k < hi) {
                const bool ends = --left == 0 && i + k + 1 < n;
                if (left == 0) left = rst;
                sp = henc_span_join(sp, henc_span_block(d[k], ends));
            }
        }
    }
    s_a[threadIdx.x] = sp.a;
    s_b[threadIdx.x] = sp.b;
    s_cut[threadIdx.x] = sp.cut;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const bool has = threadIdx.x >= (unsigned)d;
        HencSpan l{0u, 0u, 0u};
        if (has) l = HencSpan{s_a[threadIdx.x - d], s_b[threadIdx.x - d], s_cut[threadIdx.x - d]};
        __syncthreads();
        if (has) {
            const HencSpan j = henc_span_join(l, HencSpan{s_a[threadIdx.x], s_b[threadIdx.x], s_cut[threadIdx.x]});
            s_a[threadIdx.x] = j.a;
            s_b[threadIdx.x] = j.b;
            s_cut[threadIdx.x] = j.cut;
        }
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? henc_span_apply(0u, HencSpan{s_a[threadIdx.x - 1], s_b[threadIdx.x - 1], s_cut[threadIdx.x - 1]}) : 0;
    left = left0;
    for (uint32_t i = lo; i < hi; i += kBatch) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) d[k] = i + k < hi ? bits[i + k] : 0u;
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            if (i + k < hi) {
                off[i + k] = run;
                const bool ends = --left == 0 && i + k + 1 < n;
                if (left == 0) left = rst;
                run = henc_span_apply(run, henc_span_block(d[k], ends));
            }
        }
    }
    if (threadIdx.x == kThreads - 1) total_bits[blockIdx.x] = henc_span_apply(0u, HencSpan{s_a[kThreads - 1], s_b[kThreads - 1], s_cut[kThreads - 1]});
}

// Zeroes the bit buffers (16 bytes per lane).
__global__ __launch_bounds__(kThreads) void henc_zero_kernel(uint4* __restrict__ p, size_t n16)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void henc_write_kernel(const HencImage* __restrict__ images, const HencUnit* __restrict__ units,
                                                              const StandardCodeTables* __restrict__ tables, const uint32_t* __restrict__ block_off,
                                                              const uint16_t* __restrict__ block_bits)
{
    __shared__ LdsTables T;
    __shared__ uint32_t window[kWindowWords];
    __shared__ uint32_t span[2];  // first word of the workgroup's range, number of words (0: does not fit the window)
    const HencUnit u = units[blockIdx.x];
    const HencImage& im = images[u.image];
    load_tables(&T, im.tables ? im.tables : tables);
    const int t = threadIdx.x;
    const uint32_t s = u.first + t;
    const bool live = s < im.total_blocks;
    if (t == 0) {
        const uint32_t last = min(u.first + kThreads, im.total_blocks) - 1;
        const uint32_t first_bit = block_off[im.first_block + u.first];
        // one past the range's last bit; the image's last block is followed by up to 7 padding bits.  The range must not be
        // overestimated: its last word is the one that may be shared with the next workgroup.
        // With restart intervals: an interval's last block is followed by its padding and the marker, exactly.
        uint32_t end_bit = block_off[im.first_block + last] + block_bits[im.first_block + last] + (last == im.total_blocks - 1 ? 7u : 0u);
        if (henc_ends_interval<RST>(im, last)) end_bit = henc_byte_up(end_bit) + 16u;
        const uint32_t w0 = first_bit >> 5, w1 = (end_bit - 1) >> 5;
        span[0] = w0;
        span[1] = (w1 - w0 + 1 <= (uint32_t)kWindowWords) ? w1 - w0 + 1 : 0u;
    }
    __syncthreads();
    const uint32_t w0 = span[0], nwin = span[1];
    for (uint32_t i = t; i < nwin; i += kThreads) window[i] = 0;
    __syncthreads();
    if (live) {
        uint4 q[8];
        bool real;
        int diff, ti;
        fetch_block<RST>(im, s, q, &real, &diff, &ti);
        const uint32_t off = block_off[im.first_block + s];
        Emitter em;
        em.start(WindowWords{reinterpret_cast<uint32_t*>(im.raw), (HJ_LDS uint32_t*)window, nwin != 0, w0}, off);
        code_block<true>(q, real, diff, (const HJ_LDS LdsTables*)&T, ti, &em);
        // jchuff.c flush_bits: the last byte of the scan -- and of every restart interval -- is filled up with one-bits; RSTn follows
        // an interval and is marked in the bitmap behind the bit buffer
        const uint32_t marker = henc_finish_block<RST>(im, s, off, &em);
        if (RST && marker != ~0u) atomicOr(reinterpret_cast<uint32_t*>(im.raw + henc_map_offset(im.raw_bytes)) + (marker >> 5), 1u << (marker & 31));
        em.finish();
    }
    __syncthreads();
    if (nwin) {
        uint32_t* g = reinterpret_cast<uint32_t*>(im.raw);
        for (uint32_t i = t; i < nwin; i += kThreads) {
            const uint32_t w = __builtin_bswap32(window[i]);
            if (i == 0 || i == nwin - 1) {
                if (w) atomicOr(&g[w0 + i], w);  // may be shared with the neighbouring workgroup
            } else {
                g[w0 + i] = w;
            }
        }
    }
}

// 0x80 in every byte of x that is 0xFF
__device__ __forceinline__ uint32_t ff_mask(uint32_t x)
{
    const uint32_t y = ~x;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}

// valid bytes of this lane's 16-byte piece of chunk `chunk`
__device__ __forceinline__ uint32_t piece_len(const HencImage& im, uint32_t chunk)
{
    const uint32_t off = chunk * kHencChunk + threadIdx.x * 16;
    return off >= im.raw_bytes ? 0u : min(16u, im.raw_bytes - off);
}

// The marker bits of this lane's 16-byte piece of chunk `chunk` (bit i: byte i is a restart marker's FF, not data)
__device__ __forceinline__ uint32_t piece_markers(const HencImage& im, uint32_t chunk)
{
    if (!im.rst_blocks) return 0u;  // an image without restart intervals in a launch that has some: no bitmap behind its buffer
    return reinterpret_cast<const uint16_t*>(im.raw + henc_map_offset(im.raw_bytes))[chunk * (kHencChunk / 16) + threadIdx.x];
}

// 0xFF bytes that need a stuffed 0x00 behind them: all but the markers' (`markers`: piece_markers, 0 without restart intervals)
template <bool RST>
__device__ __forceinline__ uint32_t count_ff(const uint4& v, uint32_t len, uint32_t markers)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t m = ff_mask(w[i]);
        if (RST) m &= ~henc_marker_mask((markers >> (4 * i)) & 15u);
        const int valid = (int)len - 4 * i;  // bytes of this dword that belong to the stream
        if (valid <= 0)
            m = 0;
        else if (valid < 4)
            m &= (1u << (8 * valid)) - 1;
        n += __popc(m);
    }
    return n;
}

__device__ __forceinline__ uint32_t wg_sum(uint32_t v, uint32_t* scratch /*[4]*/)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t total = scratch[0] + scratch[1] + scratch[2] + scratch[3];
    __syncthreads();
    return total;
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void henc_count_kernel(const HencImage* __restrict__ images, const HencUnit* __restrict__ units,
                                                              uint32_t* __restrict__ chunk_ff)
{
    __shared__ uint32_t scratch[4];
    const HencUnit u = units[blockIdx.x];
    const HencImage& im = images[u.image];
    const uint32_t len = piece_len(im, u.first);
    uint32_t n = 0;
    if (len) n = count_ff<RST>(*reinterpret_cast<const uint4*>(im.raw + (size_t)u.first * kHencChunk + threadIdx.x * 16), len, RST ? piece_markers(im, u.first) : 0u);
    const uint32_t total = wg_sum(n, scratch);
    if (threadIdx.x == 0) chunk_ff[im.first_chunk + u.first] = total;
}

// One workgroup in total.  Per segment: chunk_out[c] = 0xFF bytes in the chunks before c; final_len = header + data + stuffed
// zeros (+ EOI behind a file's last segment); final_off = the segments of a file back to back, files at 16-byte boundaries.  A lane
// lays out the files that start in its range of descriptors.
__global__ __launch_bounds__(kThreads) void henc_layout_kernel(const HencImage* __restrict__ images, int nimages, const uint32_t* __restrict__ chunk_ff,
                                                               uint32_t* __restrict__ chunk_out, uint32_t* __restrict__ final_len,
                                                               unsigned long long* __restrict__ final_off)
{
    __shared__ unsigned long long s_sum[kThreads];
    const int per = (nimages + kThreads - 1) / kThreads;
    const int lo = min(nimages, (int)threadIdx.x * per), hi = min(nimages, lo + per);
    unsigned long long sum = 0;
    for (int f = lo; f < hi; f++) {
        uint32_t flen = 0;
        for (int i = f; i < f + (int)images[f].nseg; i++) {
            const HencImage& im = images[i];
            uint32_t ff = 0;
            for (uint32_t c = 0; c < im.num_chunks; c++) {
                chunk_out[im.first_chunk + c] = ff;
                ff += chunk_ff[im.first_chunk + c];
            }
            const uint32_t len = im.header_bytes + im.raw_bytes + ff + (im.last_seg ? 2u : 0u);
            final_len[i] = len;
            flen += len;
        }
        sum += (flen + 15) & ~15u;
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const unsigned long long v = threadIdx.x >= (unsigned)d ? s_sum[threadIdx.x - d] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = threadIdx.x ? s_sum[threadIdx.x - 1] : 0;
    for (int f = lo; f < hi; f++) {
        uint32_t flen = 0;
        for (int i = f; i < f + (int)images[f].nseg; i++) {
            final_off[i] = run + flen;
            flen += final_len[i];
        }
        run += (flen + 15) & ~15u;
    }
}

// Per chunk: bytes with a 0x00 behind every 0xFF that is data, assembled in LDS at the destination's misalignment and copied out as
// dwords (bytes at the ragged ends, which neighbouring chunks share).  Chunk 0 also writes the header, the last chunk EOI.
template <bool RST>
__global__ __launch_bounds__(kThreads) void henc_expand_kernel(const HencImage* __restrict__ images, const HencUnit* __restrict__ units,
                                                               const uint32_t* __restrict__ chunk_out, const uint32_t* __restrict__ final_len,
                                                               const unsigned long long* __restrict__ final_off, uint8_t* __restrict__ arena, int nchunks)
{
    __shared__ uint32_t wave_base[4];
    __shared__ uint32_t out_words[2 * kHencChunk / 4 + 2];
    HJ_LDS uint8_t* out = (HJ_LDS uint8_t*)out_words;
    const int t = threadIdx.x;
    // A few resident workgroups walk the chunk list: with the files going straight to host memory every store waits on PCIe,
    // and one workgroup per chunk would fill every wave slot of the chip with waves that only wait -- starving whatever runs
    // on the other streams (measured: the forward kernel of the next batch stretched from 1.1 to 3.7 ms).
    for (int unit = blockIdx.x; unit < nchunks; unit += gridDim.x) {
    const HencUnit u = units[unit];
    const HencImage& im = images[u.image];
    uint8_t* file = arena + final_off[u.image];
    const uint32_t ff_before = chunk_out[im.first_chunk + u.first];
    const uint32_t dst_off = im.header_bytes + u.first * kHencChunk + ff_before;  // inside the file
    const uint32_t a = (uint32_t)((uintptr_t)(file + dst_off) & 3);

    const uint32_t len = piece_len(im, u.first);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (len) v = *reinterpret_cast<const uint4*>(im.raw + (size_t)u.first * kHencChunk + t * 16);
    const uint32_t markers = RST && len ? piece_markers(im, u.first) : 0u;
    const uint32_t n = len ? count_ff<RST>(v, len, markers) : 0;
    uint32_t incl = n;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(incl, d);
        if ((t & 63) >= d) incl += x;
    }
    if ((t & 63) == 63) wave_base[t >> 6] = incl;
    __syncthreads();
    uint32_t excl = incl - n;
    for (int w = 0; w < (t >> 6); w++) excl += wave_base[w];
    const uint32_t chunk_ffs = wave_base[0] + wave_base[1] + wave_base[2] + wave_base[3];
    if (len) {
        uint32_t o = a + t * 16 + excl;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t i = 0; i < len; i++) {
            const uint8_t b = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            out[o++] = b;
            if (b == 0xFF && !(RST && ((markers >> i) & 1))) out[o++] = 0;
        }
    }
    __syncthreads();
    const uint32_t chunk_len = min((uint32_t)kHencChunk, im.raw_bytes - u.first * kHencChunk);
    const uint32_t n_out = chunk_len + chunk_ffs;
    uint8_t* dst = file + dst_off - a;  // 4-byte aligned
    const uint32_t first_full = a ? 1 : 0, end_full = (a + n_out) / 4;
    for (uint32_t d = first_full + t; d < end_full; d += kThreads) reinterpret_cast<uint32_t*>(dst)[d] = out_words[d];
    if (t < 4) {
        if (a && (uint32_t)t >= a && (uint32_t)t < a + n_out) dst[t] = out[t];  // head
        const uint32_t tail = max(end_full, first_full) * 4 + t;
        if (tail >= a && tail < a + n_out) dst[tail] = out[tail];
    }
    if (u.first == 0)
        for (uint32_t i = t; i < im.header_bytes; i += kThreads) file[i] = im.header[i];
    if (im.last_seg && u.first + 1 == im.num_chunks && t == 0) {
        const uint32_t flen = final_len[u.image];
        file[flen - 2] = 0xFF;
        file[flen - 1] = 0xD9;
    }
    __syncthreads();  // the staging buffer is reused by the next chunk
    }
}

}  // namespace

constexpr int kExpandGrid = 64;  // resident workgroups of the expand kernel: enough stores in flight for PCIe (swept 32..1024 on MI355X)

// `restart`: the launch has images with restart intervals and takes the kernels' flavour that carries the interval arithmetic; without
// it the kernels are the ones a batch without restart intervals has always run.
int launch_henc_hist(const HencImage* images, const HencUnit* units, int nunits, void* stream, bool restart)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(restart ? henc_hist_kernel<true> : henc_hist_kernel<false>, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units);
    return (int)hipGetLastError();
}

int launch_henc_length(const HencImage* images, const HencUnit* units, int nunits, const StandardCodeTables* tables, uint16_t* block_bits, void* stream,
                       bool restart)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(restart ? henc_length_kernel<true> : henc_length_kernel<false>, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units, tables, block_bits);
    return (int)hipGetLastError();
}

int launch_henc_scan(const HencImage* images, int nimages, const uint16_t* block_bits, uint32_t* block_off, uint32_t* total_bits, void* stream,
                     bool restart)
{
    if (nimages <= 0) return 0;
    hipLaunchKernelGGL(restart ? henc_scan_rst_kernel : henc_scan_kernel, dim3(nimages), dim3(kThreads), 0, (hipStream_t)stream, images, block_bits, block_off, total_bits);
    return (int)hipGetLastError();
}

int launch_henc_write(const HencImage* images, const HencUnit* units, int nunits, const StandardCodeTables* tables, const uint32_t* block_off,
                      const uint16_t* block_bits, void* stream, bool restart)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(restart ? henc_write_kernel<true> : henc_write_kernel<false>, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units, tables, block_off, block_bits);
    return (int)hipGetLastError();
}

int launch_henc_zero(void* p, size_t bytes, void* stream)
{
    const size_t n16 = (bytes + 15) / 16;
    if (n16 == 0) return 0;
    hipLaunchKernelGGL(henc_zero_kernel, dim3((unsigned)((n16 + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, static_cast<uint4*>(p), n16);
    return (int)hipGetLastError();
}

int launch_henc_count(const HencImage* images, const HencUnit* chunk_units, int nchunks, uint32_t* chunk_ff, void* stream, bool restart)
{
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(restart ? henc_count_kernel<true> : henc_count_kernel<false>, dim3(nchunks), dim3(kThreads), 0, (hipStream_t)stream, images, chunk_units, chunk_ff);
    return (int)hipGetLastError();
}

int launch_henc_layout(const HencImage* images, int nimages, const uint32_t* chunk_ff, uint32_t* chunk_out, uint32_t* final_len,
                       unsigned long long* final_off, void* stream)
{
    if (nimages <= 0) return 0;
    hipLaunchKernelGGL(henc_layout_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, images, nimages, chunk_ff, chunk_out, final_len, final_off);
    return (int)hipGetLastError();
}

int launch_henc_expand(const HencImage* images, const HencUnit* chunk_units, int nchunks, const uint32_t* chunk_out, const uint32_t* final_len,
                       const unsigned long long* final_off, uint8_t* arena, void* stream, bool restart)
{
    if (nchunks <= 0) return 0;
    const int grid = nchunks < kExpandGrid ? nchunks : kExpandGrid;
    hipLaunchKernelGGL(restart ? henc_expand_kernel<true> : henc_expand_kernel<false>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, images, chunk_units, chunk_out, final_len, final_off,
                       arena, nchunks);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
