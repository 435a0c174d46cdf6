// lossless_encode_kernels.hip -- gfx950 kernels of the lossless (SOF3) coder; the pipeline is described in lossless_encode_kernels.h,
// the per-sample routines and the shape are lossless_encode_core.h's, which the host twin (lossless_encode_host.cpp) runs too.
// The differences are not stored between the passes: each pass computes them again from the input.  A 2-byte difference plane costs
// as much to read as the 2-byte input, and not writing it saves one pass over the picture's bytes.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "lossless_encode_kernels.h"

namespace hipjpeg {

namespace {

constexpr int kThreads = kLencThreads;
constexpr int kStatCopies = 64;  // copies of each counter in LDS, one per lane of a wave: the lanes of one ds_add never share an address
constexpr int kStatGrid = 128;   // workgroups per picture that stride over its pieces

struct LdsCounters {
    HJ_LDS uint32_t* slots;  // [kLencSymbols][kStatCopies], this lane's column
    __device__ __forceinline__ void add(uint32_t ssss) const
    {
        __hip_atomic_fetch_add(&slots[ssss * kStatCopies], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// grid (x: picture, y: kStatGrid workgroups that stride over its pieces; grid y ends at 65535, so the pictures are x)
__global__ __launch_bounds__(kThreads) void lenc_stats_kernel(const LencImage* __restrict__ images)
{
    __shared__ uint32_t counters[kLencSymbols * kStatCopies];
    const LencImage& im = images[blockIdx.x];
    const uint32_t first = blockIdx.y;
    const uint32_t npieces = lenc_pieces(im);
    if (first >= npieces) return;  // uniform
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < (uint32_t)(kLencSymbols * kStatCopies); i += kThreads) counters[i] = 0;
    __syncthreads();
    const LdsCounters count{(HJ_LDS uint32_t*)counters + (t & (kStatCopies - 1))};
    for (uint32_t piece = first; piece < npieces; piece += kStatGrid) lenc_stat_lane(im, piece, t, count);
    __syncthreads();
    if (t < (uint32_t)kLencSymbols) {
        uint32_t sum = 0;
        for (int k = 0; k < kStatCopies; k++) sum += counters[t * kStatCopies + ((k + t) & (kStatCopies - 1))];
        if (sum) atomicAdd(reinterpret_cast<uint32_t*>(im.counts) + t, sum);
    }
}

__device__ __forceinline__ void load_codes(uint32_t* lds, const LencImage& im)
{
    if (threadIdx.x < (unsigned)kLencSymbols) lds[threadIdx.x] = reinterpret_cast<const uint32_t*>(im.codes)[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void lenc_length_kernel(const LencImage* __restrict__ images, const LencUnit* __restrict__ units,
                                                               uint32_t* __restrict__ spans)
{
    __shared__ uint32_t codes[kLencSymbols];
    const LencUnit u = units[blockIdx.x];
    const LencImage& im = images[u.image];
    load_codes(codes, im);
    __syncthreads();
    const uint32_t g = u.first + threadIdx.x;
    if (g >= im.num_groups) return;
    spans[im.first_group + g] = lenc_pack_span(lenc_group_span(im, g, (const HJ_LDS uint32_t*)codes));
}

// One workgroup per picture: offsets = exclusive segmented scan of the groups' spans (henc_span_join: associative, not commutative),
// totals[picture] = the bits of the whole scan without the last byte's padding.  The shape of henc_scan_rst_kernel, over spans.
__global__ __launch_bounds__(kThreads) void lenc_scan_kernel(const LencImage* __restrict__ images, const uint32_t* __restrict__ spans,
                                                             uint32_t* __restrict__ offsets, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t s_a[kThreads], s_b[kThreads], s_cut[kThreads];
    const LencImage& im = images[blockIdx.x];
    const uint32_t* in = spans + im.first_group;
    uint32_t* off = offsets + im.first_group;
    const uint32_t n = im.num_groups;
    const uint32_t per = (n + kThreads - 1) / kThreads;
    const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    constexpr int kBatch = 8;  // independent loads in flight per lane
    HencSpan sp{0u, 0u, 0u};
    for (uint32_t i = lo; i < hi; i += kBatch) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) d[k] = i + k < hi ? in[i + k] : 0u;  // a zero word is the empty span
#pragma unroll
        for (int k = 0; k < kBatch; k++) sp = henc_span_join(sp, lenc_unpack_span(d[k]));
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
    for (uint32_t i = lo; i < hi; i += kBatch) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) d[k] = i + k < hi ? in[i + k] : 0u;
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            if (i + k < hi) {
                off[i + k] = run;
                run = henc_span_apply(run, lenc_unpack_span(d[k]));
            }
        }
    }
    if (threadIdx.x == kThreads - 1) totals[im.index] = henc_span_apply(0u, HencSpan{s_a[kThreads - 1], s_b[kThreads - 1], s_cut[kThreads - 1]});
}

// Word sink of the write kernel's emitter: the workgroup's LDS window (zeroed; bits OR-ed in with LDS atomics).  A word outside the
// window cannot come from samples inside 0 .. 2^P - 1 and a table built from their counts; it is dropped, not stored.
struct WindowWords {
    HJ_LDS uint32_t* window;  // (LDS address 0 is a valid place for it: never test this pointer)
    uint32_t word0, nwords;
    __device__ __forceinline__ void or_word(uint32_t widx, uint32_t w) const  // w: bits in stream order, most significant first
    {
        const uint32_t i = widx - word0;
        if (i < nwords) __hip_atomic_fetch_or(&window[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

struct MapMark {
    uint32_t* map;       // the bitmap behind the bit buffer: bit i = byte i holds a marker's FF
    uint32_t raw_bytes;
    __device__ __forceinline__ void operator()(uint32_t byte) const
    {
        if (byte < raw_bytes) atomicOr(map + (byte >> 5), 1u << (byte & 31));
    }
};

__global__ __launch_bounds__(kThreads) void lenc_write_kernel(const LencImage* __restrict__ images, const LencUnit* __restrict__ units,
                                                              const HencImage* __restrict__ out, const uint32_t* __restrict__ offsets)
{
    __shared__ uint32_t codes[kLencSymbols];
    __shared__ uint32_t window[kLencWindowWords];
    __shared__ uint32_t span[2];  // first word of the workgroup's range, number of words
    const LencUnit u = units[blockIdx.x];
    const LencImage& im = images[u.image];
    const HencImage& o = out[im.index];
    uint8_t* const raw = o.raw;
    const uint32_t raw_bytes = o.raw_bytes;
    load_codes(codes, im);
    const uint32_t t = threadIdx.x;
    const uint32_t g = u.first + t;
    const uint32_t* off = offsets + im.first_group;
    if (t == 0) {
        // [offset of the first group, offset of the next workgroup's first group): exact, so that only the two end words can be shared
        // with a neighbour.  The picture's last workgroup ends with the padded last byte.
        const uint32_t first_bit = off[u.first];
        const uint32_t end_bit = u.first + kThreads < im.num_groups ? off[u.first + kThreads] : raw_bytes * 8u;
        const uint32_t w0 = first_bit >> 5;
        const uint32_t nw = end_bit > first_bit ? ((end_bit - 1) >> 5) - w0 + 1 : 0u;
        span[0] = w0;
        span[1] = min(nw, (uint32_t)kLencWindowWords);
    }
    __syncthreads();
    const uint32_t w0 = span[0], nwin = span[1];
    for (uint32_t i = t; i < nwin; i += kThreads) window[i] = 0;
    __syncthreads();
    if (g < im.num_groups) {
        const uint32_t bit = off[g];
        HencEmitter<WindowWords> em;
        em.start(WindowWords{(HJ_LDS uint32_t*)window, w0, nwin}, bit);
        lenc_group_write(im, g, bit, (const HJ_LDS uint32_t*)codes, &em,
                         MapMark{reinterpret_cast<uint32_t*>(raw + henc_map_offset(raw_bytes)), raw_bytes});
        em.finish();
    }
    __syncthreads();
    uint32_t* gw = reinterpret_cast<uint32_t*>(raw);
    const uint32_t raw_words = (raw_bytes + 3) / 4;  // (16 bytes of slack follow the buffer)
    for (uint32_t i = t; i < nwin; i += kThreads) {
        if (w0 + i >= raw_words) break;
        const uint32_t w = __builtin_bswap32(window[i]);
        if (i == 0 || i == nwin - 1) {
            if (w) atomicOr(&gw[w0 + i], w);  // may be shared with the neighbouring workgroup
        } else {
            gw[w0 + i] = w;
        }
    }
}

}  // namespace

hipError_t launch_lenc_stats(const LencImage* images, int nimages, hipStream_t stream)
{
    if (nimages <= 0) return hipSuccess;
    hipLaunchKernelGGL(lenc_stats_kernel, dim3((unsigned)nimages, kStatGrid), dim3(kThreads), 0, stream, images);
    return hipGetLastError();
}

hipError_t launch_lenc_length(const LencImage* images, const LencUnit* units, int nunits, uint32_t* spans, hipStream_t stream)
{
    if (nunits <= 0) return hipSuccess;
    hipLaunchKernelGGL(lenc_length_kernel, dim3((unsigned)nunits), dim3(kThreads), 0, stream, images, units, spans);
    return hipGetLastError();
}

hipError_t launch_lenc_scan(const LencImage* images, int nimages, const uint32_t* spans, uint32_t* offsets, uint32_t* totals, hipStream_t stream)
{
    if (nimages <= 0) return hipSuccess;
    hipLaunchKernelGGL(lenc_scan_kernel, dim3((unsigned)nimages), dim3(kThreads), 0, stream, images, spans, offsets, totals);
    return hipGetLastError();
}

hipError_t launch_lenc_write(const LencImage* images, const LencUnit* units, int nunits, const HencImage* out, const uint32_t* offsets,
                             hipStream_t stream)
{
    if (nunits <= 0) return hipSuccess;
    hipLaunchKernelGGL(lenc_write_kernel, dim3((unsigned)nunits), dim3(kThreads), 0, stream, images, units, out, offsets);
    return hipGetLastError();
}

}  // namespace hipjpeg
