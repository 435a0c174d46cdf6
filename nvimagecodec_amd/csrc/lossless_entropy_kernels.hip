// lossless_entropy_kernels.hip -- the GPU entropy stage of the lossless (SOF3) decoder: compressed scans in, difference planes out, in
// the layout lossless_entropy_decode leaves on the host, so that the reconstruction kernels run unchanged behind it.  What a lane does
// is in lossless_gpu_core.h; here is the schedule.  The host twin (lossless_gpu_host.cpp) runs the same schedule on the CPU.
//
//   ll_destuff_count_kernel / ll_destuff_compact_kernel   a workgroup per chunk of kLlDestuffChunk raw bytes of a segment, 16 bytes a
//       lane: the stuffed zeros are counted, then the kept bytes go to the segment's stream behind those of the chunks and lanes in
//       front.  The workgroup of a segment's last chunk publishes its bit count.  (Thin kernels of their own: HuffImage describes one
//       scan whose markers are dropped with the zeros and whose interval starts the host supplies in destuffed bits.  Here every interval
//       is a stream of its own whose destuffed length only the device knows.)
//   ll_sync_kernel   launch 0: pass 0 and the correction rounds inside the workgroup.  Launches 1 .. kLlMaxRipple: a workgroup whose
//       first lane started from another state than the unit in front ended in, or whose rounds were not finished, runs its rounds
//       again; the others leave at once.
//   ll_write_kernel  proof of convergence, sample counts, stores (direct: a lane's samples are consecutive in the stream, and in the
//       planes every ncomp-th of them lies next to the one before).
// All of them: 256 lanes, the lookup tables of the unit's image (4 KB at the most) built in LDS from the tables' specifications, no scratch.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "lossless_entropy_kernels.h"

namespace hipjpeg {

namespace {

constexpr int kThreads = (int)kLlLanes;

__device__ __forceinline__ uint32_t wg_sum(uint32_t v, uint32_t* scratch /*[4]*/)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t total = scratch[0] + scratch[1] + scratch[2] + scratch[3];
    __syncthreads();
    return total;
}

// exclusive sum over the workgroup's lanes, and the total
__device__ __forceinline__ uint32_t wg_exclusive_sum(uint32_t v, uint32_t* scratch /*[4]*/, uint32_t* total)
{
    const int t = threadIdx.x;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_up(incl, d);
        if ((t & 63) >= d) incl += n;
    }
    if ((t & 63) == 63) scratch[t >> 6] = incl;
    __syncthreads();
    uint32_t excl = incl - v;
    for (int w = 0; w < (t >> 6); w++) excl += scratch[w];
    *total = scratch[0] + scratch[1] + scratch[2] + scratch[3];
    __syncthreads();
    return excl;
}

// a lane's 16 raw bytes in registers, and the byte in front of them
struct LaneBytes {
    u32x4 w;
    uint32_t first, prev;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        if (i + 1u == first) return prev;
        const uint32_t k = i - first;
        const uint32_t word = k < 4u ? w.x : k < 8u ? w.y : k < 12u ? w.z : w.w;
        return (word >> (8u * (k & 3u))) & 0xFFu;
    }
};

__device__ __forceinline__ LaneBytes load_lane_bytes(const LlSegment& sg, uint32_t off)
{
    LaneBytes b;
    b.first = off;
    b.w = *(const HJ_GLOBAL u32x4*)(sg.raw + off);  // the raw copy is padded to whole 16-byte pieces
    b.prev = off > 0 ? sg.raw[off - 1] : 0u;
    return b;
}

__global__ __launch_bounds__(kThreads) void ll_destuff_count_kernel(const LlSegment* __restrict__ segments, const LlUnit* __restrict__ units,
                                                                    uint32_t* __restrict__ drops)
{
    __shared__ uint32_t scratch[4];
    const LlUnit u = units[blockIdx.x];
    const LlSegment sg = segments[u.segment];
    const uint32_t off = u.first * kLlDestuffChunk + threadIdx.x * kLlDestuffLaneBytes;
    uint32_t n = 0;
    if (off < sg.raw_bytes) {
        const uint32_t len = min(kLlDestuffLaneBytes, sg.raw_bytes - off);
        const LaneBytes b = load_lane_bytes(sg, off);
        n = __popc(ll_destuff_mask(b, off, kLlDestuffLaneBytes) & ((1u << len) - 1u));
    }
    const uint32_t total = wg_sum(n, scratch);
    if (threadIdx.x == 0) drops[sg.first_chunk + u.first] = total;
}

__global__ __launch_bounds__(kThreads) void ll_destuff_compact_kernel(const LlSegment* __restrict__ segments, const LlUnit* __restrict__ units,
                                                                      const uint32_t* __restrict__ drops, uint32_t* __restrict__ seg_bits)
{
    __shared__ uint32_t scratch[4];
    const LlUnit u = units[blockIdx.x];
    const LlSegment sg = segments[u.segment];
    const uint32_t t = threadIdx.x;
    uint32_t before = 0;
    for (uint32_t c = t; c < u.first; c += kThreads) before += drops[sg.first_chunk + c];
    before = wg_sum(before, scratch);
    const uint32_t chunk_begin = u.first * kLlDestuffChunk;
    const uint32_t off = chunk_begin + t * kLlDestuffLaneBytes;
    uint32_t mask = 0, len = 0;
    LaneBytes b;
    b.w = u32x4{0, 0, 0, 0};
    b.first = off;
    b.prev = 0;
    if (off < sg.raw_bytes) {
        len = min(kLlDestuffLaneBytes, sg.raw_bytes - off);
        b = load_lane_bytes(sg, off);
        mask = ll_destuff_mask(b, off, kLlDestuffLaneBytes) & ((1u << len) - 1u);
    }
    uint32_t chunk_drops;
    const uint32_t excl = wg_exclusive_sum(__popc(mask), scratch, &chunk_drops);
    // kept bytes: behind those of the chunks and lanes in front; off - before - excl <= off, inside the stream's raw_bytes
    HJ_GLOBAL uint8_t* dst = (HJ_GLOBAL uint8_t*)sg.stream + (off - before - excl);
#pragma unroll
    for (uint32_t i = 0; i < kLlDestuffLaneBytes; i++)
        if (i < len && !((mask >> i) & 1u)) *dst++ = (uint8_t)b(off + i);
    const uint32_t chunk_len = min(kLlDestuffChunk, sg.raw_bytes - chunk_begin);
    if (chunk_begin + chunk_len == sg.raw_bytes) {  // the segment's last chunk: ones up to the word's end, and the bit count
        const uint32_t total = sg.raw_bytes - before - chunk_drops;
        if (t < 4u && total + t < ((total + 3u) & ~3u)) ((HJ_GLOBAL uint8_t*)sg.stream)[total + t] = 0xFFu;
        if (t == 0) seg_bits[u.segment] = total * 8u;
    }
}

// A segment's bit count, by a vector load: the index is the same in every lane, and hipcc may make it the register offset of a scalar
// load, a form this project keeps out of its kernels (DESIGN "A compiler hazard worth recording", tests/test_code_object_hazards.py).
__device__ __forceinline__ uint32_t segment_bits(const uint32_t* seg_bits, uint32_t segment)
{
    return *(const volatile HJ_GLOBAL uint32_t*)(seg_bits + segment);
}

// what the parse reads through
struct KernelEnv {
    const HJ_GLOBAL uint32_t* words;
    uint32_t nwords;
    const HJ_LDS uint32_t* tables;
    __device__ __forceinline__ uint32_t word(uint32_t k) const { return k < nwords ? __builtin_bswap32(words[k]) : 0xFFFFFFFFu; }
    __device__ __forceinline__ uint32_t tab(uint32_t t, uint32_t w) const { return tables[t * kLlTableWords + w]; }
};

// byte i of a table specification, from its copy in LDS
struct SpecBytes {
    const HJ_LDS uint32_t* words;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (words[i >> 2] >> (8u * (i & 3u))) & 0xFFu; }
};

// The lookup tables of the image into LDS: the specifications first (vector loads: a lane a word), then a lane builds word t of every
// table (kLlTableWords == kThreads).  Holds a barrier: every lane of the workgroup calls it.
__device__ __forceinline__ void stage_tables(uint32_t* lds, uint32_t* lds_specs /*[4 * kLlSpecWords]*/, const LlImage& im)
{
    static_assert(kLlTableWords == (uint32_t)kThreads, "a word per lane");
    const uint32_t n = min(im.ntables, 4u);
    if (threadIdx.x < n * kLlSpecWords) lds_specs[threadIdx.x] = ((const HJ_GLOBAL uint32_t*)im.specs)[threadIdx.x];
    __syncthreads();
    for (uint32_t t = 0; t < n; t++) {
        const SpecBytes spec{(const HJ_LDS uint32_t*)lds_specs + t * kLlSpecWords};
        lds[t * kLlTableWords + threadIdx.x] = ll_table_word(spec, threadIdx.x);
    }
}

__global__ __launch_bounds__(kThreads) void ll_sync_kernel(LlArrays a, uint32_t launch)
{
    __shared__ uint32_t tables[4 * kLlTableWords];
    __shared__ uint32_t specs[4 * kLlSpecWords];
    __shared__ uint64_t ends[kThreads];
    __shared__ uint32_t scratch[4];
    const uint32_t unit = blockIdx.x, t = threadIdx.x;
    const LlUnit u = a.units[unit];
    const LlSegment sg = a.segments[u.segment];
    const uint32_t total_bits = segment_bits(a.seg_bits, u.segment);
    const uint32_t nsub = min(ll_num_subseq(total_bits), sg.max_subseq);
    const uint32_t i = u.first + t;
    const bool active = i < nsub;
    const size_t slot = (size_t)sg.first_subseq + i;
    const size_t out_now = (size_t)(launch & 1u) * a.num_units + unit, out_before = (size_t)((launch & 1u) ^ 1u) * a.num_units + unit;

    uint64_t start = 0, end = 0, incoming = 0;
    uint32_t n = 0;
    if (launch > 0) {
        if (active) {
            start = a.start[slot];
            end = a.end[slot];
            n = a.count[slot];
        }
        // nothing to do where every lane started from the state the one in front ended in (or that one ended in no state at all): the
        // first lane looks at the unit in front, the others at what the rounds of the launch before left unfinished
        bool need = false;
        if (active && i > 0) {
            const uint64_t pred = t > 0 ? a.end[slot - 1] : a.unit_out[out_before - 1];
            if (t == 0) incoming = pred;
            need = pred != kLlInvalidPacked && pred != start;
        }
        if (t == 0) a.unit_out[out_now] = a.unit_out[out_before];
        if (!__syncthreads_or(need)) return;
        if (t == 0) atomicAdd(&a.moved[launch], 1u);
    }
    const LlImage& im = a.images[sg.image];
    stage_tables(tables, specs, im);
    __syncthreads();
    KernelEnv env;
    env.words = (const HJ_GLOBAL uint32_t*)sg.stream;
    env.nwords = (total_bits + 31u) / 32u;
    env.tables = (const HJ_LDS uint32_t*)tables;
    const bool shared = im.ntables == 1u;
    const uint32_t phases = shared ? 1u : im.ncomp;
    const uint32_t limit = active ? ll_limit(i, total_bits) : 0u;
    LlNoSink sink;
    if (launch == 0 && active) {
        LlState st{0u, 0u}, from = st;
        if (i == 0)
            n = ll_parse(env, phases, shared, total_bits, limit, &st, sink);  // the segment's first bit: no guess
        else
            n = ll_pass0(env, phases, shared, total_bits, i, limit, &from, &st);
        start = ll_pack(from);
        end = ll_pack(st);
    }
    ends[t] = end;
    __syncthreads();
    for (uint32_t round = 0; round < kLlMaxRounds; round++) {
        const uint64_t pred = t > 0 ? ends[t - 1] : (launch > 0 && u.first > 0 ? incoming : start);
        const bool redo = active && pred != kLlInvalidPacked && pred != start;
        if (!__syncthreads_or(redo)) break;
        if (redo) {
            LlState st = ll_unpack(pred);
            start = pred;
            n = ll_parse(env, phases, shared, total_bits, limit, &st, sink);
            end = ll_pack(st);
            ends[t] = end;
        }
        __syncthreads();
    }
    if (active) {
        a.start[slot] = start;
        a.end[slot] = end;
        a.count[slot] = n;
    }
    if (t == 0) {  // (the thread that copied the old border state above)
        const uint32_t lanes = nsub > u.first ? min(nsub - u.first, kLlLanes) : 0u;
        a.unit_out[out_now] = lanes ? ends[lanes - 1u] : 0ull;
    }
    const uint32_t total = wg_sum(active ? n : 0u, scratch);
    if (t == 0) a.unit_count[unit] = total;
}

struct PlaneSink {
    HJ_GLOBAL uint16_t *p0, *p1, *p2, *p3;  // (four names, not an array: an index that changes per sample would put it in scratch)
    uint32_t ncomp, width, height, pitch;
    LlCursor cur;
    uint32_t k, samples;  // index of the next sample in the segment, and the segment's count
    __device__ __forceinline__ void operator()(uint32_t v)
    {
        if (k < samples && cur.row < height) {
            HJ_GLOBAL uint16_t* p = cur.comp == 0 ? p0 : cur.comp == 1 ? p1 : cur.comp == 2 ? p2 : p3;
            p[(size_t)cur.row * pitch + cur.x] = (uint16_t)v;
        }
        k++;
        cur.next(ncomp, width);
    }
};

__global__ __launch_bounds__(kThreads) void ll_write_kernel(LlArrays a)
{
    __shared__ uint32_t tables[4 * kLlTableWords];
    __shared__ uint32_t specs[4 * kLlSpecWords];
    __shared__ uint32_t scratch[4];
    const uint32_t unit = blockIdx.x, t = threadIdx.x;
    const LlUnit u = a.units[unit];
    const LlSegment sg = a.segments[u.segment];
    const uint32_t total_bits = segment_bits(a.seg_bits, u.segment);
    const uint32_t nsub = min(ll_num_subseq(total_bits), sg.max_subseq);
    if (u.first >= nsub) return;  // (a unit planned for bytes that were stuffing)
    const uint32_t i = u.first + t;
    const bool active = i < nsub;
    const size_t slot = (size_t)sg.first_subseq + i;
    const LlImage& im = a.images[sg.image];
    stage_tables(tables, specs, im);

    uint64_t start = 0, end = 0;
    uint32_t n = 0, verdict = 0;
    if (active) {
        start = a.start[slot];
        end = a.end[slot];
        n = a.count[slot];
        // the proof: this lane started where the one in front ended
        const uint64_t pred = i == 0 ? 0ull : a.end[slot - 1];
        if (pred != start) verdict |= kLlUnconverged;
        if (end == kLlInvalidPacked) verdict |= kLlInvalidCode;
    }
    // samples in front of this lane: the units of the segment in front of this one, then the lanes
    uint32_t before = 0;
    for (uint32_t c = sg.first_unit + t; c < unit; c += kThreads) before += a.unit_count[c];
    before = wg_sum(before, scratch);
    uint32_t total;
    const uint32_t excl = wg_exclusive_sum(n, scratch, &total);
    if (active && i + 1u == nsub && before + total != sg.samples) verdict |= kLlBadCount;
    if (verdict) atomicOr(&a.verdicts[sg.image], verdict);
    if (!active || n == 0) return;  // (the tables are staged by now: every lane passed wg_sum's barriers)

    KernelEnv env;
    env.words = (const HJ_GLOBAL uint32_t*)sg.stream;
    env.nwords = (total_bits + 31u) / 32u;
    env.tables = (const HJ_LDS uint32_t*)tables;
    const uint32_t ncomp = min(im.ncomp, 4u);
    PlaneSink sink{(HJ_GLOBAL uint16_t*)im.plane[0], (HJ_GLOBAL uint16_t*)im.plane[1], (HJ_GLOBAL uint16_t*)im.plane[2], (HJ_GLOBAL uint16_t*)im.plane[3],
                   ncomp, im.width, im.height, im.pitch, LlCursor(), before + excl, sg.samples};
    if (sink.k >= sg.samples) return;
    sink.cur.start(ncomp, im.width, sg.first_row, sink.k);
    LlState st = ll_unpack(start);
    st.phase = sink.cur.comp;  // a segment starts at phase 0, so the sample's index gives the phase: also where the walks kept it at 0
    (void)ll_parse(env, ncomp, im.ntables == 1u, total_bits, ll_limit(i, total_bits), &st, sink);
}

}  // namespace

hipError_t launch_lossless_entropy_sync(const LlArrays& a, hipStream_t stream)
{
    if (a.num_chunk_units <= 0 || a.num_units <= 0) return hipSuccess;
    hipLaunchKernelGGL(ll_destuff_count_kernel, dim3(a.num_chunk_units), dim3(kThreads), 0, stream, a.segments, a.chunk_units, a.drops);
    hipLaunchKernelGGL(ll_destuff_compact_kernel, dim3(a.num_chunk_units), dim3(kThreads), 0, stream, a.segments, a.chunk_units, a.drops, a.seg_bits);
    for (uint32_t launch = 0; launch <= kLlMaxRipple; launch++)
        hipLaunchKernelGGL(ll_sync_kernel, dim3(a.num_units), dim3(kThreads), 0, stream, a, launch);
    return hipGetLastError();
}

hipError_t launch_lossless_entropy_write(const LlArrays& a, hipStream_t stream)
{
    if (a.num_units <= 0) return hipSuccess;
    hipLaunchKernelGGL(ll_write_kernel, dim3(a.num_units), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hipjpeg
