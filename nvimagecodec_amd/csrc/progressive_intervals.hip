// progressive_intervals.hip -- gfx950 kernels for progressive (SOF2) files whose scans all have restart intervals.  Algorithm and the
// reasons: progressive_interval_core.h.  They stand in for prog_walk_kernel (progressive_gpu.hip) for such images: they leave the block
// start positions of every AC scan and the compact DC planes behind, and prog_replay_kernel takes it from there.
//
//   prog_interval_ac_kernel   a workgroup of 256 lanes = 256 consecutive restart intervals of one (image, component); a lane parses its
//                             interval of every AC scan of the component, in file order.  The chain's lookup tables sit in LDS.
//   prog_interval_dc_kernel   a workgroup = 256 consecutive intervals of one (image, DC scan); launched once per DC-scan index.
// The per-lane code is divergent by nature (every lane is its own scalar decoder), as the replay kernel's is.
#include <hip/hip_runtime.h>

#include "gpu_huffman.h"
#include "kernel_common.h"
#include "progressive_gpu.h"
#include "progressive_interval_core.h"

namespace hipjpeg {

namespace {

struct IntervalEnv {
    const HuffImage* himgs;
    const ProgImage* im;
    const ProgIntervalImage* iv;
    const HJ_GLOBAL uint32_t* starts;
    const HJ_LDS uint16_t* tables;
    uint32_t slot_words;
    HJ_GLOBAL unsigned long long* hist_all;  // the component's bitmaps (AC items)
    __device__ __forceinline__ uint32_t word(const ProgScan& sc, uint32_t i) const
    {
        const uint32_t n = himgs[sc.huff_image].stream_words;
        return i < n ? __builtin_bswap32(((const HJ_GLOBAL uint32_t*)sc.stream)[i]) : ~0u;
    }
    __device__ __forceinline__ uint32_t entry(const HJ_LDS uint16_t* t, uint32_t w) const
    {
        uint32_t e = t[w >> 24];
        if (e & kProgLong) e = t[(e & 0x7FFFu) * 256u + ((w >> 16) & 255u)];
        return e;
    }
    __device__ __forceinline__ uint32_t lookup(const ProgScan& sc, uint32_t w) const { return entry(tables + (uint32_t)sc.stage * slot_words, w); }
    __device__ __forceinline__ uint32_t dc_lookup(const ProgScan&, uint32_t slot, uint32_t w) const { return entry(tables + slot * slot_words, w); }
    __device__ __forceinline__ uint32_t bound(uint32_t s, uint32_t k) const
    {
        const ProgIntervalScan& q = iv->scan[s];
        if (k == 0) return 0u;
        if (k < q.count) return starts[q.first_start + k - 1u];
        return himgs[im->scan[s].huff_image].total_bits;
    }
    __device__ __forceinline__ unsigned long long hist(uint32_t b) const { return hist_all[b]; }
    __device__ __forceinline__ void set_hist(uint32_t b, unsigned long long h) const { hist_all[b] = h; }
    __device__ __forceinline__ void set_pos(const ProgScan& sc, uint32_t b, uint32_t v) const { ((HJ_GLOBAL uint32_t*)sc.block_pos)[b] = v; }
    __device__ __forceinline__ void dc_store(uint32_t c, uint32_t index, int v) const { ((HJ_GLOBAL int16_t*)im->dc_plane[c])[index] = (int16_t)v; }
    __device__ __forceinline__ void dc_or(uint32_t c, uint32_t index, int bits) const
    {
        HJ_GLOBAL int16_t* p = (HJ_GLOBAL int16_t*)im->dc_plane[c] + index;
        *p = (int16_t)(*p | bits);
    }
};

// One lookup table: pool (global) -> LDS slot, by the whole workgroup.  A table is at most slot_words entries (the batch's largest)
// and ends inside the image's pool; tables start at multiples of 64 entries.
__device__ __forceinline__ void stage_slot(HJ_LDS uint16_t* slot, const ProgImage& im, uint32_t offset, uint32_t slot_words, uint32_t t)
{
    const uint32_t left = im.pool_words > offset ? im.pool_words - offset : 0u;
    const uint32_t words = left < slot_words ? left : slot_words;
    const HJ_GLOBAL uint32_t* src = (const HJ_GLOBAL uint32_t*)(im.pool + offset);
    HJ_LDS uint32_t* dst = (HJ_LDS uint32_t*)slot;
    for (uint32_t i = t; i < words / 2; i += kProgIntervalLanes) dst[i] = src[i];
}

// unit = {image, (component << 28) | first interval}
__global__ __launch_bounds__(kProgIntervalLanes) void prog_interval_ac_kernel(ProgImage* __restrict__ images, const ProgIntervalImage* __restrict__ ivs,
                                                                              const HuffImage* __restrict__ himgs, const uint32_t* __restrict__ starts,
                                                                              const HuffUnit* __restrict__ units, uint32_t slot_words)
{
    extern __shared__ u32x4 dyn_interval_lds[];  // kProgMaxStages table slots (uint16 entries), 16-byte aligned
    HJ_LDS uint16_t* tables = (HJ_LDS uint16_t*)dyn_interval_lds;
    const HuffUnit u = units[blockIdx.x];
    ProgImage& im = images[u.image];
    const ProgIntervalImage& iv = ivs[u.image];
    const int c = (int)(u.first >> 28);
    const uint32_t t = threadIdx.x, i = (u.first & 0x0FFFFFFFu) + t;
    const uint32_t stages = im.chain_len[c] < (uint32_t)kProgMaxStages ? im.chain_len[c] : (uint32_t)kProgMaxStages;
    for (uint32_t st = 0; st < stages; st++) stage_slot(tables + st * slot_words, im, im.scan[im.chain[c][st]].table[0], slot_words, t);
    __syncthreads();
    if (i >= iv.ac_count[c]) return;
    IntervalEnv env;
    env.himgs = himgs;
    env.im = &im;
    env.iv = &iv;
    env.starts = (const HJ_GLOBAL uint32_t*)starts;
    env.tables = tables;
    env.slot_words = slot_words;
    env.hist_all = (HJ_GLOBAL unsigned long long*)iv.hist[c];
    if (!prog_interval_ac(env, im, iv, c, i)) im.status = 1;  // benign race: every writer stores the same value
}

// unit = {image, first interval} of the image's dc_index-th DC scan
__global__ __launch_bounds__(kProgIntervalLanes) void prog_interval_dc_kernel(ProgImage* __restrict__ images, const ProgIntervalImage* __restrict__ ivs,
                                                                              const HuffImage* __restrict__ himgs, const uint32_t* __restrict__ starts,
                                                                              const HuffUnit* __restrict__ units, uint32_t dc_index, uint32_t slot_words)
{
    extern __shared__ u32x4 dyn_interval_lds[];  // four table slots
    HJ_LDS uint16_t* tables = (HJ_LDS uint16_t*)dyn_interval_lds;
    const HuffUnit u = units[blockIdx.x];
    ProgImage& im = images[u.image];
    const ProgIntervalImage& iv = ivs[u.image];
    const uint32_t sidx = im.dc_chain[dc_index];
    const ProgScan& sc = im.scan[sidx];
    const uint32_t t = threadIdx.x, i = u.first + t;
    if (sc.ah == 0) {  // a first scan: the tables of its components (at most four)
        const uint32_t n = sc.ncomp < 4u ? sc.ncomp : 4u;
        for (uint32_t k = 0; k < n; k++) stage_slot(tables + k * slot_words, im, sc.table[k], slot_words, t);
    }
    __syncthreads();
    if (i >= iv.scan[sidx].count) return;
    IntervalEnv env;
    env.himgs = himgs;
    env.im = &im;
    env.iv = &iv;
    env.starts = (const HJ_GLOBAL uint32_t*)starts;
    env.tables = tables;
    env.slot_words = slot_words;
    env.hist_all = nullptr;
    if (!prog_interval_dc(env, im, iv, sidx, i)) im.status = 1;
}

}  // namespace

int launch_prog_interval_ac(ProgImage* images, const ProgIntervalImage* ivs, const HuffImage* himgs, const uint32_t* starts, const HuffUnit* units,
                            int nunits, unsigned slot_words, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(prog_interval_ac_kernel, dim3(nunits), dim3(kProgIntervalLanes), slot_words * 2u * kProgMaxStages, (hipStream_t)stream, images, ivs,
                       himgs, starts, units, slot_words);
    return (int)hipGetLastError();
}

int launch_prog_interval_dc(ProgImage* images, const ProgIntervalImage* ivs, const HuffImage* himgs, const uint32_t* starts, const HuffUnit* units,
                            int nunits, unsigned dc_index, unsigned slot_words, void* stream)
{
    if (nunits <= 0) return 0;
    // a first scan stages the tables of its components, four at the most; a refinement scan none
    hipLaunchKernelGGL(prog_interval_dc_kernel, dim3(nunits), dim3(kProgIntervalLanes), slot_words * 2u * 4u, (hipStream_t)stream, images, ivs,
                       himgs, starts, units, dc_index, slot_words);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
