// progressive_encode.hip -- gfx950 kernels of the GPU coder's progressive output (see progressive_encode.h for the pipeline and
// progressive_encode_core.h for the per-block routines, which the host emulation runs as well).
#include <hip/hip_runtime.h>

#include "huffman_encode_core.h"  // henc_map_offset
#include "kernel_common.h"
#include "progressive_encode.h"

namespace hipjpeg {

namespace {

constexpr int kThreads = 256;

struct LdsCount {  // symbol counts of one workgroup
    HJ_LDS uint32_t* h;
    __device__ void sym(int s) const { __hip_atomic_fetch_add(&h[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ void bits(uint32_t, int) const {}
};

struct GlobalWords {  // the scan's bit buffer: big-endian words, OR-ed in (neighbouring blocks share words)
    uint32_t* p;
    __device__ void or_word(uint32_t i, uint32_t w) const { atomicOr(&p[i], __builtin_bswap32(w)); }
};

__device__ PencBlockArrays at_scan(const PencBlockArrays& a, uint32_t fb)
{
    return PencBlockArrays{a.sum + fb, a.pre + fb, a.post + fb, a.piece + fb, a.flusher + fb, a.rel + fb, a.own + fb, a.bits + fb, a.off + fb};
}

// RST (all four kernels): the launch has scans with restart intervals (PencScan::rst_blocks, progressive_encode_core.h).
template <bool RST>
__global__ __launch_bounds__(kThreads) void penc_summary_kernel(const PencScan* __restrict__ scans, const HencUnit* __restrict__ units,
                                                                uint8_t* __restrict__ sum)
{
    __shared__ uint32_t hist[256];
    const HencUnit u = units[blockIdx.x];
    const PencScan& sc = scans[u.image];
    if (sc.kind == kPencDcRefine) return;  // uniform: no table, nothing to count
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = u.first + threadIdx.x;
    if (i < sc.nblocks) {
        LdsCount cnt{(HJ_LDS uint32_t*)hist};
        const uint32_t s = penc_block_summary<RST>(sc, i, cnt);
        if (sc.kind != kPencDcFirst) sum[sc.first_block + i] = (uint8_t)s;
    }
    __syncthreads();
    const uint32_t v = hist[threadIdx.x];
    if (v) atomicAdd(&sc.hist[threadIdx.x], v);
}

// One wave per AC scan walks the run recurrence 64 blocks at a time: the summaries are loaded by the lanes, the steps taken in
// order with the state in scalar registers, and every lane stores the results of its own block.  A stretch of 64 empty blocks
// (tail, no content, no correction bits) that cannot reach 0x7FFF only lengthens the run and is taken in one step -- unless one of
// them ends a restart interval, whose flush the steps have to see.
template <bool RST>
__global__ __launch_bounds__(64) void penc_runs_kernel(const PencScan* __restrict__ scans, const uint32_t* __restrict__ ac_scans,
                                                       const uint8_t* __restrict__ sum, uint32_t* __restrict__ pre, uint32_t* __restrict__ post,
                                                       uint32_t* __restrict__ piece, uint32_t* __restrict__ flusher, uint16_t* __restrict__ rel)
{
    const PencScan& sc = scans[ac_scans[blockIdx.x]];
    const uint32_t lane = threadIdx.x, n = sc.nblocks, fb = sc.first_block;
    PencIntervalEnds<RST> ends(sc.rst_blocks, n);
    PencRun r{0, 0, 0};
    uint32_t eobs = 0;  // lane j counts the EOBn symbols with j bits of run length (symbol j << 4)
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        const uint32_t s = i < n ? (uint32_t)sum[fb + i] : 2u;
        const uint32_t cnt = min(64u, n - base);
        if (__ballot(s != 2u) == 0 && r.n + cnt < kPencMaxRun && !ends.before(base + cnt)) {
            if (r.n == 0) r.ps = base;
            r.n += cnt;
            continue;
        }
        PencStep mine{0, 0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t sk = (uint32_t)__builtin_amdgcn_readlane((int)s, (int)k);
            const PencStep st = penc_run_step<RST>(r, base + k, sk, ends.at(base + k));
            if (st.pre) eobs += lane == (uint32_t)penc_eob_nbits(st.pre & 0xFFFF) ? 1u : 0u;
            if (st.post) eobs += lane == (uint32_t)penc_eob_nbits(st.post & 0xFFFF) ? 1u : 0u;
            if (lane == k) mine = st;
        }
        if (i < n) {
            if (mine.pre) {
                pre[fb + i] = mine.pre;
                flusher[fb + mine.pre_ps] = i;
            }
            if (mine.post) {
                post[fb + i] = mine.post;
                flusher[fb + mine.post_ps] = i;
            }
            if ((s & 2) && (s >> 2)) {
                piece[fb + i] = mine.ps;
                rel[fb + i] = (uint16_t)mine.rel;
            }
        }
    }
    const uint32_t e = penc_run_end(r);
    if (e) {
        eobs += lane == (uint32_t)penc_eob_nbits(e & 0xFFFF) ? 1u : 0u;
        if (lane == 0) {
            post[fb + n - 1] = e;
            flusher[fb + r.ps] = n - 1;
        }
    }
    if (lane < 15 && eobs) atomicAdd(&sc.hist[lane << 4], eobs);
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void penc_length_kernel(const PencScan* __restrict__ scans, const HencUnit* __restrict__ units,
                                                               const uint32_t* __restrict__ pre, const uint32_t* __restrict__ post,
                                                               uint16_t* __restrict__ own, uint16_t* __restrict__ bits)
{
    __shared__ uint32_t codes[256];
    const HencUnit u = units[blockIdx.x];
    const PencScan& sc = scans[u.image];
    if (sc.kind != kPencDcRefine) codes[threadIdx.x] = sc.codes[threadIdx.x];
    __syncthreads();
    const uint32_t i = u.first + threadIdx.x;
    if (i >= sc.nblocks) return;
    const size_t g = (size_t)sc.first_block + i;
    const bool ac = sc.kind >= kPencAcFirst;
    uint32_t o;
    const uint32_t len = penc_block_length<RST>(sc, i, codes, ac ? pre[g] : 0u, ac ? post[g] : 0u, &o);
    own[g] = (uint16_t)o;
    bits[g] = (uint16_t)len;
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void penc_write_kernel(const PencScan* __restrict__ scans, const HencImage* __restrict__ segs,
                                                              const HencUnit* __restrict__ units, PencBlockArrays a)
{
    __shared__ uint32_t codes[256];
    const HencUnit u = units[blockIdx.x];
    const PencScan& sc = scans[u.image];
    if (sc.kind != kPencDcRefine) codes[threadIdx.x] = sc.codes[threadIdx.x];
    __syncthreads();
    const uint32_t i = u.first + threadIdx.x;
    if (i >= sc.nblocks) return;
    const HencImage& seg = segs[u.image];
    const GlobalWords words{reinterpret_cast<uint32_t*>(seg.raw)};
    const uint32_t marker = penc_block_write<RST>(sc, i, codes, words, at_scan(a, sc.first_block));
    // RSTn is marked in the bitmap behind the bit buffer, so that count / expand do not stuff its FF (huffman_encode_core.h)
    if (RST && marker != ~0u) atomicOr(reinterpret_cast<uint32_t*>(seg.raw + henc_map_offset(seg.raw_bytes)) + (marker >> 5), 1u << (marker & 31));
}

}  // namespace

// `restart`: the launch has scans with restart intervals and takes the kernels' flavour that carries them; without it the kernels are
// the ones a batch without restart intervals has always run.
int launch_penc_summary(const PencScan* scans, const HencUnit* units, int nunits, uint8_t* sum, void* stream, bool restart)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(restart ? penc_summary_kernel<true> : penc_summary_kernel<false>, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, scans, units, sum);
    return (int)hipGetLastError();
}

int launch_penc_runs(const PencScan* scans, const uint32_t* ac_scans, int nac, const uint8_t* sum, uint32_t* pre, uint32_t* post, uint32_t* piece,
                     uint32_t* flusher, uint16_t* rel, void* stream, bool restart)
{
    if (nac <= 0) return 0;
    hipLaunchKernelGGL(restart ? penc_runs_kernel<true> : penc_runs_kernel<false>, dim3(nac), dim3(64), 0, (hipStream_t)stream, scans, ac_scans, sum, pre, post, piece, flusher, rel);
    return (int)hipGetLastError();
}

int launch_penc_length(const PencScan* scans, const HencUnit* units, int nunits, const uint32_t* pre, const uint32_t* post, uint16_t* own,
                       uint16_t* bits, void* stream, bool restart)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(restart ? penc_length_kernel<true> : penc_length_kernel<false>, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, scans, units, pre, post, own, bits);
    return (int)hipGetLastError();
}

int launch_penc_write(const PencScan* scans, const HencImage* segs, const HencUnit* units, int nunits, const PencBlockArrays& a, void* stream, bool restart)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(restart ? penc_write_kernel<true> : penc_write_kernel<false>, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, scans, segs, units, a);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
