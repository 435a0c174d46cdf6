// gpu_huffman.hip -- gfx950 kernels of the GPU entropy decoder (algorithm and data structures: huffman_gpu_core.h).
//
// This is the analogue of nvJPEG's GPU_HYBRID backend that the reference switches to for large baseline images
// (extensions/nvjpeg/cuda_decoder.cpp:512-521): the Huffman stage moves to the device, so neither the host cores nor the
// PCIe copy of 6 MB of coefficients per image sit on the critical path any more -- only the ~0.5 MB bitstream crosses.
//
// Mapping: one lane decodes one 1024-bit subsequence; a workgroup owns 255 (the first launch: 510) consecutive subsequences of ONE image.
// Decoding is inherently serial per lane (data-dependent code lengths); parallelism comes from the number of subsequences
// (4096 per 0.5 MB image, ~1M per 256-image batch).  Everything a lane touches per symbol lives in LDS:
//   * the workgroup's 32 KB of bitstream, loaded once with coalesced dword loads, byte-swapped to MSB-first words and stored
//     one row of 33 words per lane (32 own words + a copy of the successor's first word): the odd row stride spreads lanes
//     that sit at the same column over different banks, and a lane's two-word window never leaves its row;
//   * the image's two-level Huffman lookup tables (uint16 entries, typically ~10 KB);
//   * per-MCU-position table offsets and block addressing constants, the zigzag permutation.
// Kernels:
//   huff_sync_pair_kernel  the first launch: two sync units per workgroup, the paired schedule and the workgroup-local
//                      synchronisation rounds in LDS; publishes end states, hands what is left to huff_tail_kernel
//   huff_sync_kernel   the ripple over single units as a launch of its own (an A/B aid; huff_tail_kernel<true> otherwise): counts the
//                      workgroups whose LAST end state moved (the only state another workgroup consumes)
//   huff_copy_records_kernel  where every block starts: first block index of every subsequence (sums and scans the completed-block
//                      counts), then copies the records the last synchronisation decodes took
//   huff_pos_kernel    walks from the converged states the subsequences without a usable record
//   huff_blocks_kernel one lane per block: decode into LDS, store whole 128-byte lines (DC differences to a compact array);
//                      two 256-lane teams per workgroup share one copy of the tables: 16 waves per CU
//   huff_dc_kernel     per (image, component): DC differences -> DC values, stored into the blocks
#include <hip/hip_runtime.h>

#include <type_traits>

#include "gpu_huffman.h"
#include "huffman_gpu_core.h"
#include "kernel_common.h"

namespace hipjpeg {

namespace {

constexpr int kThreads = 256;

constexpr int kRowShift = kSubseqWords == 32 ? 5 : kSubseqWords == 16 ? 4 : kSubseqWords == 64 ? 6 : -1;  // log2(words per subsequence)
static_assert(kRowShift > 0, "subsequences of 512, 1024 or 2048 bits");

struct KSlot {
    int16_t* base;  // coef[comp] + blk0 * 64
    uint32_t stride_y, stride_x;
};

// Stream words in LDS: every subsequence ("row") is staged together with the kStagedExtra words behind it, which cover the bit
// reader's look-ahead (the last symbol of a walk starts before the row's end: its window reaches into word 32, the word
// requested ahead is word 33) -- a walk never leaves its row -- and the rows are TRANSPOSED: word k of row r sits at index
// k * rows + r.  The bank of an access is then r mod 32 whatever k is: lanes that walk their own rows never collide, however
// far apart their positions are, and stepping to the next word is adding a constant to an address (BitReader's cursor).
constexpr int kStagedExtra = 2;
constexpr int kRowWords = kSubseqWords + kStagedExtra;
static_assert(kSubseqWords % 4 == 0 && kStagedExtra == 2, "stage_rows: 16-byte groups and one 8-byte group per row");
__host__ __device__ constexpr int staged_lds_words(int rows) { return rows * kRowWords; }

struct WgShared {
    uint32_t stream[staged_lds_words(kSyncThreads)];
    unsigned long long end[kSyncThreads];  // end state of lane t's subsequence ([0] = halo = state entering the workgroup)
    uint32_t tsel[10];
    uint32_t queue[kSyncThreads];
    uint32_t wave_count[kSyncThreads / 64];
};

// The first sync launch's workgroup (huff_sync_pair_kernel): two sync units of an image, 2 * kHuffOwn subsequences and the halo.  The
// staged rows hold one parity of them at a time (column t: the row lane t is about to decode), the end states all of them.
constexpr int kPairRows = 2 * kHuffOwn + 1;
struct PairShared {
    uint32_t stream[staged_lds_words(kSyncThreads)];
    unsigned long long end[2 * kSyncThreads];  // end state of local row r ([0] = halo = state entering the workgroup)
    unsigned long long second_from;            // the state the second unit's first subsequence was last decoded from
    uint32_t tsel[10];
    uint32_t wave_count[kSyncThreads / 64];
    uint16_t queue[kSyncThreads];  // a round's tasks are rows of one parity: at most one per lane, below 2 * kSyncThreads
};
// Three workgroups per CU beside the standard tables (13,824 B), LDS handed out in 1,280-byte granules
// (profiles/block_pass_teams/lds_granule.txt): 160 KB / 3 = 54,613 -> 42 granules = 53,760 B each.
static_assert(kSyncThreads != 256 || sizeof(PairShared) + 13824 <= 53760, "huff_sync_pair_kernel: three workgroups per CU");

// restart boundaries live in global memory (a handful of reads per decode; the destuffed positions come from the host's
// marker walk)
__device__ __forceinline__ uint32_t load_boundary(const uint32_t* boundaries, uint32_t n, uint32_t i)
{
    return i < n ? ((const HJ_GLOBAL uint32_t*)boundaries)[i] : 0xFFFFFFFFu;
}
// How the lane walks take a block's end and a long code (huffman_gpu_core.h has both routines).  huff_sync_kernel, whose waves
// have every lane busy, takes both as selects (select_walk: the table selection in registers, a long code as a step of its own,
// the MCU position as a countdown, the tables as two halves with the pool's base inside; profiles/walk_step_diet/README.md).  The
// lane mode of the tail kernels and huff_pos_kernel keep the branches (decode_subsequence, position_subsequence), tsel[] in LDS
// and the second-level read inside the branch: with a few lanes busy, often one, a branch that is not taken is the cheapest form
// (profiles/walk_steps/README.md).  What both forms share by construction is the pair table's layout.

// The image's lookup tables in LDS as every walk reads them: one definition of the accessors huffman_gpu_core.h asks an Env for.
struct LdsTables {
    uint32_t pool;                // LDS byte address of the lookup tables
    const HJ_LDS uint32_t* tsel;  // per MCU position: BYTE offsets of the DC / AC first-level tables, packed lo/hi
    // byte offset of the window's entry inside a first-level (or pair) table, inside a second-level table
    static __device__ __forceinline__ uint32_t index1(uint32_t w) { return (w >> (31 - kHuffFastBits)) & ((2u << kHuffFastBits) - 2); }
    static __device__ __forceinline__ uint32_t index2(uint32_t w) { return (w >> 15) & ((2u << kHuffSubBits) - 2); }
    __device__ __forceinline__ uint32_t tables(int k) const { return tsel[k]; }
    __device__ __forceinline__ uint32_t lookup1(uint32_t t, uint32_t w) const { return *(const HJ_LDS uint16_t*)(uintptr_t)(pool + t + index1(w)); }
    __device__ __forceinline__ uint32_t lookup2(uint32_t e, uint32_t w) const  // (pool offset / 64 entries -> bytes)
    {
        return *(const HJ_LDS uint16_t*)(uintptr_t)(pool + ((e & 0x1FFu) << 7) + index2(w));
    }
    __device__ __forceinline__ uint32_t lookup_pair(uint32_t t, uint32_t w) const  // lookup1's address + a constant: one more LDS read, no more arithmetic
    {
        return *(const HJ_LDS uint16_t*)(uintptr_t)(pool + t + 2 * kPairOffset + index1(w));
    }
};

// The table selection of the select step (select_walk) as wave-uniform values: a few dozen scalar instructions once per wave.  The
// classes in countdown order, of byte offsets as tsel[] holds them; pairs and halves are held in vector registers -- a select between two of
// them is then one v_bfi_b32, where two scalar operands would cost a second instruction.  pool: LDS byte address of the tables.
__device__ __forceinline__ StepTables make_step_tables(const HuffImage& im, uint32_t pool)
{
    const auto of = [&](uint32_t q) { return ((uint32_t)im.k[q].tdc * 2) | ((uint32_t)im.k[q].tac * 2 << 16); };
    TableClasses c = make_countdown_classes(im.blocks_per_mcu, of);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c.pair[i] = HJ_UNIFORM(c.pair[i]);
        asm("" : "+v"(c.pair[i]));
    }
    c.bit0 = HJ_UNIFORM(c.bit0);
    c.bit1 = HJ_UNIFORM(c.bit1);
    StepTables s = split_classes(c, 1u, pool);  // (the classes hold byte offsets)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        asm("" : "+v"(s.dc[i]));
        asm("" : "+v"(s.ac[i]));
    }
    return s;
}

// The sync and position kernels' environment: a lane's row of the staged stream, the tables.
struct DevEnv : LdsTables {
    uint32_t stream_base;  // LDS byte address of the staged words
    uint32_t word0;        // image word index of the first word of staged row 0
    uint32_t row_addr;     // this lane's walk: LDS byte address of word 0 of its row ...
    uint32_t row_word0;    // ... and the image word index of that word (set_row)
    StepTables step;       // for huff_sync_kernel: the table selection as the select step takes it (make_step_tables)
    const uint32_t* boundaries;
    uint32_t num_boundaries;
    __device__ __forceinline__ uint32_t boundary(uint32_t i) const { return load_boundary(boundaries, num_boundaries, i); }
    static constexpr uint32_t kCursorStep = (uint32_t)kSyncThreads * 4u;  // consecutive words of a row, in bytes
    __device__ __forceinline__ void set_row(int row)
    {
        row_addr = stream_base + ((uint32_t)row << 2);
        row_word0 = word0 + ((uint32_t)row << kRowShift);
    }
    // row `row` staged in column `column` (huff_sync_pair_kernel: a lane's own column holds whatever row it decodes next)
    __device__ __forceinline__ void set_column_row(int column, int row)
    {
        row_addr = stream_base + ((uint32_t)column << 2);
        row_word0 = word0 + ((uint32_t)row << kRowShift);
    }
    __device__ __forceinline__ uint32_t cursor(uint32_t i) const { return row_addr + (i - row_word0) * kCursorStep; }
    __device__ __forceinline__ uint32_t fetch(uint32_t c) const { return *(const HJ_LDS uint32_t*)(uintptr_t)c; }
};

__device__ __forceinline__ uint32_t boundary0_of(const HuffImage& im, uint32_t subseq)
{
    return im.restart_interval ? ((const HJ_GLOBAL uint32_t*)im.sub_boundary)[subseq] : 0u;
}
// Block-start records (huffman_gpu_core.h) in global memory: fire-and-forget 16-bit stores from the walk's end-of-block branch.
// The records' base is uniform, the offset a 32-bit byte count (SGPR base + VGPR offset addressing).
struct SlotRecorder {
    HJ_GLOBAL char* records;  // the batch's records
    uint32_t off;             // byte offset of this subsequence's record
    uint32_t bit0;            // first bit of the subsequence
    // reports behind the last slot go to the scratch slot (the mark then says "overflow", or does not count them)
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t pos) const
    {
        *(HJ_GLOBAL uint16_t*)(records + (off + 2 * min(i, (uint32_t)kRecSlots))) = (uint16_t)(pos - bit0);
    }
};
// subsequence j of the image
__device__ __forceinline__ SlotRecorder slot_recorder(uint16_t* records, const HuffImage& im, uint32_t j)
{
    SlotRecorder r;
    r.records = (HJ_GLOBAL char*)records;
    r.off = (im.first_subseq + j) * (uint32_t)(2 * kRecShorts);
    r.bit0 = j * kSubseqBits;
    return r;
}
// the mark of the subsequence after a recording decode from (begin, z0) that ended in `st`
__device__ __forceinline__ void put_mark(const SlotRecorder& r, uint32_t begin, uint32_t limit, uint32_t total_bits, uint32_t z0, const SubseqState& st)
{
    *(HJ_GLOBAL uint16_t*)(r.records + (r.off + 2 * kRecMark)) = (uint16_t)record_mark(begin, min(limit, total_bits), z0, st);
}

// The environment of the select step (select_walk): the tables of an MCU position from registers -- four classes, or at most two --
// as LDS addresses with the pool's base inside, so that a lookup adds nothing but the window's index.
template <bool FOUR>
struct StepEnv : DevEnv {
    __device__ __forceinline__ explicit StepEnv(const DevEnv& e) : DevEnv(e) {}
    __device__ __forceinline__ void step_tables(uint32_t d, uint32_t* tdc, uint32_t* tac) const { select_halves<FOUR>(step, d, tdc, tac); }
    __device__ __forceinline__ uint32_t step_entry(uint32_t t, uint32_t w) const { return *(const HJ_LDS uint16_t*)(uintptr_t)(t + index1(w)); }
    __device__ __forceinline__ uint32_t step_pair(uint32_t t, uint32_t w) const  // the same address + a constant
    {
        return *(const HJ_LDS uint16_t*)(uintptr_t)(t + 2 * kPairOffset + index1(w));
    }
    __device__ __forceinline__ uint32_t step_second(uint32_t e) const { return second_table_of(e, 7u, pool); }  // / 64 entries -> bytes
};
// huff_sync_kernel's walk: the select form, with or without restart handling (a wave-uniform choice: one image per workgroup), with
// or without records (uniform too; never across restart boundaries).  The everyday scan's two table classes get the short
// selection (uniform as well).
__device__ __forceinline__ SubseqState sync_walk(bool rst, bool record, const HuffGeom& geom, const DevEnv& env, uint32_t begin, uint32_t limit, int z, int k,
                                                 uint32_t boundary0, const SlotRecorder& rec)
{
    const auto walk = [&](const auto& senv) {
        if (rst) return select_walk<true>(geom, senv, begin, limit, z, k, boundary0);
        return record ? select_walk<false>(geom, senv, begin, limit, z, k, 0, rec) : select_walk<false>(geom, senv, begin, limit, z, k);
    };
    if (env.step.bit1 == 0) return walk(StepEnv<false>(env));
    return walk(StepEnv<true>(env));
}

// Staging of stream words: lane t brings subsequence `row` of the image (-1: filled with ones) and the kStagedExtra words behind
// it into column t of the transposed rows (see WgShared).  16-byte global loads, all of a lane's loads in flight together; words
// behind the end of the stream read as ones.  stage_rows: the cooperative form, lane t takes row first_row + t.
template <int ROWS>
__device__ __forceinline__ void stage_row(uint32_t* lds_stream, const HuffImage& im, int row)
{
    const int t = threadIdx.x;
    const HJ_GLOBAL uint32_t* g = (const HJ_GLOBAL uint32_t*)im.stream;
    const int nwords = (int)im.stream_words;
    const int w0 = row * kSubseqWords;
    constexpr int kGroups = kSubseqWords / 4;  // 16-byte groups per row; the look-ahead words are one 8-byte group more
    u32x4 v[kGroups];
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 tail;
    {
        const int gd = w0 + kSubseqWords;
        const int gc = min(max(gd, 0), (nwords - 1) & ~1);
        const u32x2 x = *(const HJ_GLOBAL u32x2*)(g + gc);
        tail = (gd >= 0 && gd < nwords) ? x : u32x2{~0u, ~0u};
    }
#pragma unroll
    for (int i = 0; i < kGroups; i++) {
        const int gd = w0 + i * 4;
        // streams are allocated in whole 64-byte units: a 16-byte group that starts inside the stream is readable.  The
        // load itself is unconditional (clamped address) so that all of them are in flight together.
        const int gc = min(max(gd, 0), (nwords - 1) & ~3);
        const u32x4 x = *(const HJ_GLOBAL u32x4*)(g + gc);
        v[i] = (gd >= 0 && gd < nwords) ? x : u32x4{~0u, ~0u, ~0u, ~0u};
    }
    HJ_LDS uint32_t* dst = (HJ_LDS uint32_t*)lds_stream + t;
#pragma unroll
    for (int i = 0; i < kGroups; i++) {
        dst[(4 * i + 0) * ROWS] = __builtin_bswap32(v[i].x);
        dst[(4 * i + 1) * ROWS] = __builtin_bswap32(v[i].y);
        dst[(4 * i + 2) * ROWS] = __builtin_bswap32(v[i].z);
        dst[(4 * i + 3) * ROWS] = __builtin_bswap32(v[i].w);
    }
    dst[(kSubseqWords + 0) * ROWS] = __builtin_bswap32(tail.x);
    dst[(kSubseqWords + 1) * ROWS] = __builtin_bswap32(tail.y);
}
template <int ROWS>
__device__ __forceinline__ void stage_rows(uint32_t* lds_stream, const HuffImage& im, int first_row)
{
    stage_row<ROWS>(lds_stream, im, first_row + (int)threadIdx.x);
}

// lookup tables -> LDS
template <int THREADS>
__device__ __forceinline__ void stage_pool(HJ_LDS uint16_t* pool, const HuffImage& im)
{
    const HJ_GLOBAL u32x4* gp = (const HJ_GLOBAL u32x4*)im.pool;
    const uint32_t npool = im.pool_words >> 3;  // pool_words is a multiple of 64
    for (uint32_t i = threadIdx.x; i < npool; i += THREADS) {
        const u32x4 x = gp[i];
        HJ_LDS uint32_t* lp = reinterpret_cast<HJ_LDS uint32_t*>(pool) + i * 4;
        lp[0] = x.x;
        lp[1] = x.y;
        lp[2] = x.z;
        lp[3] = x.w;
    }
}

// per-MCU-position constants and the zigzag permutation -> LDS (needs >= 80 lanes).  zzw (the block pass alone) takes the permutation as
// byte offsets into a block of int16: 2 * index, still a byte each (<= 126).
__device__ __forceinline__ void stage_constants(uint32_t* tsel, KSlot* kslot, uint32_t* zzw, const HuffImage& im, bool with_addresses)
{
    const int t = threadIdx.x;
    if (t < 10) {
        const HuffK hk = im.k[t];
        tsel[t] = ((uint32_t)hk.tdc * 2) | ((uint32_t)hk.tac * 2 << 16);  // byte offsets (<= 2 * kMaxPoolWords < 65536)
        if (with_addresses) {
            KSlot s;
            s.base = im.coef[hk.comp & 3] + (size_t)hk.blk0 * 64;
            s.stride_y = hk.stride_y;
            s.stride_x = hk.stride_x;
            kslot[t] = s;
        }
    }
    if (zzw && t >= 64 && t < 80) {
        constexpr uint8_t zz[64] = HJ_ZIGZAG_DEVICE_TABLE;
        const int i = (t - 64) * 4;
        zzw[t - 64] = ((uint32_t)zz[i] | ((uint32_t)zz[i + 1] << 8) | ((uint32_t)zz[i + 2] << 16) | ((uint32_t)zz[i + 3] << 24)) << 1;
    }
}

template <class Shared>
__device__ __forceinline__ DevEnv make_env(Shared& sh, HJ_LDS uint16_t* pool, uint32_t first, const HuffGeom& geom, const HuffImage& im)
{
    DevEnv env;
    env.stream_base = (uint32_t)(uintptr_t)(HJ_LDS uint32_t*)sh.stream;
    env.word0 = (first - 1) * kSubseqWords;  // row 0 = the halo (wraps for the first workgroup of an image; so do the indices)
    env.row_addr = env.stream_base;
    env.row_word0 = env.word0;
    env.pool = (uint32_t)(uintptr_t)pool;
    env.tsel = (const HJ_LDS uint32_t*)sh.tsel;
    // (huff_pos_kernel never takes the select step, but the compiler keeps some ninety scalar instructions of the class builder in
    // it: the tables move out of that kernel together with a change that is allowed to move its code;
    // profiles/walk_two_forms/README.md)
    env.step = make_step_tables(im, env.pool);
    env.boundaries = geom.boundaries;
    env.num_boundaries = geom.num_boundaries;
    return env;
}

// Packs the lanes with has == true to the front: returns how many there are; *task = value of the t-th of them for the
// lanes t below that count, -1 for the others.  Contains barriers: call from uniform control flow.
template <class Shared>
__device__ __forceinline__ int compact_tasks(Shared& sh, bool has, int value, int* task)
{
    const int t = threadIdx.x;
    const unsigned long long mask = __ballot(has);
    const int below = __popcll(mask & ((1ull << (t & 63)) - 1));
    if ((t & 63) == 0) sh.wave_count[t >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    int base = 0, n = 0;
#pragma unroll
    for (int w = 0; w < kSyncThreads / 64; w++) {
        const int c = (int)sh.wave_count[w];
        if (w < (t >> 6)) base += c;
        n += c;
    }
    if (has) sh.queue[base + below] = (std::remove_reference_t<decltype(sh.queue[0])>)value;
    __syncthreads();
    *task = t < n ? (int)sh.queue[t] : -1;
    return n;
}

// ---- zero-copy input: bitstreams fetched from the caller's pinned host memory ------------------------------------------------
// One DMA call per image costs the submitting thread 15-20 us (256 of them: 5 ms per batch, measured); one kernel that pulls the bytes
// over PCIe costs one launch.  Few resident workgroups on purpose -- waves that wait on PCIe reads slow the kernels beside them as
// long as they occupy wave slots -- each walking the destuff kernels' chunk list (kDestuffChunk raw bytes per item).
constexpr int kGatherGroups = 64;
__global__ __launch_bounds__(kThreads) void gather_raw_kernel(const HuffImage* __restrict__ images, const HuffUnit* __restrict__ units, int nunits)
{
    for (int ui = blockIdx.x; ui < nunits; ui += gridDim.x) {
        const HuffUnit u = units[ui];
        const HuffImage& im = images[u.image];
        const uint8_t* src = im.raw_src;
        if (!src) continue;  // staged by the host (uniform per item)
        const uint32_t begin = u.first * (uint32_t)kDestuffChunk;
        if (begin >= im.raw_bytes) continue;
        const uint32_t n = min((uint32_t)kDestuffChunk, im.raw_bytes - begin);
        const uint8_t* s = src + begin;
        uint8_t* d = const_cast<uint8_t*>(im.raw) + begin;  // 16-byte aligned: raw offsets and kDestuffChunk are multiples of 16
        typedef u32x4 __attribute__((aligned(1))) u32x4_unaligned;  // the caller's buffer starts at any byte
        for (uint32_t i = threadIdx.x * 16u; i + 16u <= n; i += kThreads * 16u) *(HJ_GLOBAL u32x4*)(d + i) = *(const HJ_GLOBAL u32x4_unaligned*)(s + i);
        const uint32_t tail = n & ~15u;
        if (threadIdx.x < (n & 15u)) d[tail + threadIdx.x] = s[tail + threadIdx.x];
    }
}

// ---- byte-stuffing removal ------------------------------------------------------------------------------------------
// The file's entropy-coded segment escapes every 0xFF data byte as FF 00.  Two kernels turn it into the plain bitstream the
// decoders read: the first counts the stuffed bytes of every 16 KB chunk, the second compacts each chunk to its final
// position (chunk offset minus the stuffed bytes before it) through LDS.  Fill bytes (FF FF) never get here (gpu_entropy_eligible()).
// Restart markers do, in images with a restart interval and only there: the parser notes every FF D0..D7 of a scan (ScanWalk::visit,
// rst_after), and a scan whose markers are not exactly the ones its restart interval calls for -- none without an interval -- is not
// eligible.  So an image without a restart interval has nothing but FF 00 to drop, which is what the parser counted for it
// (ScanHeader::chunk_drops), and its chunks take the mask of the stuffed zeros alone: one byte test per word instead of five.

__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu); }  // 0x80 per zero byte

// 0x80 in every byte of x (little-endian dword) that is 0x00 and whose predecessor byte is 0xFF; prev = the byte in front of x.
// (A byte is 0x00 behind 0xFF exactly where "the byte, or its predecessor's complement" is zero: one byte test for both conditions.)
__device__ __forceinline__ uint32_t stuffed_zero_mask(uint32_t x, uint32_t prev) { return zero_bytes(x | ~((x << 8) | prev)); }

// 0x80 in both bytes of every restart marker FF D0..D7 that has a byte in x; prev = the byte in front of x, next = the byte behind it.
__device__ __forceinline__ uint32_t marker_mask(uint32_t x, uint32_t prev, uint32_t next)
{
    const uint32_t ff_x = zero_bytes(~x);                                // x's byte is 0xFF
    const uint32_t rst_x = zero_bytes((x & 0xF8F8F8F8u) ^ 0xD0D0D0D0u);  // x's byte is D0..D7
    const uint32_t ff_before = (ff_x << 8) | (prev == 0xFFu ? 0x80u : 0u);
    const uint32_t after = (x >> 8) | (next << 24);                      // successor of each byte
    return (rst_x & ff_before) | (ff_x & zero_bytes((after & 0xF8F8F8F8u) ^ 0xD0D0D0D0u));
}

// Bytes of x to drop: a 0x00 behind an 0xFF (stuffing) and, with `markers` (images with a restart interval), both bytes of a restart
// marker.
__device__ __forceinline__ uint32_t stuffed_mask(uint32_t x, uint32_t prev, uint32_t next, bool markers)
{
    const uint32_t d = stuffed_zero_mask(x, prev);
    return markers ? d | marker_mask(x, prev, next) : d;
}

// stuffed-byte masks of the 64 bytes at p (16-byte aligned); returns the count
__device__ __forceinline__ uint32_t lane_masks(const uint8_t* p, bool has_prev, bool markers, uint32_t m[16], uint32_t x[16])
{
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint32_t prev = has_prev ? p[-1] : 0u;
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint4 v = q[i];
        x[4 * i + 0] = v.x;
        x[4 * i + 1] = v.y;
        x[4 * i + 2] = v.z;
        x[4 * i + 3] = v.w;
    }
    const uint32_t behind = p[64];  // the raw copy is padded with 16 neutral bytes: always readable
#pragma unroll
    for (int i = 0; i < 16; i++) {
        m[i] = stuffed_mask(x[i], prev, i < 15 ? (x[i < 15 ? i + 1 : 15] & 0xFFu) : behind, markers);
        prev = x[i] >> 24;
        n += __popc(m[i]);
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

// unit.first = chunk index inside the image; drops[im.first_chunk + chunk] = stuffed bytes in the chunk
__global__ __launch_bounds__(kThreads) void destuff_count_kernel(const HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                                 uint32_t* __restrict__ drops)
{
    __shared__ uint32_t scratch[4];
    const HuffUnit u = units[blockIdx.x];
    const HuffImage& im = images[u.image];
    const uint32_t off = u.first * kDestuffChunk + threadIdx.x * 64;
    const bool markers = im.restart_interval != 0;  // (the compact kernel's rule)
    uint32_t n = 0;
    if (off < im.raw_bytes) {  // the raw copy is padded to 16 bytes with a neutral value; whole 16-byte pieces are readable
        uint32_t m[16], x[16];
        const uint32_t pieces = min(4u, (im.raw_bytes - off + 15) / 16);
        if (pieces == 4) {
            n = lane_masks(im.raw + off, off > 0, markers, m, x);
        } else {
            uint32_t prev = off > 0 ? im.raw[off - 1] : 0u;
            const uint32_t* words = reinterpret_cast<const uint32_t*>(im.raw + off);  // 16 neutral bytes of padding follow the data
            for (uint32_t i = 0; i < pieces * 4; i++) {
                const uint32_t w = words[i];
                n += __popc(stuffed_mask(w, prev, words[i + 1] & 0xFFu, markers));
                prev = w >> 24;
            }
        }
    }
    const uint32_t total = wg_sum(n, scratch);
    if (threadIdx.x == 0) drops[im.first_chunk + u.first] = total;
}

// (256 x 1080p: 94 us for 2,048 chunks, eight resident per CU.  The time is the chunks' work, not their number: two chunks per workgroup 147 us,
// four 149.  Per CU and launch the LDS pipeline was busy 33 us -- 64 single-byte stores per lane then -- and the vector ALUs 20.  With the
// loads in flight together 70 us; with the compaction in dwords 68, six resident per CU: profiles/entropy_residue/.  That version
// issued 1,544 vector instructions per lane, which is what its time was.  With the mask of the stuffed zeros alone for images
// without a restart interval, one byte permute for the squeeze and a one-register accumulator about 900 of 1,172 run: 51 us, 61
// registers, eight resident per CU: profiles/entropy_residue2/.)
__global__ __launch_bounds__(kThreads) void destuff_compact_kernel(HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                                   const uint32_t* __restrict__ drops, unsigned int* __restrict__ counters)
{
    // the stage's convergence counters (64 words) start at zero: cleared here, by the first kernel of the stage, instead of by a
    // fill kernel of their own in front of it
    if (blockIdx.x == 0 && threadIdx.x < 64 && counters) counters[threadIdx.x] = 0u;
    __shared__ uint32_t scratch[4];
    __shared__ uint32_t wave_base[4];
    // One LDS buffer, twice: first the raw chunk (loaded as consecutive dwords: whole lines per wave), then the compacted image.  Both are
    // PADDED by a dword per 64 bytes -- dword g sits at g + (g >> 4), byte k at k + (k >> 6 << 2): a lane owns 64 consecutive bytes, its
    // neighbour the next 64, and without the padding the lanes of a wave would all hit the same two banks (round 2's version did: 55 % of
    // its LDS cycles were bank conflicts, and its global loads touched 64 lines per instruction).
    __shared__ uint32_t buf[kDestuffChunk / 4 + kDestuffChunk / 64 + 8];
    // squeeze_sel[m]: the byte selector (v_perm_b32) that takes the bytes whose bit is set in m out of a word, packs the others to the
    // bottom and puts zeros above them (selector byte 0x0C)
    __shared__ uint32_t squeeze_sel[16];
    HJ_LDS uint8_t* bytes = (HJ_LDS uint8_t*)buf;
    const HuffUnit u = units[blockIdx.x];
    HuffImage& im = images[u.image];
    const int t = threadIdx.x;
    if (t < 16) {
        uint32_t sel = 0x0C0C0C0Cu, j = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (!((uint32_t)t >> b & 1u)) {
                sel = (sel & ~(0xFFu << (8 * j))) | (b << (8 * j));
                j++;
            }
        squeeze_sel[t] = sel;
    }
    const uint32_t raw_bytes = im.raw_bytes;
    const bool markers = im.restart_interval != 0;  // workgroup-uniform: see the comment above zero_bytes()
    // stuffed bytes in the chunks before this one
    uint32_t before = 0;
    for (uint32_t c = t; c < u.first; c += kThreads) before += drops[im.first_chunk + c];
    before = wg_sum(before, scratch);
    const uint32_t chunk_begin = u.first * kDestuffChunk;
    const uint32_t chunk_len = min((uint32_t)kDestuffChunk, raw_bytes - chunk_begin);
    const uint32_t gout = chunk_begin - before;  // destination offset of the chunk's first kept byte
    const uint32_t a = gout & 3;                 // the LDS image shares the destination's misalignment

    // raw chunk -> LDS (the raw copy is padded to 16 bytes with a neutral value and 16 more: whole 16-byte pieces are readable)
    // The loads go out unconditionally from clamped indices, all of a lane's four in flight together, and the pieces behind the
    // chunk's end are replaced afterwards (a test around each load made every one of them wait for its own latency).
    {
        const uint32_t pieces = (chunk_len + 15) / 16;  // chunk_len >= 1: 16-byte pieces, at raw offsets that are multiples of 16
        const HJ_GLOBAL u32x4* src = (const HJ_GLOBAL u32x4*)(im.raw + chunk_begin);
        constexpr uint32_t kPiecesPerLane = kDestuffChunk / 16 / kThreads;
        u32x4 v[kPiecesPerLane];
#pragma unroll
        for (uint32_t i = 0; i < kPiecesPerLane; i++) v[i] = src[min(i * kThreads + t, pieces - 1)];
#pragma unroll
        for (uint32_t i = 0; i < kPiecesPerLane; i++) {
            const uint32_t q = i * kThreads + t, g = q * 4 + (q >> 2);  // dwords 4q .. 4q + 3 share their padding
            const u32x4 x = q < pieces ? v[i] : u32x4{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
            buf[g] = x.x;
            buf[g + 1] = x.y;
            buf[g + 2] = x.z;
            buf[g + 3] = x.w;
        }
    }
    const uint32_t before_chunk = chunk_begin > 0 ? im.raw[chunk_begin - 1] : 0u;                    // (lane 0's predecessor byte)
    const uint32_t behind_chunk = chunk_len == (uint32_t)kDestuffChunk ? im.raw[chunk_begin + kDestuffChunk] : 0x01u;  // (lane 255's successor)
    __syncthreads();

    const uint32_t off = chunk_begin + t * 64;
    // The lane's 64 bytes, word by word: the mask of the bytes to drop, their count, and the word SQUEEZED -- its dropped bytes taken
    // out, the kept ones packed to the bottom, zeros above them: one byte permute, its selector looked up by the mask's four bits -- with
    // eight times the number of dropped bytes (bits of a shift) in six bits of `gone`.  One code path for words with and without
    // drops.  The stream's last lane squeezes the neutral bytes behind the stream's end like data: they land behind the last kept byte,
    // inside the buffer (a lane never stores more than its 64 bytes), where no lane has bytes of its own and the copy-out, which goes
    // by the counts, does not look.
    uint32_t x[16];
    uint32_t gone[4] = {0, 0, 0, 0};  // five words each
    uint32_t n = 0, len = 0;
    if (off < raw_bytes) {
        len = min(64u, raw_bytes - off);
        const uint32_t pieces = (len + 15) / 16;
        const uint32_t before_lane = t > 0 ? buf[(t - 1) * 17 + 15] >> 24 : before_chunk;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) x[i] = i < pieces * 4 ? buf[t * 17 + i] : 0x01010101u;
        uint32_t d[16];
        uint32_t prev = before_lane;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            d[i] = stuffed_zero_mask(x[i], prev);
            prev = x[i] >> 24;
        }
        if (markers) {
            const uint32_t behind = pieces == 4 ? (t < kThreads - 1 ? buf[(t + 1) * 17] & 0xFFu : behind_chunk) : 0x01u;
            prev = before_lane;
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                d[i] |= marker_mask(x[i], prev, i < 15 ? (x[i < 15 ? i + 1 : 15] & 0xFFu) : behind);
                prev = x[i] >> 24;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t p = __popc(d[i]);
            n += p;
            gone[i / 5] |= p << (6 * (i % 5) + 3);
            // the mask's bytes are 0x80 or 0: their dot product with (1, 2, 4, 8) is 0x80 times the four bits as a number
            const uint32_t m = __builtin_amdgcn_udot4(d[i], 0x08040201u, 0u, false) >> 7;
            x[i] = __builtin_amdgcn_perm(x[i], x[i], squeeze_sel[m]);
        }
    }
    // exclusive scan of the per-lane counts: inside the wave by shuffles, across the four waves through LDS
    uint32_t incl = n;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d);
        if ((t & 63) >= d) incl += v;
    }
    if ((t & 63) == 63) wave_base[t >> 6] = incl;
    __syncthreads();  // (every lane holds its 64 bytes in registers from here on: the buffer is free for the compacted image)
    uint32_t excl = incl - n;
    for (int w = 0; w < (t >> 6); w++) excl += wave_base[w];
    const uint32_t chunk_drops = wave_base[0] + wave_base[1] + wave_base[2] + wave_base[3];
    // Kept bytes of this lane -> LDS, as aligned dwords: the squeezed words are appended to a register accumulator, which gives off a
    // dword whenever it holds four bytes.  A lane's first dword can begin with the last bytes of the lanes in front: it goes out with
    // zeros there.  What the accumulator holds at the end, fewer than four bytes, is stored byte by byte behind a barrier, into the dword
    // that the next lane to fill one has written by then.  No two lanes store the same dword: a lane gives off a dword only once it is
    // full, and the lanes in front of it have left that one to their byte stores.
    auto padded = [](uint32_t k) { return k + ((k >> 6) << 2); };
    const uint32_t o0 = a + t * 64 - excl, cnt0 = o0 & 3;
    // (The accumulator is one register: below its cnt < 4 bytes nothing is set, so a word shifted up by cnt bytes fills it and leaves
    // its own top bytes for the next dword.  Only the store depends on whether the dword is full; the rest are selects.)
    uint32_t slot = o0 >> 2, bits = 8 * cnt0, acc = 0;  // bits: eight times the bytes the accumulator holds
    if (len) {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const unsigned long long w = (unsigned long long)x[i] << bits;
            const uint32_t p = (gone[i / 5] >> (6 * (i % 5))) & 63u;
            const bool full = bits >= p;  // bits / 8 + (4 - p / 8) kept bytes make a dword
            acc |= (uint32_t)w;
            if (full) buf[slot + (slot >> 4)] = acc;
            acc = full ? (uint32_t)(w >> 32) : acc;
            slot += full ? 1u : 0u;
            bits = (bits - p) & 24u;
        }
    }
    const uint32_t o = slot * 4, cnt = bits / 8;
    __syncthreads();
    {  // what the accumulator still holds (in front of it the neighbours' bytes, if the lane never filled a dword)
        const uint32_t from = slot == (o0 >> 2) ? cnt0 : 0u;
#pragma unroll
        for (uint32_t b = 0; b < 3; b++)
            if (b >= from && b < cnt) bytes[padded(o + b)] = (uint8_t)((uint32_t)acc >> (8 * b));
    }
    __syncthreads();
    // LDS -> destination: whole dwords in the middle, single bytes at the ragged ends (neighbouring chunks share those dwords)
    const uint32_t n_out = chunk_len - chunk_drops;
    uint8_t* dst = const_cast<uint8_t*>(im.stream) + (gout - a);  // 4-byte aligned
    const uint32_t first_full = a ? 1 : 0, end_full = (a + n_out) / 4;
    for (uint32_t d = first_full + t; d < end_full; d += kThreads) reinterpret_cast<uint32_t*>(dst)[d] = buf[d + (d >> 4)];
    if (t < 4) {
        if (a && (uint32_t)t >= a && (uint32_t)t < a + n_out) dst[t] = bytes[padded((uint32_t)t)];  // head
        const uint32_t tail = max(end_full, first_full) * 4 + t;
        if (tail >= a && tail < a + n_out && tail >= 4 * first_full) dst[tail] = bytes[padded(tail)];
    }
    // the last chunk knows the destuffed length: publish it and lay down the 0xFF slack behind the data
    if (chunk_begin + chunk_len == raw_bytes) {
        const uint32_t total = raw_bytes - before - chunk_drops;
        const uint32_t padded = ((total + 3) & ~3u) + kStreamSlackBytes;
        uint8_t* s = const_cast<uint8_t*>(im.stream);
        if (total + t < padded) s[total + t] = 0xFF;
        if (t == 0) {
            im.total_bits = total * 8;
            im.num_subseq = (total * 8 + kSubseqBits - 1) / kSubseqBits;
            im.stream_words = padded / 4;
        }
    }
}

// states[]: one 8-byte record per subsequence (batch-wide indexing through HuffImage::first_subseq).
// incoming[]: per sync unit, the state it was entered with the last time it ran.
// counters[0] += 1 for every workgroup whose outgoing state (end state of its last subsequence) differs from the published
// one; counters[2..5] = statistics (2, 3: the first launch, huff_sync_pair_kernel below; 4, 5: the later ones).
//
// The ripple over single units as a sync-kernel launch (HIPJPEG_RIPPLE_IN_SYNC=1, an A/B aid: the launches behind the first are
// huff_tail_kernel<true>'s otherwise).  A workgroup whose incoming state still equals the one it was entered with has nothing to do
// and leaves before staging anything; otherwise the ripple starts from its first subsequence: a subsequence whose predecessor's end
// state differs from the one it was decoded from is decoded again, to the workgroup's fixpoint.  Every round packs the subsequences to
// redo into the lowest lanes.
__global__ __launch_bounds__(kSyncThreads) void huff_sync_kernel(const HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                             unsigned long long* __restrict__ states, unsigned long long* __restrict__ incoming,
                                                             unsigned int* __restrict__ counters, uint16_t* records)
{
    __shared__ WgShared sh;
    extern __shared__ uint16_t dyn_pool[];
    HJ_LDS uint16_t* pool = (HJ_LDS uint16_t*)dyn_pool;
    const HuffUnit u = units[blockIdx.x];
    const HuffImage& im = images[u.image];
    const HuffGeom geom = make_geom(im);
    const uint32_t nsub = (geom.total_bits + kSubseqBits - 1) / kSubseqBits;
    if (u.first >= nsub) return;  // uniform: the stream turned out shorter than planned
    unsigned long long* gstate = states + im.first_subseq;
    const int t = threadIdx.x;
    const uint32_t j = u.first - 1 + t;  // subsequence of lane t (lane 0: the halo; none for the first workgroup of an image)
    const bool owner = t >= 1 && j < nsub;
    const int n_rows = (int)min((uint32_t)kSyncThreads, nsub - u.first + 1);  // rows 1 .. n_rows-1 are owned
    const unsigned long long in_state = u.first ? __hip_atomic_load(&gstate[u.first - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kSyncMask : 0ull;
    if (in_state == incoming[blockIdx.x]) return;  // uniform
    stage_rows<kSyncThreads>(sh.stream, im, (int)u.first - 1);
    stage_pool<kSyncThreads>(pool, im);
    stage_constants(sh.tsel, nullptr, nullptr, im, false);
    __syncthreads();

    DevEnv env = make_env(sh, pool, u.first, geom, im);
    const bool rst = im.restart_interval != 0;
    // block-start records: every correction decode takes them (not across restart boundaries)
    const bool recording = !rst;
    const unsigned long long old_global = owner ? gstate[j] : ~0ull;
    sh.end[t] = t == 0 ? in_state : old_global;
    int task = t == 1 ? 1 : -1;
    int rounds = 0;
    for (int round = 0; round < kSyncThreads + 2; round++) {
        __syncthreads();
        rounds++;
        unsigned long long now = 0;
        bool moved = false;
        if (task >= 0) {
            const SubseqState p = unpack_state(sh.end[task - 1]);
            env.set_row(task);  // the predecessor's walk ended on a symbol that starts in this row
            const uint32_t jt = u.first - 1 + task;
            const SlotRecorder rec = slot_recorder(records, im, jt);
            const SubseqState st = sync_walk(rst, recording, geom, env, p.end_bit, (jt + 1) * kSubseqBits, p.zk & 255, p.zk >> 8, boundary0_of(im, jt), rec);
            if (recording) put_mark(rec, p.end_bit, (jt + 1) * kSubseqBits, geom.total_bits, p.zk & 255, st);
            now = pack_state(st);
            moved = ((now ^ sh.end[task]) & kSyncMask) != 0;
        }
        __syncthreads();  // every start state has been read before any end state is replaced
        if (task >= 0) sh.end[task] = now;
        if (compact_tasks(sh, moved && task + 1 < n_rows, task + 1, &task) == 0) break;
    }
    __syncthreads();
    if (owner) {
        const unsigned long long mine = sh.end[t];
        if (mine != old_global) {
            __hip_atomic_store(&gstate[j], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t == n_rows - 1 && ((mine ^ old_global) & kSyncMask) != 0) atomicAdd(counters + 0, 1u);
        }
    }
    if (t == 0) {
        incoming[blockIdx.x] = in_state;
        // statistics: correction rounds (sum, maximum) of the later launches
        atomicAdd(counters + 4, (unsigned)rounds);
        atomicMax(counters + 5, (unsigned)rounds);
    }
}

// The first launch in pairs: a workgroup takes TWO consecutive sync units of one image (pairs[]: index of the first, bit 31 = there
// is a second), kPairRows local rows, and decodes them in a schedule that wastes less than "everything from a guess, then everything
// again" (1 + 1 + 0.36 walks per bit): only the EVEN rows start from the assumed state, the odd rows wait for them.
//   phase A  even rows (the halo is row 0) from the assumed state, no records             0.5 of the bits
//   phase B  odd rows from A's end state of the row in front (1,024 bits of history: right two times in three), records   0.5
//   round 1  even rows but the halo, from B's end states, records                         0.5
//   round 2  odd rows whose start state moved in round 1                                  ~0.18
//   ...      successors of the rows that moved, the parity alternating; tasks packed into the lowest lanes
// The staged rows hold what the lanes are about to decode: lane t stages the row of its task into column t itself, so nothing but a
// lane's own program order stands between staging and walking, and a round with few tasks stages few rows.  A and B are one lane's
// two rows one after the other: no barrier between them either.
// In the first workgroup of an image row 0 does not exist: row 1 (subsequence 0) is decoded in B from the exact initial state.
// What the kernel leaves is per UNIT, as huff_sync_kernel leaves it: states[], the task lists and counts (local rows of the unit),
// incoming[].  The second unit's incoming[] is the state its first subsequence (row kSyncThreads here) was last decoded from: where the
// row in front moved after that, the tail kernel sees a state in front that is not incoming[] and decodes the subsequence again --
// that row is therefore never put on the list.  So when the kernel ends every subsequence was last decoded from the state now in
// front of it, or is on its unit's list, or its unit's incoming[] differs from the state in front.
// max_rounds counts the correction rounds (B is none); tail_count == nullptr: the rounds run to the workgroup's fixpoint.
__global__ __launch_bounds__(kSyncThreads) void huff_sync_pair_kernel(const HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                                  const uint32_t* __restrict__ pairs, unsigned long long* __restrict__ states,
                                                                  unsigned long long* __restrict__ incoming, unsigned int* __restrict__ counters,
                                                                  int max_rounds, uint16_t* __restrict__ tail_tasks, uint32_t* __restrict__ tail_count,
                                                                  uint16_t* records)
{
    __shared__ PairShared sh;
    extern __shared__ uint16_t dyn_pool[];
    HJ_LDS uint16_t* pool = (HJ_LDS uint16_t*)dyn_pool;
    const uint32_t pair = pairs[blockIdx.x];
    const uint32_t ui = pair & 0x7FFFFFFFu;
    const HuffUnit u = units[ui];
    const HuffImage& im = images[u.image];
    const HuffGeom geom = make_geom(im);
    const uint32_t nsub = (geom.total_bits + kSubseqBits - 1) / kSubseqBits;
    if (u.first >= nsub) return;  // uniform: the stream turned out shorter than planned
    unsigned long long* gstate = states + im.first_subseq;
    const int t = threadIdx.x;
    const int n_rows = (int)min((uint32_t)((pair >> 31) ? kPairRows : kSyncThreads), nsub - u.first + 1);  // rows 1 .. n_rows-1 are owned
    const bool second = n_rows > kSyncThreads;  // the second unit owns rows (its first subsequence lies inside the stream)
    const auto subseq_of = [&](int row) { return u.first - 1 + (uint32_t)row; };
    const bool in_a = 2 * t < n_rows && (t > 0 || u.first > 0);
    if (in_a) stage_row<kSyncThreads>(sh.stream, im, (int)subseq_of(2 * t));
    stage_pool<kSyncThreads>(pool, im);
    stage_constants(sh.tsel, nullptr, nullptr, im, false);
    __syncthreads();

    DevEnv env = make_env(sh, pool, u.first, geom, im);
    const bool rst = im.restart_interval != 0;
    const bool recording = !rst;  // block-start records: every decode but A's takes them (not across restart boundaries)
    const auto decode = [&](int row, unsigned long long from, bool record) {
        const SubseqState p = unpack_state(from);
        const uint32_t jt = subseq_of(row);
        env.set_column_row(t, row);
        const SlotRecorder rec = slot_recorder(records, im, jt);
        const SubseqState st = sync_walk(rst, record, geom, env, p.end_bit, (jt + 1) * kSubseqBits, p.zk & 255, p.zk >> 8, boundary0_of(im, jt), rec);
        if (record) put_mark(rec, p.end_bit, (jt + 1) * kSubseqBits, geom.total_bits, p.zk & 255, st);
        return pack_state(st);
    };
    // A, then B: rows 2t and 2t + 1
    unsigned long long mine = 0;  // first workgroup of an image, row 0: the exact initial state (bit 0, z 0, k 0)
#pragma unroll 1
    for (int ph = 0; ph < 2; ph++) {
        const int row = 2 * t + ph;
        const bool active = ph ? row < n_rows : in_a;
        if (active) {
            if (ph) stage_row<kSyncThreads>(sh.stream, im, (int)subseq_of(row));
            const unsigned long long from = ph ? mine : (unsigned long long)subseq_of(row) * kSubseqBits;
            if (row == kSyncThreads) sh.second_from = from & kSyncMask;
            mine = decode(row, from, ph && recording);
        }
        if (active || row == 0) sh.end[row] = mine;
    }
    __syncthreads();
    // Round 1: a wrong guess is decoded again.  With records, so is every other even row: A records nothing, and the rows that
    // guessed right (about one in 300) are decoded again from the same state, record, and stop there.
    int task = -1;
    if (t >= 1 && 2 * t < n_rows && (recording || (sh.end[2 * t - 1] & kSyncMask) != (unsigned long long)subseq_of(2 * t) * kSubseqBits)) task = 2 * t;
    int rounds = 0, pending = 0;
    for (int round = 0; round < kPairRows + 2; round++) {
        rounds++;
        bool moved = false;
        if (task >= 0) {
            stage_row<kSyncThreads>(sh.stream, im, (int)subseq_of(task));
            const unsigned long long from = sh.end[task - 1];
            if (task == kSyncThreads) sh.second_from = from & kSyncMask;
            const unsigned long long now = decode(task, from, recording);
            moved = ((now ^ sh.end[task]) & kSyncMask) != 0;
            // (a round's rows are of one parity: nobody reads this entry as a start state before the barriers of compact_tasks)
            sh.end[task] = now;
        }
        pending = compact_tasks(sh, moved && task + 1 < n_rows, task + 1, &task);
        if (pending == 0 || rounds >= max_rounds) break;
    }
    // what is left goes to the tail kernel, unit by unit.  The rows ascend with the lanes (compact_tasks keeps the order, a round's
    // tasks are the successors of the round before): the first unit's tasks are the lowest lanes'.
    if (tail_count) {
        const int n_first = __syncthreads_count(task >= 0 && task < kSyncThreads);
        const int skip = n_first < pending && sh.queue[n_first] == kSyncThreads ? 1 : 0;  // the second unit's first row: incoming[] says it
        if (task >= 0 && task < kSyncThreads) tail_tasks[(size_t)ui * kSyncThreads + t] = (uint16_t)task;
        if (task > kSyncThreads) tail_tasks[(size_t)(ui + 1) * kSyncThreads + (t - n_first - skip)] = (uint16_t)(task - kHuffOwn);
        if (t == 0) {
            tail_count[ui] = (uint32_t)n_first;
            if (second) tail_count[ui + 1] = (uint32_t)(pending - n_first - skip);
        }
    }
#pragma unroll
    for (int row = t; row < 2 * kSyncThreads; row += kSyncThreads)
        if (row >= 1 && row < n_rows) __hip_atomic_store(&gstate[subseq_of(row)], sh.end[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) {
        const unsigned n_units = second ? 2u : 1u;
        incoming[ui] = sh.end[0] & kSyncMask;
        if (second) incoming[ui + 1] = sh.second_from;
        // per unit, as huff_sync_kernel counts: workgroups whose last end state is new; correction rounds (sum, maximum)
        atomicAdd(counters + 1, n_units);
        atomicAdd(counters + 2, (unsigned)rounds * n_units);
        atomicMax(counters + 3, (unsigned)rounds);
    }
}

// ---- tail corrections ---------------------------------------------------------------------------------------------------
// After pass 0 and the first correction rounds most subsequences are settled; what remains are chains: a decoder that has
// not yet found the MCU phase hands a wrong end state to its successor, which must be decoded again, and so on for a few
// thousand bits (per round a third of the subsequences decoded still change their end state: 8-10 rounds for a 1080p picture).
// Each link is one full single-lane decode, strictly after the previous one, so the kernel's time is the longest chain -- IF
// every group is resident.  One WAVE per group of 255 subsequences; kTailWaves waves share a workgroup and with it the lookup
// tables in LDS; a wave has kTailSlots row buffers (a lane stages the row it is about to decode: reading the stream through
// the vector cache instead costs a lone lane a third more per round) and takes more tasks than that in several helpings -- only
// the first tail round has that many; end states live in global memory.  So all groups of a 256 x 1080p batch are resident at
// once.  (One wave per workgroup with its own 12 KB of tables and 64 rows: 7 per CU, the batch took 2.1 shifts -- 543 us
// against 300 us for a batch that fits.)  The waves of a workgroup never synchronise with each other after the tables are in
// place.
constexpr int kTailWaves = 4;
constexpr int kTailThreads = 64 * kTailWaves;
#ifndef HJ_TAIL_SLOTS
#define HJ_TAIL_SLOTS 32  // A/B switch (tools/ab_entropy.sh): 64 row buffers per wave halve the helpings of the first tail round -- and take 414 us against 287
#endif
constexpr int kTailSlots = HJ_TAIL_SLOTS;
static_assert(kTailSlots == 32 || kTailSlots == 64, "a power of two, at most one row buffer per lane");
constexpr int kTailRowWords = kSubseqWords + 4;  // whole 16-byte groups

struct TailWave {
    uint32_t rows[kTailSlots * kTailRowWords];
    uint16_t list[2][kSyncThreads];  // subsequences to decode this round / next round
    uint32_t count[2];
};
struct TailShared {
    TailWave wave[kTailWaves];
    uint32_t tsel[10];
};

struct TailEnv : LdsTables {
    uint32_t row_base;  // LDS byte address of this lane's row buffer
    uint32_t word0;     // image word index of its first word
    const uint32_t* boundaries;
    uint32_t num_boundaries;
    __device__ __forceinline__ uint32_t boundary(uint32_t i) const { return load_boundary(boundaries, num_boundaries, i); }
    static constexpr uint32_t kCursorStep = (uint32_t)kTailSlots * 4u;  // the slots are transposed like the rows of the sync kernel
    __device__ __forceinline__ uint32_t cursor(uint32_t i) const { return row_base + (i - word0) * kCursorStep; }
    __device__ __forceinline__ uint32_t fetch(uint32_t c) const { return *(const HJ_LDS uint32_t*)(uintptr_t)c; }
};
// The walk of a tail lane: the branch form, with or without restart handling (a wave-uniform choice: one image per wave), with or
// without records (uniform too; never across restart boundaries).
__device__ __forceinline__ SubseqState lane_walk(bool rst, bool record, const HuffGeom& geom, const TailEnv& env, uint32_t begin, uint32_t limit, int z, int k,
                                                 uint32_t boundary0, const SlotRecorder& rec)
{
    if (rst) return decode_subsequence<true>(geom, env, begin, limit, z, k, boundary0);
    return record ? decode_subsequence<false>(geom, env, begin, limit, z, k, 0, rec) : decode_subsequence<false>(geom, env, begin, limit, z, k);
}

// orders a wave's own LDS / global traffic between its lanes (the waves of the tail kernel run on their own)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// RIPPLE mode (the launches behind the first): nothing is handed over by the sync kernel; a group whose predecessor's last end state
// is no longer the state it was entered with starts over at its first subsequence, and the correction runs as far as it changes
// anything.  counters[0] counts the groups whose own last end state moved -- zero: the batch has converged.
//
// The first launch enters the same way.  When it starts the sync kernel is done, and the state in front of every group has two
// correction rounds behind it; the state the group's first subsequence was decoded from (incoming[]: for a pair's first unit the
// halo lane's decode from an assumed state, wrong for one group in three; for its second unit a state of the first unit's last row)
// may no longer be that state.  So the group takes the state in front as it is when its wave gets there, and
// if that is not the guess, its first subsequence joins the first round as one more chain beside the ones handed over.  When its
// lists are empty the wave looks in front once more (kTailReentries times at most) and follows what it finds as a single chain; it
// never waits -- not every batch has all its groups resident -- and a group that is done before the one in front of it moved is
// left to the ripple launch, as before.
// The read is no snapshot: the wave of the group in front may already have stored a newer last end state, or store one a moment
// later.  Whatever is read is a state that group had at some time; incoming[] records exactly the state that was used; the ripple
// launch behind compares it with the final one and starts the group over if they differ.  So the result does not depend on timing,
// only the split of the work between the two launches does.  This rests on two facts: one wave alone writes a group's states and
// records, and a subsequence's last decode is the one from its converged start state, so its record is final.

// the state in front of group `u` as it is now (0 for the first group of an image)
__device__ __forceinline__ unsigned long long state_in_front(const unsigned long long* states, const HuffImage& im, const HuffUnit u)
{
    return u.first ? __hip_atomic_load(&states[im.first_subseq + u.first - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kSyncMask : 0ull;
}

// the chains of one group (sync unit `ui`), walked by one wave
// ---- one chain link by a whole wave ---------------------------------------------------------------------------------------------
// The last links of a chain are one lane's work with 63 lanes idle, 28 us per subsequence: a lone wave pays 10+ cycles for every
// dependent instruction of the decode step.  With one or two chains left the wave turns to ONE subsequence instead
// (cooperative_subsequence in huffman_gpu_core.h, the window below): lane l decodes
// the symbol that WOULD start l bits behind the current position (as a DC symbol and as an AC symbol of the current MCU position:
// two lookups per lane, all lanes at once), and the walk itself is scalar -- read the entry at the current offset, add its length,
// track zigzag position and MCU position -- about a dozen scalar instructions per symbol instead of fifty vector ones.  Same state
// evolution as decode_subsequence<false>, symbol by symbol (a pair step there is two steps here).  Streams with restart intervals
// keep the lane-parallel walk.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

// row: the wave's row buffer (word j of the subsequence at row[j * kTailSlots], kTailRowWords of them), staged by the caller
// The window of cooperative_subsequence (huffman_gpu_core.h) on a wave: lane l holds the entries for bit offset l.
// row: the wave's row buffer (word j of the subsequence at row[j * kTailSlots], kTailRowWords of them), staged by the caller.
struct CoopWindow : LdsTables {
    const HJ_LDS uint32_t* row;
    uint32_t row_bit0, lane;
    uint32_t edc, eac;
    __device__ __forceinline__ uint32_t entry(uint32_t table, uint32_t w) const
    {
        uint32_t e = lookup1(table, w);
        if ((e >> 9) == kZadvLong) e = lookup2(e, w);
        return e;
    }
    __device__ __forceinline__ void open(uint32_t pos, uint32_t ts)
    {
        const uint32_t b = pos + lane - row_bit0, bit = b & 31u;  // the 32 bits from bit pos + lane on
        const uint32_t w0 = row[(b >> 5) * kTailSlots], w1 = row[((b >> 5) + 1) * kTailSlots];
        const uint32_t w = bit ? __builtin_amdgcn_alignbit(w0, w1, 32u - bit) : w0;
        edc = entry(ts & 0xFFFFu, w);
        eac = entry(ts >> 16, w);
    }
    __device__ __forceinline__ uint32_t dc(uint32_t rel) const { return lane_read(edc, rel); }
    __device__ __forceinline__ uint32_t ac(uint32_t rel) const { return lane_read(eac, rel); }
};

// Round budget.  A 1080p photograph at q90 needs 11 rounds in the tail and 3 in a ripple launch; noise at q98 -- long codes, few
// symbols per subsequence, slow to fall into step -- 125 and 40 (tests/devtools/rounds_by_quality.py).  A chain that is still
// going after 192 subsequences (a fifth of a megabit without meeting the true trajectory) sits on a periodic stream and would
// walk through the rest of the image, 28 us per subsequence: the image is given up (the host decoder takes it).
constexpr int kTailRoundBudget = 192, kRippleRoundBudget = 192;
#ifndef HJ_COOP_CHAINS
#define HJ_COOP_CHAINS 2
#endif
constexpr int kCoopChains = HJ_COOP_CHAINS;  // chains a round may have left for the wave to take them one by one (0: never)
#ifndef HJ_TAIL_REENTRIES
#define HJ_TAIL_REENTRIES 4
#endif
constexpr uint32_t kTailEnter = 1u << 31;  // huff_tail_kernel's work word of a group: the state in front of it has moved
constexpr int kTailReentries = HJ_TAIL_REENTRIES;  // times a group of the first tail launch looks in front again when its lists are empty
                                                   // (2, 4 and 8 measure the same: profiles/tail_entry/README.md)

// Both builds enter with state_in_front() as it reads at that moment and store what they used to incoming[ui]; why a read that
// races with the wave of the group in front cannot change the result is argued under "RIPPLE mode" above (one wave alone writes a
// group's states and records; a subsequence's last decode is the one from its converged start state).
template <bool RIPPLE>
__device__ __forceinline__ void tail_group(TailWave& ws, TailEnv env, HuffImage& im, const HuffUnit u, uint32_t ui, int lane,
                                           unsigned long long* __restrict__ states, unsigned long long* __restrict__ incoming,
                                           unsigned int* __restrict__ counters, const uint16_t* __restrict__ tail_tasks, uint32_t pending,
                                           uint32_t pass_id, uint16_t* records)
{
    const HuffGeom geom = make_geom(im);
    const uint32_t nsub = (geom.total_bits + kSubseqBits - 1) / kSubseqBits;
    if (u.first >= nsub) return;
    unsigned long long* gstate = states + im.first_subseq;
    const int n_rows = (int)min((uint32_t)kSyncThreads, nsub - u.first + 1);
    // the state the group is entered with ([0] of its rows): the one in front of it now, read once
    unsigned long long entering = state_in_front(states, im, u);
    if (RIPPLE) {
        if (lane == 0) {
            incoming[ui] = entering;
            ws.list[0][0] = 1;
        }
    } else {
        for (uint32_t i = lane; i < pending; i += 64) ws.list[0][i] = tail_tasks[(size_t)ui * kSyncThreads + i];
        // The sync kernel's rounds moved the state in front since the group's row 1 was last decoded from it (a pair's first unit:
        // from the halo's guess; its second unit: from the first unit's last row as it then was): row 1 is decoded again, an
        // ordinary member of the first Jacobi round.  Task 1 is never among the tasks handed over -- the sync kernel lists rows 2
        // and up and leaves row 1 to this test.
        if (entering != incoming[ui]) {  // uniform
            if (lane == 0) {
                incoming[ui] = entering;
                ws.list[0][pending] = 1;
            }
            pending++;
        }
    }
    if (lane == 0) ws.count[0] = pending;
    wave_sync();
    const bool rst = im.restart_interval != 0;
    const bool recording = !rst;  // every decode here can be a subsequence's last one
    bool out_moved = false;  // the group's last end state changed
    const HJ_GLOBAL uint32_t* g = (const HJ_GLOBAL uint32_t*)im.stream;
    const uint32_t gwords = im.stream_words;
    env.row_base = (uint32_t)(uintptr_t)(HJ_LDS uint32_t*)&ws.rows[lane & (kTailSlots - 1)];  // word k of slot s at index k * kTailSlots + s
    int rounds = 0, cur = 0, reentries = 0;
    bool unfinished = false;
    for (;;) {
        uint32_t n = ws.count[cur];
        if (n == 0) {
            // Nothing left: look in front once more before leaving.  The group in front may have moved on meanwhile; what it has
            // now is taken like the state at entry, as one chain from row 1.  No waiting: a group that is done before its
            // predecessor moved is left to the ripple launch.  The round count carries on.
            if (RIPPLE || reentries >= kTailReentries || rounds >= kTailRoundBudget) break;
            const unsigned long long front = state_in_front(states, im, u);
            if (front == entering) break;  // uniform
            reentries++;
            entering = front;
            wave_sync();  // every lane has read the count
            if (lane == 0) {
                incoming[ui] = entering;
                ws.list[cur][0] = 1;
                ws.count[cur] = 1;
            }
            wave_sync();
            n = 1;
        }
        if (rounds >= (RIPPLE ? kRippleRoundBudget : kTailRoundBudget)) {
            unfinished = true;
            break;
        }
        rounds++;
        wave_sync();  // every lane has read the count before it is reused
        if (lane == 0) ws.count[cur ^ 1] = 0;
        wave_sync();
        if (kCoopChains > 0 && n <= (uint32_t)kCoopChains && !rst) {
            // the few chains that are left, one after the other, each followed to its end by the whole wave (cooperative_subsequence)
            CoopWindow win;
            static_cast<LdsTables&>(win) = env;
            win.row = (const HJ_LDS uint32_t*)&ws.rows[0];
            win.lane = (uint32_t)lane;
            win.edc = win.eac = 0;
            const uint32_t changes = cooperative_table_changes(win, geom.blocks_per_mcu);
            for (uint32_t q = 0; q < n && !unfinished; q++) {
                for (int task = (int)uni(ws.list[cur][q]);; task++) {
                    if (rounds++ >= (RIPPLE ? kRippleRoundBudget : kTailRoundBudget)) {
                        unfinished = true;
                        break;
                    }
                    const unsigned long long before =
                        task == 1 ? entering : __hip_atomic_load(&gstate[u.first - 2 + task], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long old = __hip_atomic_load(&gstate[u.first - 1 + task], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t word0 = (u.first - 1 + task) * kSubseqWords;
                    wave_sync();  // the row buffer's last reader is done
                    if (lane < kTailRowWords) {
                        const uint32_t d = word0 + lane;
                        ws.rows[lane * kTailSlots] = d < gwords ? __builtin_bswap32(g[d]) : ~0u;
                    }
                    wave_sync();
                    const SubseqState p = unpack_state(before);
                    win.row_bit0 = word0 * 32u;
                    const uint32_t jt = u.first - 1 + task;
                    // (every lane stores the same value to the same address: one write)
                    const SlotRecorder rec = slot_recorder(records, im, jt);
                    const SubseqState st = cooperative_subsequence(geom, win, changes, p.end_bit, (jt + 1) * kSubseqBits, p.zk & 255u, p.zk >> 8, rec);
                    if (lane == 0) put_mark(rec, p.end_bit, (jt + 1) * kSubseqBits, geom.total_bits, p.zk & 255u, st);
                    const unsigned long long now = pack_state(st);
                    const bool moved = ((now ^ old) & kSyncMask) != 0;
                    if (lane == 0) __hip_atomic_store(&gstate[u.first - 1 + task], now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    wave_sync();
                    if (!moved) break;
                    if (task + 1 >= n_rows) {
                        out_moved = true;
                        break;
                    }
                }
            }
            if (unfinished) break;
            cur ^= 1;  // every chain has been followed to its end: the list for the next round is empty
            continue;
        }
        for (uint32_t base = 0; base < n; base += kTailSlots) {
            const bool busy = lane < kTailSlots && base + lane < n;
            const int task = busy ? (int)ws.list[cur][base + lane] : 1;
            unsigned long long now = 0;
            bool moved = false;
            if (busy) {
                // Jacobi: every lane of the iteration starts from the end state its predecessor had BEFORE this iteration
                const unsigned long long before =
                    task == 1 ? entering : __hip_atomic_load(&gstate[u.first - 2 + task], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long old = __hip_atomic_load(&gstate[u.first - 1 + task], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // stage the row: 32 words + the reader's look-ahead, straight from the destuffed stream
                env.word0 = (u.first - 1 + task) * kSubseqWords;
                HJ_LDS uint32_t* row = (HJ_LDS uint32_t*)(uintptr_t)env.row_base;
#pragma unroll
                for (int i = 0; i < kTailRowWords / 4; i++) {
                    const uint32_t d = env.word0 + 4 * i;
                    const u32x4 x = *(const HJ_GLOBAL u32x4*)(g + min(d, (gwords - 1) & ~3u));
                    const bool ok = d < gwords;
                    row[(4 * i + 0) * kTailSlots] = ok ? __builtin_bswap32(x.x) : ~0u;
                    row[(4 * i + 1) * kTailSlots] = ok ? __builtin_bswap32(x.y) : ~0u;
                    row[(4 * i + 2) * kTailSlots] = ok ? __builtin_bswap32(x.z) : ~0u;
                    row[(4 * i + 3) * kTailSlots] = ok ? __builtin_bswap32(x.w) : ~0u;
                }
                const SubseqState p = unpack_state(before);
                const uint32_t jt = u.first - 1 + task;
                const SlotRecorder rec = slot_recorder(records, im, jt);
                const SubseqState st = lane_walk(rst, recording,geom, env, p.end_bit, (jt + 1) * kSubseqBits, p.zk & 255, p.zk >> 8, boundary0_of(im, jt), rec);
                if (recording) put_mark(rec, p.end_bit, (jt + 1) * kSubseqBits, geom.total_bits, p.zk & 255, st);
                now = pack_state(st);
                moved = ((now ^ old) & kSyncMask) != 0;
            }
            wave_sync();  // all start states have been read
            if (busy) __hip_atomic_store(&gstate[u.first - 1 + task], now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out_moved |= busy && moved && task + 1 == n_rows;
            const bool more = busy && moved && task + 1 < n_rows;
            const unsigned long long mask = __ballot(more);
            const uint32_t have = ws.count[cur ^ 1];
            if (more) ws.list[cur ^ 1][have + __popcll(mask & ((1ull << lane) - 1))] = (uint16_t)(task + 1);
            wave_sync();
            if (lane == 0) ws.count[cur ^ 1] = have + (uint32_t)__popcll(mask);
            wave_sync();
        }
        cur ^= 1;
    }
    const bool any_out = __ballot(out_moved) != 0;
    if (lane == 0) {
        atomicAdd(counters + (RIPPLE ? 4 : 6), (unsigned)rounds);
        atomicMax(counters + (RIPPLE ? 5 : 7), (unsigned)rounds);
        if (unfinished) {
            im.gave_up = 1;  // benign race: every writer stores the same value
        } else if (RIPPLE && any_out) {
            atomicAdd(counters + 0, 1u);
            im.moved_pass = pass_id;  // (same)
        }
    }
}

// (at least 5 waves per SIMD, i.e. at most 96 VGPRs: what "every group of the batch resident at once" rests on)
template <bool RIPPLE>
__global__ __launch_bounds__(kTailThreads, 5) void huff_tail_kernel(HuffImage* __restrict__ images, const HuffUnit* __restrict__ units, int nunits,
                                                                 unsigned long long* __restrict__ states, unsigned long long* __restrict__ incoming,
                                                                 unsigned int* __restrict__ counters, const uint16_t* __restrict__ tail_tasks,
                                                                 const uint32_t* __restrict__ tail_count, uint32_t pass_id, uint16_t* records)
{
    __shared__ TailShared sh;
    extern __shared__ uint16_t dyn_pool[];
    HJ_LDS uint16_t* pool = (HJ_LDS uint16_t*)dyn_pool;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t ui0 = blockIdx.x * kTailWaves, ui = ui0 + wave;
    const bool valid = ui < (uint32_t)nunits;
    const HuffUnit u = units[valid ? ui : ui0];
    // what every group of the workgroup has to do (uniform: every lane looks at all of them)
    uint32_t todo[kTailWaves];
    // Most workgroups of the ripple launch find nothing to do, and the way out is a chain of dependent loads: unit -> descriptor ->
    // state in front.  The four groups' loads of a level go out together (clamped indices instead of branches), so a workgroup
    // pays the chain once, not four times.
    {
        HuffUnit uq[kTailWaves];
        uint32_t bits[kTailWaves], gave[kTailWaves], base[kTailWaves];
        unsigned long long front[kTailWaves], came[kTailWaves];
#pragma unroll
        for (int q = 0; q < kTailWaves; q++) {
            const uint32_t i = min(ui0 + q, (uint32_t)nunits - 1);
            uq[q] = units[i];
            came[q] = incoming[i];
            todo[q] = RIPPLE ? 0u : tail_count[i];  // the sync kernel left tasks (at most kHuffOwn)
        }
#pragma unroll
        for (int q = 0; q < kTailWaves; q++) {
            const HuffImage& iq = images[uq[q].image];
            bits[q] = iq.total_bits;
            gave[q] = iq.gave_up;
            base[q] = iq.first_subseq;
        }
#pragma unroll
        for (int q = 0; q < kTailWaves; q++) {
            const uint32_t nsub = (bits[q] + kSubseqBits - 1) / kSubseqBits;
            const bool inside = uq[q].first != 0 && uq[q].first < nsub;  // (a group past the stream's end is never entered)
            front[q] = __hip_atomic_load(&states[inside ? base[q] + uq[q].first - 1 : 0u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kSyncMask;
            if (uq[q].first == 0) front[q] = 0;
            if (uq[q].first >= nsub || gave[q] != 0) front[q] = came[q];
        }
#pragma unroll
        for (int q = 0; q < kTailWaves; q++) {
            // or the state in front is no longer the one the group was entered with (the first launch: pass 0's guess)
            if (front[q] != came[q]) todo[q] |= kTailEnter;
            if (ui0 + q >= (uint32_t)nunits) todo[q] = 0;
        }
        if ((todo[0] | todo[1] | todo[2] | todo[3]) == 0) return;  // uniform, before anything is staged
    }
    static_assert(kTailWaves == 4, "the work test above");
    uint32_t pending = 0;
#pragma unroll
    for (int q = 0; q < kTailWaves; q++) pending = q == wave ? todo[q] : pending;
    const bool work_here = pending != 0;
    pending = RIPPLE ? pending >> 31 : pending & ~kTailEnter;  // the tasks handed to tail_group, which looks in front itself
    // the groups of a workgroup usually belong to one image; where an image ends inside it, its tables are staged in turn
#pragma unroll 1
    for (int s = 0; s < kTailWaves; s++) {
        if (ui0 + s >= (uint32_t)nunits) break;  // uniform
        const uint32_t image = units[ui0 + s].image;
        if (s > 0 && image == units[ui0 + s - 1].image) continue;  // uniform: staged with the slot before
        uint32_t work = 0;
#pragma unroll
        for (int q = 0; q < kTailWaves; q++)
            if (ui0 + q < (uint32_t)nunits && units[ui0 + q].image == image) work |= todo[q];
        if (work == 0) continue;  // uniform: nothing left in this image's groups
        HuffImage& im = images[image];
        __syncthreads();  // the tables of the image before are no longer in use
        stage_pool<kTailThreads>(pool, im);
        stage_constants(sh.tsel, nullptr, nullptr, im, false);
        __syncthreads();
        if (valid && u.image == image && work_here) {
            TailEnv env;
            env.row_base = 0;
            env.word0 = 0;
            env.pool = (uint32_t)(uintptr_t)pool;
            env.tsel = (const HJ_LDS uint32_t*)sh.tsel;
            env.boundaries = im.boundaries;
            env.num_boundaries = im.num_boundaries;
            tail_group<RIPPLE>(sh.wave[wave], env, im, u, ui, lane, states, incoming, counters, tail_tasks, pending, pass_id, records);
        }
    }
}

// ---- write pass, step 1: where the blocks start -----------------------------------------------------------------------------
// One lane per subsequence (the sync units, lane 0 idles).  First the number of the block in progress where the lane's subsequence
// begins: the completed-block counts (SubseqState::nblocks, the top 16 bits of a state) of the image's subsequences in front of the
// unit, which every workgroup sums for itself -- at most one image's states, all of a lane's loads in flight together -- plus a scan
// of the unit's own counts.  No workgroup waits for another.  (The sums in front cost an image of n subsequences n * n / 510 two-byte
// loads in all: 33 k for a 1080p photograph's 4,096, cached; a single scan of 100 MB, 800 k subsequences, would pay a billion --
// from some tens of thousands of subsequences on, the sums belong in a pass of their own again.)  The workgroup that holds the image's last subsequence knows how many
// blocks the stream completes: it writes decoded_blocks and flags a stream that ends before the last block.
// Then the records: a lane takes its usable record -- the last synchronisation decode took it, from the converged start state;
// walkers[unit] = how many lanes of the unit have none (overflow, an image with restart intervals: their damage check is in the
// walk, or records == nullptr: HIPJPEG_POSITION_PASS=1); those get first_block[] for huff_pos_kernel.  When every lane has one, the
// records of the unit name one contiguous run of blocks: they are gathered in LDS and leave as consecutive dwords (stored straight
// from the lanes, a wave's stores would touch a cache line per lane).
constexpr int kCopyCapacity = kHuffOwn * kRecSlots;  // blocks the records of a unit can name
constexpr int kSyncWaves = kSyncThreads / 64;
__global__ __launch_bounds__(kSyncThreads) void huff_copy_records_kernel(HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                                     const unsigned long long* __restrict__ states, uint32_t* __restrict__ first_block,
                                                                     const uint16_t* __restrict__ records, uint32_t* __restrict__ walkers)
{
    __shared__ uint32_t s_pos[kCopyCapacity];
    __shared__ uint32_t s_range[2];  // first block of the run, block behind it
    __shared__ uint32_t s_front[kSyncWaves], s_own[kSyncWaves];
    const HuffUnit u = units[blockIdx.x];
    HuffImage& im = images[u.image];
    const uint32_t nsub = (im.total_bits + kSubseqBits - 1) / kSubseqBits;
    const int t = threadIdx.x;
    const uint32_t j = u.first - 1 + t;
    const bool owner = t != 0 && j < nsub;
    const uint32_t g = im.first_subseq + j;
    // the counts: little-endian states, nblocks in bits 48..63 = the fourth uint16
    const HJ_GLOBAL uint16_t* counts = (const HJ_GLOBAL uint16_t*)(states + im.first_subseq) + 3;
    const uint32_t nfront = min(u.first, nsub);
    uint32_t front = 0;
    constexpr int kBatch = 8;  // independent loads in flight per lane
    for (uint32_t i0 = t; i0 < nfront; i0 += kBatch * kSyncThreads) {
        uint32_t d[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const uint32_t i = i0 + k * kSyncThreads;
            d[k] = i < nfront ? counts[(size_t)i * 4] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) front += d[k];
    }
    const uint32_t own = owner ? counts[(size_t)j * 4] : 0u;
    bool walk = owner;
    uint32_t n = 0, fresh = 0;
    u32x4 v[kRecShorts / 8];
    if (owner && records && im.restart_interval == 0) {
        // the whole record in one go (64 bytes: four 16-byte loads in flight together), the mark last
        const HJ_GLOBAL u32x4* src = (const HJ_GLOBAL u32x4*)records + (size_t)g * (kRecShorts / 8);
#pragma unroll
        for (int q = 0; q < kRecShorts / 8; q++) v[q] = src[q];
        const uint32_t mark = v[kRecShorts / 8 - 1].w >> 16;
        if (mark_valid(mark)) {
            walk = false;
            n = mark & (kRecFresh - 1u);
            fresh = mark & kRecFresh;
        }
    }
    // wave sums of the counts in front, inclusive wave scans of the own counts; the rest through LDS
    for (int off = 32; off > 0; off >>= 1) front += __shfl_xor(front, off);
    uint32_t incl = own;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(incl, d);
        if ((t & 63) >= d) incl += x;
    }
    if ((t & 63) == 63) {
        s_front[t >> 6] = front;
        s_own[t >> 6] = incl;
    }
    const int n_walk = __syncthreads_count(walk);
    uint32_t fb = incl - own;  // the block in progress where subsequence j begins
#pragma unroll
    for (int w = 0; w < kSyncWaves; w++) fb += s_front[w] + (w < (t >> 6) ? s_own[w] : 0u);
    if (t == 0) walkers[blockIdx.x] = (uint32_t)n_walk;
    const uint32_t total_blocks = im.total_blocks;
    {
        // the image's last subsequence (a stream without a bit: the unit at 0, its lane 0)
        const uint32_t last_sub = nsub ? nsub - 1 : 0u;
        if (nsub ? j == last_sub && t != 0 : u.first == 0 && t == 0) {
            const uint32_t decoded = fb + own;
            im.decoded_blocks = decoded;
            if (decoded < total_blocks) im.status = 2;  // the stream ends before the last block
        }
    }
    if (u.first >= nsub) return;  // uniform: no subsequence here
    if (walk) first_block[g] = fb;
    // the record's blocks are consecutive: the one in progress at the start if fresh, else the next one
    const uint32_t b0 = fb + (fresh ? 0u : 1u);
    HJ_GLOBAL uint32_t* out = (HJ_GLOBAL uint32_t*)im.block_pos;
    const uint32_t bit0 = j * kSubseqBits;
    auto slot = [&](int i) { return bit0 + ((v[i >> 3][(i >> 1) & 3] >> (16 * (i & 1))) & 0xFFFFu); };
    if (n_walk == 0) {
        // uniform: lane 1 holds the first block of the run, the last owner the block behind it (unsettled streams -- the host
        // decoder takes them -- can have anything here: the run is clipped to the buffer)
        const int last = (int)min((uint32_t)kSyncThreads, nsub - u.first + 1) - 1;
        if (t == 1) s_range[0] = b0;
        if (t == last) s_range[1] = b0 + n;
        __syncthreads();
        const uint32_t base = s_range[0];
#pragma unroll
        for (int i = 0; i < kRecSlots; i++) {
            const uint32_t at = b0 - base + (uint32_t)i;
            if ((uint32_t)i < n && at < (uint32_t)kCopyCapacity) s_pos[at] = slot(i);
        }
        __syncthreads();
        const uint32_t count = min(s_range[1] - base, (uint32_t)kCopyCapacity);
        for (uint32_t i = t; i < count; i += kSyncThreads)
            if (base + i < total_blocks) out[base + i] = s_pos[i];
    } else if (!walk) {
#pragma unroll
        for (int i = 0; i < kRecSlots; i++)
            if ((uint32_t)i < n && b0 + i < total_blocks) out[b0 + i] = slot(i);
    }
}

// Then the walks, same workgroup shape: every lane whose subsequence has no usable record walks it from the converged start state
// and records the bit position of each block that starts inside it.  A workgroup without such lanes leaves at once.
// records == nullptr: every subsequence is walked (HIPJPEG_POSITION_PASS=1).
// A launch of its own, behind every batch (which records overflowed only the device knows): the walk's registers (97, four waves per
// SIMD) and its LDS (the staged rows and tables, 50 KB) inside huff_copy_records_kernel would take that kernel from five resident
// workgroups per CU to three.
__global__ __launch_bounds__(kSyncThreads) void huff_pos_kernel(HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                            const unsigned long long* __restrict__ states, const uint32_t* __restrict__ first_block,
                                                            const uint16_t* __restrict__ records, const uint32_t* __restrict__ walkers)
{
    __shared__ WgShared sh;
    extern __shared__ uint16_t dyn_pool[];
    HJ_LDS uint16_t* pool = (HJ_LDS uint16_t*)dyn_pool;
    const HuffUnit u = units[blockIdx.x];
    HuffImage& im = images[u.image];
    const HuffGeom geom = make_geom(im);
    const uint32_t nsub = (geom.total_bits + kSubseqBits - 1) / kSubseqBits;
    if (u.first >= nsub) return;
    if (records && walkers[blockIdx.x] == 0) return;  // uniform: every record of the workgroup was usable
    const int t = threadIdx.x;
    const uint32_t j = u.first - 1 + t;
    const bool rst = im.restart_interval != 0;
    bool walk = t != 0 && j < nsub;
    if (walk && records && !rst) walk = !mark_valid(records[(size_t)(im.first_subseq + j) * kRecShorts + kRecMark]);
    stage_rows<kSyncThreads>(sh.stream, im, (int)u.first - 1);
    stage_pool<kSyncThreads>(pool, im);
    stage_constants(sh.tsel, nullptr, nullptr, im, false);
    __syncthreads();
    if (!walk) return;
    DevEnv env = make_env(sh, pool, u.first, geom, im);
    env.set_row(t);
    const unsigned long long* st = states + im.first_subseq;
    uint32_t begin = 0;
    int z = 0, k = 0;
    if (j > 0) {
        const SubseqState p = unpack_state(st[j - 1]);
        begin = p.end_bit;
        z = p.zk & 255;
        k = p.zk >> 8;
    }
    HJ_GLOBAL uint32_t* out = (HJ_GLOBAL uint32_t*)im.block_pos;
    const uint32_t total_blocks = im.total_blocks;
    auto rec = [&](uint32_t block, uint32_t pos) {
        if (block < total_blocks) out[block] = pos;
    };
    if (rst) {
        uint32_t fault = 0;
        position_subsequence<true>(geom, env, begin, (j + 1) * kSubseqBits, z, k, first_block[im.first_subseq + j], rec, boundary0_of(im, j), &fault);
        if (fault) im.status = 1;  // damaged restart interval: the host decoder takes the image (benign race: same value)
    } else
        position_subsequence<false>(geom, env, begin, (j + 1) * kSubseqBits, z, k, first_block[im.first_subseq + j], rec);
}

// ---- write pass, step 2: one lane per block -----------------------------------------------------------------------------------
// A TEAM of 256 lanes takes one block unit: kHuffMcusPerWg consecutive MCUs (scan order) of one image, 256 blocks per round.  Every
// lane decodes its block into a 128-byte LDS buffer, and the finished blocks leave as whole 128-byte lines, eight lanes per block --
// each line written once, no memset, no partial-line traffic.  Lanes idle once their block is done: chroma blocks are
// short, luma blocks long; the wave runs as long as its longest block.  Block buffers and the flush are a wave's own (lane t flushes
// buffers of lanes t & ~63 ..., and fetches their destinations with a cross-lane read), so between the rounds a wave only has to order
// its own LDS traffic: the waves of a team do not wait for each other's longest block.
//
// A WORKGROUP is kBTeams = 2 teams: two consecutive units of the same image, one copy of the image's lookup tables and constants.  What
// this buys is residency: the pass waits on latency, LDS is what limits its waves, and the table copy was the part of a workgroup's LDS
// that bought no lanes.  Per 512 lanes: 2 x 32 KB of block buffers + the tables (13,824 B for the standard ones) + 384 B of constants
// = 79,744 B, so two workgroups fit the CU's 160 KiB -- 16 waves per CU, four per SIMD, where 256-lane workgroups with a table copy
// each stopped at three (static_assert below).  Larger tables (up to 24 KB): one workgroup per CU, 8 waves, as two 256-lane ones had
// before.  Measured on 256 x 1080p: 576 us against 600 (profiles/block_pass_teams/), 486 since the zero fill goes through the
// swizzle too (profiles/block_pass_residency/).
//   * The units of an image are consecutive in `units`, unit j of the image covering MCUs j * kHuffMcusPerWg ...; the grid has one
//     workgroup per unit, and the workgroup that looks at unit j works only if j is a multiple of kBTeams: it takes units j .. j +
//     kBTeams - 1 as far as the image has them.  The others leave at once, whole workgroups, in front of every barrier (which
//     workgroup looks at which unit: see the kernel).  A workgroup never spans two images; an image with an odd number of units
//     ends with a workgroup whose second team has no unit.
//   * A team without work -- no unit, or a truncated stream whose decoded blocks end in front of its unit -- has zero items: it
//     stages its share of the tables, arrives at both workgroup barriers, and writes zero group sums for its unit if it has one.
//     No lane returns between the two barriers.
//   * Each unit keeps its own four group sums: the DC pass sees what it saw with one unit per workgroup.
constexpr int kBTeamThreads = kHuffBlocksPerWg;  // lanes of a team (one block per lane per round)
constexpr int kBTeams = 2;                       // measured: 1 team (3 workgroups per CU) 564 us, 2: 486 (651 / 576 / 4 teams, one 1024-lane workgroup: 634, with the unswizzled zero fill) -- DESIGN.md §3.2
constexpr int kBThreads = kBTeams * kBTeamThreads;
static_assert((kBTeams & (kBTeams - 1)) == 0, "unit j starts a workgroup when j % kBTeams == 0");
// 128-byte buffers, lane L's at byte L * 128.  The starts of a wave's buffers would all fall on bank 0; instead of padding the
// stride (144 before: 16 bytes per lane that the budget above does not have) the 16-byte chunks inside a buffer are swizzled:
// byte x of lane L's block lives at (L * 128 | (L & 7) << 4) ^ x.  For equal x the lanes of a wave then hit eight distinct 16-byte
// offsets of the 128 bytes the 32 banks of a 2-byte store span -- the same spread as stride 144 (L * 144 mod 128 = (L & 7) * 16) --
// and the store's address is one XOR of a per-lane constant with the byte offset, which the zigzag table holds ready (doubled).
// Every access takes the swizzle: put(), the flush reads (chunk c of lane L at unit c ^ (L & 7)) and the zero fill.
constexpr int kBlockBufBytes = 128;

struct BlockShared {
    // the constants first: their addresses stay below 64 KB, the reach of the offset field of an LDS instruction (the zigzag byte
    // is read in every coefficient step)
    KSlot kslot[10];
    uint32_t tsel[10];
    uint32_t zz[16];  // zigzag permutation as BYTE offsets into a block (2 * index), 4 entries per word
    int32_t dc_sum[kBTeams][4];  // per team and component: sum of the DC differences of the team's blocks
    uint32_t kcomp[10];          // component of MCU position k
    __attribute__((aligned(128))) uint8_t blocks[kBThreads * kBlockBufBytes];  // 128-aligned: the swizzle XORs below bit 7
};
// The budget.  gfx950 hands out LDS in units of 1,280 bytes (160 KiB / 128), measured on the device: 256-lane workgroups with 53,760 B
// are resident three per CU, with 54,272 B two (units of 512 B would still allow three); 81,920 B two, 81,921 B one
// (profiles/block_pass_teams/lds_granule.txt).  Two workgroups with the standard tables must fit a CU: the four Annex K tables are
// 13,696 B as the stage expands them (6,144 first-level and pair entries + 11 second-level tables of 64), 13,824 B of dynamic LDS
// as the launcher rounds it.
constexpr unsigned kLdsBytesPerCu = 160u * 1024u, kLdsGranule = 1280u, kStandardPoolBytes = 13824u;
constexpr unsigned lds_allocated(unsigned bytes) { return (bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule; }
static_assert(2 * lds_allocated((unsigned)sizeof(BlockShared) + kStandardPoolBytes) <= kLdsBytesPerCu,
              "two 512-lane workgroups of the block pass per CU (16 waves) with the standard lookup tables");

struct BlockEnv : LdsTables {
    const uint32_t* gstream;
    uint32_t gwords;
    uint32_t buf;  // LDS byte address of this lane's block buffer with its swizzle, (L * 128 | (L & 7) << 4)
    const HJ_LDS KSlot* kslot;
    const HJ_LDS uint8_t* zz;
    static constexpr uint32_t kCursorStep = 1;  // the cursor is the word index
    __device__ __forceinline__ uint32_t cursor(uint32_t i) const { return i; }
    __device__ __forceinline__ uint32_t fetch(uint32_t i) const { return word(i); }
    // The lanes read the stream through the vector cache: a unit's span is ~7 KB and every word is needed by one or two neighbouring
    // lanes, the prefetch in the bit reader covers the latency, and LDS is what limits the waves (staging 4096 words per 256 lanes was
    // measured at 959 us against 771 us without, 256 x 1080p).
    __device__ __forceinline__ uint32_t word(uint32_t i) const
    {
        // unconditional load from a clamped index, selection afterwards: the request leaves at the top of the decode step and
        // nothing waits for it before the value is consumed at the bottom
        // (byte offset in 32 bits -- a stream is far below 4 GB: SGPR base + VGPR offset addressing)
        const uint32_t x = *(const HJ_GLOBAL uint32_t*)((const HJ_GLOBAL char*)gstream + (min(i, gwords - 1) << 2));
        return i < gwords ? __builtin_bswap32(x) : ~0u;
    }
    __device__ __forceinline__ int16_t* block_ptr(int k, uint32_t mx, uint32_t my) const
    {
        const HJ_LDS KSlot* s = kslot + k;
        int16_t* base = s->base;
        const uint32_t sy = s->stride_y, sx = s->stride_x;
        return base + (size_t)(my * sy + mx * sx) * 64;
    }
    // decode_block hands zigzag()'s value to put(): here it is the coefficient's byte offset in the block, not its index
    __device__ __forceinline__ int zigzag(int z) const { return zz[z]; }
    __device__ __forceinline__ void put(int byte_offset, int value) const { *(HJ_LDS int16_t*)(uintptr_t)(buf ^ (uint32_t)byte_offset) = (int16_t)value; }
};

// (kBThreads, 4): four waves per SIMD, i.e. at most 128 VGPRs -- two workgroups of eight waves on a CU's four SIMDs
__global__ __launch_bounds__(kBThreads, 4) void huff_blocks_kernel(HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                                   uint32_t nunits, int32_t* __restrict__ group_sums)
{
    __shared__ BlockShared sh;
    extern __shared__ uint16_t dyn_pool[];
    HJ_LDS uint16_t* pool = (HJ_LDS uint16_t*)dyn_pool;
    // Workgroup w looks at unit (w % H) * kBTeams + w / H, H = gridDim.x / kBTeams: the first H workgroups at every kBTeams-th unit,
    // which is where the workgroups with work are unless images with an odd number of units have shifted them -- the ones that
    // leave at once come behind them and pass through the slots the last working ones free.  (Workgroups go to the chip's eight
    // XCDs in turn: with unit w for workgroup w the working ones, every second, all landed on four of them -- twice the time.)
    const uint32_t per_team = gridDim.x / (uint32_t)kBTeams;
    const uint32_t unit0 = (blockIdx.x % per_team) * (uint32_t)kBTeams + blockIdx.x / per_team;
    if (unit0 >= nunits) return;
    const HuffUnit u0 = units[unit0];  // first = first MCU of a unit (kHuffMcusPerWg MCUs)
    // the unit is a second team's: the workgroup of the unit in front of it takes it (uniform: the whole workgroup leaves)
    if ((u0.first / (uint32_t)kHuffMcusPerWg) % (uint32_t)kBTeams != 0) return;
    HuffImage& im = images[u0.image];
    const HuffGeom geom = make_geom(im);
    const uint32_t bpm = geom.blocks_per_mcu;
    const uint32_t nblocks = min(im.total_blocks, im.decoded_blocks);  // a truncated stream: the scan kernel has flagged it
    const uint32_t total_mcus = geom.mcus_x * geom.mcus_y;
    const int t = threadIdx.x, team = t / kBTeamThreads, tt = t % kBTeamThreads;
    // the team's unit is units[unit0 + team] = {u0.image, first} if the image has it
    const uint32_t first = u0.first + (uint32_t)team * kHuffMcusPerWg;
    const bool has_unit = first < total_mcus;
    const uint32_t b_first = first * bpm;
    // nothing to decode (no unit, or the decoded blocks end in front of it): no items, but every barrier below
    const uint32_t mcus = has_unit && b_first < nblocks ? min((uint32_t)kHuffMcusPerWg, total_mcus - first) : 0u;
    const uint32_t items = mcus * bpm;
    if (t < 4 * kBTeams) sh.dc_sum[t >> 2][t & 3] = 0;
    if (t >= 32 && t < 42) sh.kcomp[t - 32] = im.k[t - 32].comp & 3;
    stage_pool<kBThreads>(pool, im);
    stage_constants(sh.tsel, sh.kslot, sh.zz, im, true);
    // The zero fill goes through the swizzle like every other access to the buffers: step i clears chunk i ^ (t & 7).  A 16-byte LDS
    // store is served in groups of eight consecutive lanes on 32 banks (128 bytes): chunk i of every lane, 128 bytes apart, puts the
    // eight lanes of a group on the same four banks -- 64 LDS cycles per store where the swizzled one takes 8, eight stores per round
    // (profiles/block_pass_residency/).
    const uint32_t my_buf = (uint32_t)(uintptr_t)(HJ_LDS uint8_t*)sh.blocks + (((uint32_t)t * kBlockBufBytes) | (((uint32_t)t & 7u) << 4));
    auto zero_fill = [my_buf] {
#pragma unroll
        for (uint32_t i = 0; i < kBlockBufBytes / 16; i++) *(HJ_LDS u32x4*)(uintptr_t)(my_buf ^ (i << 4)) = u32x4{0u, 0u, 0u, 0u};
    };
    zero_fill();
    __syncthreads();  // barrier 1 of 2: tables, constants and zeroed sums are in place
    BlockEnv env;
    env.gstream = reinterpret_cast<const uint32_t*>(im.stream);
    env.gwords = im.stream_words;
    env.pool = (uint32_t)(uintptr_t)pool;
    env.buf = my_buf;
    env.tsel = (const HJ_LDS uint32_t*)sh.tsel;
    env.kslot = (const HJ_LDS KSlot*)sh.kslot;
    env.zz = (const HJ_LDS uint8_t*)sh.zz;
    uint32_t err = 0;
    // Between the steps of a round a wave waits for its own lanes only (wave_sync: LDS operations of a wave complete in order).  The
    // trip count is a team's own; nothing in the loop waits for another wave.
    static_assert(kBTeamThreads % 64 == 0, "whole waves: lane t flushes the buffers of lanes (t & ~63) ...");
    // Work items are ordered by MCU position first: item i is position i / mcus of MCU i % mcus, so that the 256 lanes of
    // a round hold blocks of the same component -- luma blocks run ~4x longer than chroma blocks, and a wave takes as long
    // as its longest block.
    for (uint32_t base = 0; base < items; base += kBTeamThreads) {
        wave_sync();  // zeroed buffers are in place
        const uint32_t item = base + tt;
        int16_t* dst = nullptr;
        if (item < items) {
            const uint32_t k = item / mcus, mcu = first + (item - k * mcus);
            const uint32_t b = mcu * bpm + k;
            if (b < nblocks) {
                const uint32_t my = mcu / geom.mcus_x, mx = mcu - my * geom.mcus_x;
                dst = env.block_ptr((int)k, mx, my);
                const uint32_t bpos = im.block_pos[b];
                // restart intervals: the first block of interval j+1 starts exactly at boundary j -- anything else means
                // the trajectory went through a damaged interval (the host decoder takes the image and names the error)
                if (geom.interval_blocks != 0 && k == 0 && b != 0 && b % geom.interval_blocks == 0 &&
                    bpos != load_boundary(geom.boundaries, geom.num_boundaries, b / geom.interval_blocks - 1))
                    err = 1;
                const int dc = decode_block(geom, env, bpos, (int)k, &err);
                ((HJ_GLOBAL int16_t*)geom.dc_diff)[b] = (int16_t)dc;
                atomicAdd(&sh.dc_sum[team][sh.kcomp[k]], (int)(int16_t)dc);
            }
        }
        wave_sync();
        // eight lanes per block, 16 bytes each: every store instruction writes eight whole lines.  Lane 8 * i + j of the wave holds
        // the destination of the block that lanes 8 * j .. 8 * j + 7 store in step i; chunk c of lane L's buffer sits at unit c ^ (L & 7).
        const uint32_t dst_lo = (uint32_t)(uintptr_t)dst, dst_hi = (uint32_t)((uintptr_t)dst >> 32);
        const int lane = t & 63, chunk = t & 7;
        // (all cross-lane reads, then all buffer reads -- a wave's own buffers, readable whether or not the block exists -- then the
        // stores: the LDS round trips overlap instead of following each other)
        int16_t* p[8];
        u32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int src = 8 * i + (lane >> 3);
            const uint32_t lo = (uint32_t)__shfl((int)dst_lo, src, 64), hi = (uint32_t)__shfl((int)dst_hi, src, 64);
            p[i] = (int16_t*)(((uintptr_t)hi << 32) | lo);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int blk = (t & ~63) + 8 * i + (lane >> 3);
            v[i] = *(const HJ_LDS u32x4*)&sh.blocks[blk * kBlockBufBytes + ((chunk ^ (blk & 7)) << 4)];
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (p[i]) __builtin_nontemporal_store(v[i], (HJ_GLOBAL u32x4*)p[i] + chunk);
        if (base + kBTeamThreads < items) {
            wave_sync();
            zero_fill();
        }
    }
    if (err) im.status = 1;  // benign race: every writer stores the same value
    __syncthreads();         // barrier 2 of 2: every team arrives, with or without items
    if (has_unit && tt < 4) group_sums[(size_t)(unit0 + team) * 4 + tt] = sh.dc_sum[team][tt];
}

// ---- fused decode (round 3): the DC differences alone ------------------------------------------------------------------------
// When the pixel kernels decode the coefficient blocks themselves (decode_kernels.hip, FUSED builds: Huffman decode into the LDS
// slots the IDCT reads, no coefficient ever reaches HBM), the block pass above is not launched.  What remains of it is this: one
// lane per block reads the block's FIRST symbol -- its DC difference -- at the recorded start position, so that the DC pass can
// integrate the predictors before the pixel kernels run.  Table lookups go to memory through the vector cache (one or two per
// block; staging the tables in LDS would cost more than it saves).  Same work units and group sums as the block pass; also the
// restart-interval check of the block pass (an interval's first block starts exactly at its boundary).
__global__ __launch_bounds__(kThreads) void huff_dcdiff_kernel(HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                              int32_t* __restrict__ group_sums)
{
    __shared__ int32_t s_sum[4];
    __shared__ uint32_t s_tdc[10], s_comp[10];
    const HuffUnit u = units[blockIdx.x];  // first = first MCU of the workgroup's kHuffMcusPerWg MCUs
    HuffImage& im = images[u.image];
    const HuffGeom geom = make_geom(im);
    const uint32_t bpm = geom.blocks_per_mcu;
    const uint32_t nblocks = min(im.total_blocks, im.decoded_blocks);
    const uint32_t b_first = u.first * bpm;
    const int t = threadIdx.x;
    if (t < 4) s_sum[t] = 0;
    if (t >= 32 && t < 42) {
        s_tdc[t - 32] = im.k[t - 32].tdc;
        s_comp[t - 32] = im.k[t - 32].comp & 3;
    }
    __syncthreads();
    if (b_first < nblocks) {
        const uint32_t mcus = min((uint32_t)kHuffMcusPerWg, geom.mcus_x * geom.mcus_y - u.first);
        const uint32_t items = mcus * bpm;
        const HJ_GLOBAL uint32_t* g = (const HJ_GLOBAL uint32_t*)im.stream;
        const HJ_GLOBAL uint16_t* pool = (const HJ_GLOBAL uint16_t*)im.pool;
        const uint32_t gwords = im.stream_words;
        uint32_t err = 0;
        for (uint32_t item = t; item < items; item += kThreads) {
            const uint32_t b = b_first + item;
            if (b >= nblocks) break;
            const uint32_t k = item % bpm;
            const uint32_t bpos = im.block_pos[b];
            if (geom.interval_blocks != 0 && k == 0 && b != 0 && b % geom.interval_blocks == 0 &&
                bpos != load_boundary(geom.boundaries, geom.num_boundaries, b / geom.interval_blocks - 1))
                err = 1;
            const uint32_t i = bpos >> 5, sft = bpos & 31;
            const uint32_t w0 = i < gwords ? __builtin_bswap32(g[i]) : ~0u, w1 = i + 1 < gwords ? __builtin_bswap32(g[i + 1]) : ~0u;
            const uint32_t w = sft ? (w0 << sft) | (w1 >> (32 - sft)) : w0;
            uint32_t e = pool[s_tdc[k] + (w >> (32 - kHuffFastBits))];
            if ((e >> 9) == kZadvLong) e = pool[((e & 0x1FFu) << 6) + ((w >> (32 - kHuffFastBits - kHuffSubBits)) & ((1u << kHuffSubBits) - 1))];
            const uint32_t total = e & 31u, nb_raw = (e >> 5) & 15u;
            const bool bad = nb_raw >= total;
            const uint32_t nb = bad ? 0u : nb_raw;
            const uint32_t v = nb ? (w << (total - nb)) >> (32 - nb) : 0u;
            const uint32_t m = (1u << nb) - 1u;
            const int dc = (v << 1) <= m ? (int)v - (int)m : (int)v;
            if (bad || bpos + total > geom.total_bits) err = 1;
            ((HJ_GLOBAL int16_t*)geom.dc_diff)[b] = (int16_t)dc;
            atomicAdd(&s_sum[s_comp[k]], (int)(int16_t)dc);
        }
        if (err) im.status = 1;  // benign race: every writer stores the same value
    }
    __syncthreads();
    if (t < 4) group_sums[(size_t)blockIdx.x * 4 + t] = s_sum[t];
}

// ---- DC differences -> DC values ------------------------------------------------------------------------------------------
// Images without restart intervals: one workgroup per block-pass unit (kHuffMcusPerWg MCUs).  The predictor value a group
// starts from is the sum of the group sums in front of it (the block pass left them: a few dozen numbers), so every group
// integrates its own MCUs without waiting for anybody.  A lane takes whole consecutive MCUs of one component: it adds their entries
// serially, ONE wave scan runs over the lane totals, and the lane walks its entries again to store them -- no division per entry (the
// block's place inside the MCU advances with the entry, the MCU's place in the image is divided out once per lane), and the scan's
// six shuffle steps once per wave instead of once per 64 entries (at 4:2:0 the luma wave ran eight scans and three divisions per
// entry back to back, 50 us per 256 x 1080p; 38 us with the lanes' MCUs, 31 with the group's loads in flight together:
// profiles/entropy_residue2/).
//
// This is the last kernel of the stage that every image passes, and nothing behind it changes a verdict: the group at an image's MCU 0
// reports the image (huff_verdict(): status, gave_up), the first workgroup the stage's convergence counters, into
// `verdicts` -- the host's pinned memory where that is mapped (kHuffVerdictCounters words of counters, then a word per image), so that
// no copy command has to follow the stage.
constexpr bool kDcSplit = kHuffMcusPerWg % 128 == 0;  // component 0's MCUs can go to two waves, whole MCUs to every lane
constexpr uint32_t kDcLaneMcus = kHuffMcusPerWg / 64;  // MCUs a lane takes at most
static_assert(kHuffMcusPerWg % 64 == 0, "huff_dc_group_kernel: the same number of MCUs for every lane of a wave");

// The lane's `live` MCUs of one component, `bpc` entries each (BPC: the same at compile time, 0 = any), the first at d, the next bpm
// entries on: their sum ...
template <uint32_t BPC>
__device__ __forceinline__ int dc_lane_total(const int16_t* d, uint32_t live, uint32_t bpc, uint32_t bpm)
{
    const uint32_t nb = BPC ? BPC : bpc;
    int sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kDcLaneMcus; q++) {
        if (q < live) {
#pragma unroll
            for (uint32_t jj = 0; jj < nb; jj++) sum += d[q * bpm + jj];
        }
    }
    return sum;
}

// ... and their running sums from `run` on, stored to the component's DC plane (h x v blocks per MCU, row-major; the lane's first MCU
// is (mx, my) of the image's mcus_x columns).
template <uint32_t BPC>
__device__ __forceinline__ void dc_lane_store(const int16_t* d, HJ_GLOBAL int16_t* plane, int run, uint32_t live, uint32_t bpc, uint32_t bpm,
                                              uint32_t h, uint32_t v, uint32_t bw, uint32_t mx, uint32_t my, uint32_t mcus_x)
{
    const uint32_t nb = BPC ? BPC : bpc;
#pragma unroll
    for (uint32_t q = 0; q < kDcLaneMcus; q++) {
        if (q < live) {
            HJ_GLOBAL int16_t* p = plane + (my * v) * bw + mx * h;  // the MCU's first block; dx counts along its row of h blocks
            uint32_t dx = 0;
#pragma unroll
            for (uint32_t jj = 0; jj < nb; jj++) {
                run += d[q * bpm + jj];
                p[dx] = (int16_t)run;
                if (++dx == h) {
                    dx = 0;
                    p += bw;
                }
            }
            if (++mx == mcus_x) {
                mx = 0;
                my++;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void huff_dc_group_kernel(const HuffImage* __restrict__ images, const HuffUnit* __restrict__ units,
                                                                 const int32_t* __restrict__ group_sums, const unsigned int* __restrict__ counters,
                                                                 unsigned int* __restrict__ verdicts)
{
    __shared__ int16_t s_diff[kHuffMcusPerWg * 10];
    __shared__ int s_base[4];
    __shared__ int s_half;
    const HuffUnit u = units[blockIdx.x];  // first = first MCU of the group
    const HuffImage& im = images[u.image];
    if (verdicts) {
        if (blockIdx.x == 0 && threadIdx.x < kHuffVerdictCounters) verdicts[threadIdx.x] = counters[threadIdx.x];
        if (u.first == 0 && threadIdx.x == 64) verdicts[kHuffVerdictCounters + u.image] = huff_verdict(im.status, im.gave_up);
    }
    if (im.restart_interval != 0) return;  // uniform: huff_dc_kernel takes those
    const int t = threadIdx.x;
    const uint32_t bpm = im.blocks_per_mcu;
    const uint32_t mcus_x = im.mcus_x, total_mcus = mcus_x * im.mcus_y;
    const uint32_t mcus = min((uint32_t)kHuffMcusPerWg, total_mcus - u.first);
    const uint32_t n = mcus * bpm;
    const uint32_t g = u.first / kHuffMcusPerWg;  // groups in front of this one: units blockIdx.x - g .. blockIdx.x - 1
    if (t < 4) s_base[t] = 0;
    // (the group sums are fetched beside the differences, one round of memory latency for both; they meet in s_base behind the
    // barrier and are read behind the next one, the one the lane totals need anyway)
    const HJ_GLOBAL int32_t* sums = (const HJ_GLOBAL int32_t*)group_sums + (size_t)(blockIdx.x - g) * 4;
    int part = (uint32_t)t < g * 4 ? sums[t] : 0;  // i & 3 = t & 3: a lane stays with one component
    {
        // all of a lane's loads in flight together (a loop of load and store waited for every one of them in turn)
        const HJ_GLOBAL int16_t* diff = (const HJ_GLOBAL int16_t*)im.dc_diff + (size_t)u.first * bpm;
        constexpr uint32_t kLoads = (kHuffMcusPerWg * 10 + kThreads - 1) / kThreads;
        int16_t e[kLoads];
#pragma unroll
        for (uint32_t k = 0; k < kLoads; k++) e[k] = k * kThreads + t < n ? diff[k * kThreads + t] : (int16_t)0;
#pragma unroll
        for (uint32_t k = 0; k < kLoads; k++)
            if (k * kThreads + t < n) s_diff[k * kThreads + t] = e[k];
    }
    for (uint32_t i = t + kThreads; i < g * 4; i += kThreads) part += sums[i];  // (images of more than 64 groups)
    __syncthreads();
    if (part != 0) atomicAdd(&s_base[t & 3], part);
    // Wave w takes component w; where the frame leaves the fourth wave free (up to three components) it takes the second half of
    // component 0's MCUs -- at 4:2:0 luma has four of an MCU's six entries.  A lane owns whole, consecutive MCUs.
    const int wave = t >> 6, lane = t & 63;
    const bool split = kDcSplit && im.ncomp <= 3;
    const bool helper = split && wave == 3;
    const int c = helper ? 0 : wave;
    const bool active = c < (int)im.ncomp;
    const uint32_t per_lane = split && c == 0 ? kHuffMcusPerWg / 128 : kHuffMcusPerWg / 64;
    const uint32_t m0 = ((helper ? 64u : 0u) + (uint32_t)lane) * per_lane;
    const uint32_t live = active && m0 < mcus ? min(per_lane, mcus - m0) : 0u;
    uint32_t h = 1, v = 1, bpc = 1, bw = 0, mx = 0, my = 0;
    const int16_t* d = s_diff;
    HJ_GLOBAL int16_t* plane = nullptr;
    int x = 0;
    if (active) {
        h = im.comp_h[c], v = im.comp_v[c], bpc = h * v, bw = im.blocks_w[c];
        d = s_diff + m0 * bpm + im.comp_k0[c];
        plane = (HJ_GLOBAL int16_t*)im.dc_plane[c];
        my = (u.first + m0) / mcus_x, mx = (u.first + m0) - my * mcus_x;
        x = bpc == 1 ? dc_lane_total<1>(d, live, bpc, bpm) : bpc == 2 ? dc_lane_total<2>(d, live, bpc, bpm)
          : bpc == 4 ? dc_lane_total<4>(d, live, bpc, bpm) : dc_lane_total<0>(d, live, bpc, bpm);
    }
    const int own = x;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int y = __shfl_up(x, s, 64);
        if (lane >= s) x += y;
    }
    if (split && wave == 0 && lane == 63) s_half = x;  // component 0's first half, for the wave that takes the second
    __syncthreads();
    if (!active) return;
    const int run = s_base[c] + (helper ? s_half : 0) + (x - own);
    if (bpc == 1) dc_lane_store<1>(d, plane, run, live, bpc, bpm, h, v, bw, mx, my, mcus_x);
    else if (bpc == 2) dc_lane_store<2>(d, plane, run, live, bpc, bpm, h, v, bw, mx, my, mcus_x);
    else if (bpc == 4) dc_lane_store<4>(d, plane, run, live, bpc, bpm, h, v, bw, mx, my, mcus_x);
    else dc_lane_store<0>(d, plane, run, live, bpc, bpm, h, v, bw, mx, my, mcus_x);
}

// Images with restart intervals (the predictor starts over inside the image): one workgroup per (image, component)
// integrates the DC differences in MCU order; DC values go to the component's compact
// DC plane (raster block order), which the IDCT kernels read beside the coefficient blocks.
__global__ __launch_bounds__(kThreads) void huff_dc_kernel(const HuffImage* __restrict__ images, const HuffUnit* __restrict__ units)
{
    __shared__ int s_sum[kThreads];
    __shared__ int s_flag[kThreads];
    const HuffUnit u = units[blockIdx.x];  // first = component
    const HuffImage& im = images[u.image];
    const int c = (int)u.first;
    const uint32_t h = im.comp_h[c], v = im.comp_v[c], bpc = h * v;  // blocks of this component per MCU
    const uint32_t bpm = im.blocks_per_mcu, k0 = im.comp_k0[c];
    const uint32_t mcus = im.mcus_x * im.mcus_y;
    const uint32_t n = mcus * bpc;
    HJ_GLOBAL int16_t* plane = (HJ_GLOBAL int16_t*)im.dc_plane[c];
    const HJ_GLOBAL int16_t* diff = (const HJ_GLOBAL int16_t*)im.dc_diff;
    const uint32_t bw = im.blocks_w[c], mcus_x = im.mcus_x;
    // restart intervals: the predictor starts over every `seg` entries of the component (0xFFFFFFFF: never)
    const uint32_t seg = im.restart_interval ? im.restart_interval * bpc : 0xFFFFFFFFu;
    // entry s of the component (MCU order) sits at diff[(s / bpc) * bpm + k0 + s % bpc]; every lane takes a contiguous run
    const uint32_t per = (n + kThreads - 1) / kThreads;
    const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    auto index_of = [&](uint32_t s) {
        const uint32_t mcu = s / bpc;
        return mcu * bpm + k0 + (s - mcu * bpc);
    };
    constexpr int kBatch = 8;  // independent loads in flight per lane
    // per lane: the running sum at the end of its run (since the last restart inside the run, if any)
    int sum = 0, flag = 0;
    uint32_t until = lo < hi ? (seg == 0xFFFFFFFFu ? 0xFFFFFFFFu : (seg - lo % seg) % seg) : 0xFFFFFFFFu;  // entries until the next restart
    for (uint32_t s = lo; s < hi; s += kBatch) {
        int d[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++) d[i] = s + i < hi ? (int)diff[index_of(s + i)] : 0;
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            if (s + i < hi) {
                if (until == 0) {
                    sum = 0;
                    flag = 1;
                    until = seg;
                }
                until--;
            }
            sum += d[i];
        }
    }
    s_sum[threadIdx.x] = sum;
    s_flag[threadIdx.x] = flag;
    __syncthreads();
    // segmented inclusive scan over the lanes: (a, fa) . (b, fb) = fb ? (b, 1) : (a + b, fa)
    for (int off = 1; off < kThreads; off <<= 1) {
        int a = 0, fa = 0;
        if (threadIdx.x >= (unsigned)off) {
            a = s_sum[threadIdx.x - off];
            fa = s_flag[threadIdx.x - off];
        }
        __syncthreads();
        if (threadIdx.x >= (unsigned)off && !s_flag[threadIdx.x]) {
            s_sum[threadIdx.x] += a;
            s_flag[threadIdx.x] = fa;
        }
        __syncthreads();
    }
    int run = threadIdx.x ? s_sum[threadIdx.x - 1] : 0;
    until = lo < hi ? (seg == 0xFFFFFFFFu ? 0xFFFFFFFFu : (seg - lo % seg) % seg) : 0xFFFFFFFFu;
    for (uint32_t s = lo; s < hi; s += kBatch) {
        int d[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++) d[i] = s + i < hi ? (int)diff[index_of(s + i)] : 0;
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            if (s + i < hi) {
                if (until == 0) {
                    run = 0;
                    until = seg;
                }
                until--;
                run += d[i];
                const uint32_t mcu = (s + i) / bpc, jj = (s + i) - mcu * bpc;
                const uint32_t my = mcu / mcus_x, mx = mcu - my * mcus_x;
                const uint32_t dy = jj / h, dx = jj - dy * h;
                plane[(my * v + dy) * bw + (mx * h + dx)] = (int16_t)run;
            }
        }
    }
}

}  // namespace

int launch_gather_raw(const HuffImage* images, const HuffUnit* chunk_units, int nchunks, void* stream)
{
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(gather_raw_kernel, dim3(min(nchunks, kGatherGroups)), dim3(kThreads), 0, (hipStream_t)stream, images, chunk_units, nchunks);
    return (int)hipGetLastError();
}

int launch_destuff(HuffImage* images, const HuffUnit* chunk_units, int nchunks, uint32_t* drops, bool count_on_device, unsigned int* counters,
                   void* stream)
{
    if (nchunks <= 0) return 0;
    if (count_on_device)
        hipLaunchKernelGGL(destuff_count_kernel, dim3(nchunks), dim3(kThreads), 0, (hipStream_t)stream, images, chunk_units, drops);
    hipLaunchKernelGGL(destuff_compact_kernel, dim3(nchunks), dim3(kThreads), 0, (hipStream_t)stream, images, chunk_units, drops, counters);
    return (int)hipGetLastError();
}

// HIPJPEG_RIPPLE_IN_SYNC=1: the second and later launches use the sync kernel's ripple branch as in round 1 (A/B aid)
static bool ripple_in_tail_kernel()
{
    static const bool v = getenv("HIPJPEG_RIPPLE_IN_SYNC") == nullptr;
    return v;
}

int launch_huff_sync(HuffImage* images, const HuffUnit* units, int nunits, const uint32_t* pairs, int npairs, unsigned long long* states,
                     unsigned long long* incoming, unsigned int* changed, int first_pass, int max_rounds, uint16_t* tail_tasks, uint32_t* tail_count,
                     uint16_t* records, unsigned pool_bytes, void* stream, unsigned pass_id)
{
    if (nunits <= 0 || (first_pass && npairs <= 0)) return 0;
    const dim3 tail_grid((nunits + kTailWaves - 1) / kTailWaves);
    if (!first_pass && ripple_in_tail_kernel()) {
        // corrections across group borders: the tail kernel's workgroups (little LDS, a row staged per decode) instead of the
        // sync kernel's, which would stage 255 rows to decode one or two
        hipLaunchKernelGGL(huff_tail_kernel<true>, tail_grid, dim3(kTailThreads), pool_bytes, (hipStream_t)stream, images, units, nunits, states, incoming,
                           changed, nullptr, nullptr, pass_id, records);
        return (int)hipGetLastError();
    }
    if (first_pass)  // two units per workgroup, the paired schedule
        hipLaunchKernelGGL(huff_sync_pair_kernel, dim3(npairs), dim3(kSyncThreads), pool_bytes, (hipStream_t)stream, images, units, pairs, states, incoming,
                           changed, max_rounds, tail_tasks, tail_count, records);
    else  // HIPJPEG_RIPPLE_IN_SYNC=1: the ripple over single units
        hipLaunchKernelGGL(huff_sync_kernel, dim3(nunits), dim3(kSyncThreads), pool_bytes, (hipStream_t)stream, images, units, states, incoming, changed,
                           records);
    if (tail_count)
        hipLaunchKernelGGL(huff_tail_kernel<false>, tail_grid, dim3(kTailThreads), pool_bytes, (hipStream_t)stream, images, units, nunits, states, incoming,
                           changed, tail_tasks, tail_count, 0u, records);
    return (int)hipGetLastError();
}

int launch_huff_write(HuffImage* images, const HuffUnit* sync_units, int nsync_units, const HuffUnit* block_units, int nblock_units,
                      const unsigned long long* states, uint32_t* first_block, const uint16_t* records, uint32_t* walkers, int32_t* group_sums,
                      unsigned pool_bytes, void* stream, bool dc_only)
{
    if (nsync_units <= 0) return 0;
    hipLaunchKernelGGL(huff_copy_records_kernel, dim3(nsync_units), dim3(kSyncThreads), 0, (hipStream_t)stream, images, sync_units, states, first_block,
                       records, walkers);
    hipLaunchKernelGGL(huff_pos_kernel, dim3(nsync_units), dim3(kSyncThreads), pool_bytes, (hipStream_t)stream, images, sync_units, states, first_block,
                       records, walkers);
    if (nblock_units > 0) {
        if (dc_only)
            hipLaunchKernelGGL(huff_dcdiff_kernel, dim3(nblock_units), dim3(kThreads), 0, (hipStream_t)stream, images, block_units, group_sums);
        else
            hipLaunchKernelGGL(huff_blocks_kernel, dim3((nblock_units + kBTeams - 1) / kBTeams * kBTeams), dim3(kBThreads), pool_bytes, (hipStream_t)stream,
                               images, block_units, (uint32_t)nblock_units, group_sums);
    }
    return (int)hipGetLastError();
}

int launch_huff_dc(const HuffImage* images, const HuffUnit* rst_units, int nrst_units, const HuffUnit* block_units, int nblock_units,
                   const int32_t* group_sums, const unsigned int* counters, unsigned int* verdicts, void* stream)
{
    if (nblock_units > 0)
        hipLaunchKernelGGL(huff_dc_group_kernel, dim3(nblock_units), dim3(kThreads), 0, (hipStream_t)stream, images, block_units, group_sums, counters,
                           verdicts);
    if (nrst_units > 0) hipLaunchKernelGGL(huff_dc_kernel, dim3(nrst_units), dim3(kThreads), 0, (hipStream_t)stream, images, rst_units);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
