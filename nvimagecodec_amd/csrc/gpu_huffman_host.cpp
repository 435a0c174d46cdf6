// gpu_huffman_host.cpp -- see gpu_huffman_host.h
#include "gpu_huffman_host.h"
#include "scratch_fill.h"

#include <algorithm>
#include <cstring>

namespace hipjpeg {

uint32_t scan_mcus_x(const FrameInfo& f, const ScanHeader& sc)
{
    return (uint32_t)(sc.ncomp == 1 ? (f.comp[sc.comp_index[0]].samp_w + 7) / 8 : f.mcus_x);
}

uint32_t scan_mcus_y(const FrameInfo& f, const ScanHeader& sc)
{
    return (uint32_t)(sc.ncomp == 1 ? (f.comp[sc.comp_index[0]].samp_h + 7) / 8 : f.mcus_y);
}

uint32_t scan_blocks_per_mcu(const FrameInfo& f, const ScanHeader& sc)
{
    if (sc.ncomp == 1) return 1;
    uint32_t n = 0;
    for (int i = 0; i < sc.ncomp; i++) n += (uint32_t)(f.comp[sc.comp_index[i]].h * f.comp[sc.comp_index[i]].v);
    return n;
}

namespace {
// One scan of a sequential frame: plain stuffing, every restart interval closed by its marker, tables present and expandable, at
// most 10 blocks per MCU, bit positions that fit 32 bits.
bool gpu_scan_eligible(const FrameInfo& f, const ScanHeader& sc)
{
    if (sc.ncomp < 1 || !sc.plain_stuffing) return false;
    {
        // restart intervals: every interval but the last must be closed by its marker (RST0..7 in order: plain_stuffing)
        const size_t mcus = (size_t)scan_mcus_x(f, sc) * scan_mcus_y(f, sc);
        const size_t expect = sc.restart_interval ? (mcus + sc.restart_interval - 1) / sc.restart_interval - 1 : 0;
        if (sc.rst_after.size() != expect) return false;
    }
    for (int i = 0; i < sc.ncomp; i++)
        if (!sc.dc[sc.td[i]].present || !sc.ac[sc.ta[i]].present) return false;
    if (scan_blocks_per_mcu(f, sc) > 10) return false;
    if ((sc.data_end - sc.data_begin) >= (1ull << 28)) return false;  // bit positions are 32-bit
    const size_t words = gpu_pool_words(sc);
    return words != 0 && words <= (size_t)kMaxPoolWords;
}
}  // namespace

bool gpu_entropy_eligible(const FrameInfo& f)
{
    if (f.progressive() || f.scans.empty() || f.scans.size() > (size_t)kMaxSeqScans) return false;
    // every component in exactly one scan: the scans then write disjoint components and each starts its own DC prediction, so they
    // are independent streams (a component no scan codes, or one coded twice, keeps the host decoder's verdict)
    int coded[4] = {0, 0, 0, 0};
    for (const ScanHeader& sc : f.scans) {
        if (!gpu_scan_eligible(f, sc)) return false;
        for (int i = 0; i < sc.ncomp; i++) coded[sc.comp_index[i]]++;
    }
    for (int c = 0; c < f.ncomp; c++)
        if (coded[c] != 1) return false;
    return true;
}

size_t destuff_scan(const uint8_t* data, const ScanHeader& sc, uint8_t* out)
{
    const uint8_t* p = data + sc.data_begin;
    const uint8_t* end = data + sc.data_end;
    uint8_t* o = out;
    while (p < end) {
        const uint8_t* ff = static_cast<const uint8_t*>(memchr(p, 0xFF, (size_t)(end - p)));
        if (!ff) {
            memcpy(o, p, (size_t)(end - p));
            o += end - p;
            break;
        }
        memcpy(o, p, (size_t)(ff - p));
        o += ff - p;
        p = ff + 1;
        while (p < end && *p == 0xFF) p++;  // fill bytes
        if (p < end && *p == 0x00) {
            *o++ = 0xFF;
            p++;
        } else if (p < end && *p >= 0xD0 && *p <= 0xD7) {
            p++;  // restart marker: dropped; the interval behind it starts at this (byte-aligned) position
        } else {
            break;  // another marker (cannot happen before data_end) or the end
        }
    }
    const size_t n = (size_t)(o - out);
    memset(o, 0xFF, kStreamSlackBytes + ((4 - (n & 3)) & 3));  // whole 32-bit words stay readable past the end
    return n;
}

namespace {

// Walks the canonical code of `s`; calls fn(length, code, symbol) for every code.  False if the code is over-subscribed.
template <class Fn>
bool for_each_code(const HuffSpec& s, Fn fn)
{
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < s.bits[l]; i++, k++, code++) {
            if (code >= (1u << l) || k >= 256) return false;
            fn(l, code, s.vals[k]);
        }
        code <<= 1;
    }
    return true;
}

// entries of one table: first level + second-level tables; 0 = malformed
size_t table_words(const HuffSpec& s, bool is_dc)
{
    if (!s.present) return 0;
    std::vector<uint8_t> has_sub(1u << kHuffFastBits, 0);
    size_t words = (1u << kHuffFastBits) + (is_dc ? 0u : kPairOffset);  // AC: first level + pair table
    bool bad = false;
    bool ok = for_each_code(s, [&](int l, uint32_t code, uint8_t sym) {
        if (is_dc && sym > 15) bad = true;
        if (l > kHuffFastBits) {
            const uint32_t prefix = code >> (l - kHuffFastBits);
            if (!has_sub[prefix]) {
                has_sub[prefix] = 1;
                words += 1u << kHuffSubBits;
            }
        }
    });
    return ok && !bad ? words : 0;
}

// Expands one table at pool[base...] (base is a multiple of 64); returns the number of entries used.
size_t expand_table(const HuffSpec& s, bool is_dc, uint16_t* pool, size_t base)
{
    uint16_t* first = pool + base;
    for (int i = 0; i < (1 << kHuffFastBits); i++) first[i] = (uint16_t)kEntryInvalid;
    size_t used = (1u << kHuffFastBits) + (is_dc ? 0u : kPairOffset);
    for_each_code(s, [&](int l, uint32_t code, uint8_t sym) {
        const uint32_t nb = sym & 15u, run = sym >> 4;
        // DC: the symbol is the size category.  AC: (run, size); size 0 is EOB except for run 15 (ZRL, 16 zeros) -- libjpeg
        // treats every other run with size 0 as EOB too (jdhuff.c decode_mcu: "if (r != 15) break").
        const uint32_t zadv = is_dc ? 1u : (nb ? run + 1 : (run == 15 ? 16u : 64u));
        const uint16_t e = (uint16_t)make_entry((uint32_t)l + nb, nb, zadv);
        if (l <= kHuffFastBits) {
            const uint32_t lo = code << (kHuffFastBits - l);
            for (uint32_t j = 0; j < (1u << (kHuffFastBits - l)); j++) first[lo + j] = e;
        } else {
            const uint32_t prefix = code >> (l - kHuffFastBits);
            if ((first[prefix] >> 9) != kZadvLong) {  // still "no such code": open a second-level table
                first[prefix] = (uint16_t)(((base + used) / 64) | (kZadvLong << 9));
                for (int j = 0; j < (1 << kHuffSubBits); j++) pool[base + used + j] = (uint16_t)kEntryInvalid;
                used += 1u << kHuffSubBits;
            }
            uint16_t* sub = pool + (size_t)(first[prefix] & 0x1FFu) * 64;
            const uint32_t lo = (code & ((1u << (l - kHuffFastBits)) - 1)) << (16 - l);
            for (uint32_t j = 0; j < (1u << (16 - l)); j++) sub[lo + j] = e;
        }
    });
    if (!is_dc) {
        // pair table (huffman_gpu_core.h): window w = a first symbol of t1 bits and, in the 10 - t1 bits behind it, a whole second one
        uint16_t* pair = first + kPairOffset;
        for (uint32_t w = 0; w < (1u << kHuffFastBits); w++) {
            const uint32_t e1 = first[w], t1 = e1 & 31u, z1 = e1 >> 9;
            pair[w] = (uint16_t)e1;  // no pair here: the single step
            if (e1 == kEntryInvalid || z1 == kZadvLong || z1 == 64u || t1 + 2 > (uint32_t)kHuffFastBits) continue;
            const uint32_t e2 = first[(w << t1) & ((1u << kHuffFastBits) - 1)], t2 = e2 & 31u, z2 = e2 >> 9;
            if (e2 == kEntryInvalid || z2 == kZadvLong || t1 + t2 > (uint32_t)kHuffFastBits) continue;
            pair[w] = (uint16_t)make_pair_entry(t1 + t2, z2 == 64u ? 63u : z1 + z2);
        }
    }
    return used;
}

}  // namespace

size_t gpu_pool_words(const ScanHeader& sc)
{
    size_t words = 0;
    bool dc_seen[4] = {false, false, false, false}, ac_seen[4] = {false, false, false, false};
    for (int i = 0; i < sc.ncomp; i++) {
        const int td = sc.td[i], ta = sc.ta[i];
        if (!dc_seen[td]) {
            dc_seen[td] = true;
            const size_t w = table_words(sc.dc[td], true);
            if (!w) return 0;
            words += w;
        }
        if (!ac_seen[ta]) {
            ac_seen[ta] = true;
            const size_t w = table_words(sc.ac[ta], false);
            if (!w) return 0;
            words += w;
        }
    }
    return words;
}

void build_gpu_pool(const ScanHeader& sc, HuffImage* im, uint16_t* pool)
{
    size_t dc_off[4] = {0, 0, 0, 0}, ac_off[4] = {0, 0, 0, 0};
    bool dc_seen[4] = {false, false, false, false}, ac_seen[4] = {false, false, false, false};
    size_t used = 0;
    // DC tables first, AC tables behind them: the walkers read the pair-table slot (kPairOffset entries behind the first level)
    // of whatever table they are at -- behind a DC table that is some other table's entries, ignored, but inside the pool
    for (int i = 0; i < sc.ncomp; i++) {
        const int td = sc.td[i];
        if (!dc_seen[td]) {
            dc_seen[td] = true;
            dc_off[td] = used;
            used += expand_table(sc.dc[td], true, pool, used);
        }
    }
    for (int i = 0; i < sc.ncomp; i++) {
        const int ta = sc.ta[i];
        if (!ac_seen[ta]) {
            ac_seen[ta] = true;
            ac_off[ta] = used;
            used += expand_table(sc.ac[ta], false, pool, used);
        }
    }
    im->pool_words = (uint32_t)used;
    for (uint32_t k = 0; k < im->blocks_per_mcu; k++) {
        const int c = im->k[k].comp;
        im->k[k].tdc = (uint16_t)dc_off[sc.td[c]];
        im->k[k].tac = (uint16_t)ac_off[sc.ta[c]];
    }
}

bool pair_table_steps(const HuffSpec& ac, uint32_t* out)
{
    const size_t words = table_words(ac, false);
    if (!words || words > (size_t)kMaxPoolWords) return false;
    std::vector<uint16_t> pool(words);
    expand_table(ac, false, pool.data(), 0);
    for (uint32_t w = 0; w < (1u << kHuffFastBits); w++)
        for (uint32_t z = 0; z < 64; z++) {
            const uint32_t e = pool[w], pr = pool[kPairOffset + w];
            const bool two = pair_fits(z, e), lng = e >= (kZadvLong << 9);
            const uint32_t x = lng ? 0u : two ? pr : e;
            out[w * 64 + z] = (x & 31u) | ((x >> 9) << 8) | ((two && pr != e ? 1u : 0u) << 16) | ((lng ? 1u : 0u) << 17);
        }
    return true;
}

void fill_huff_image(const FrameInfo& f, const ScanHeader& sc, uint32_t stream_bytes, HuffImage* im)
{
    memset(im, 0, sizeof *im);
    im->total_bits = stream_bytes * 8u;
    im->num_subseq = (im->total_bits + kSubseqBits - 1) / kSubseqBits;
    im->stream_words = (uint32_t)((((size_t)stream_bytes + 3) & ~(size_t)3) + kStreamSlackBytes) / 4;
    // a one-component scan: one block per MCU over the component's real blocks (T.81 A.2.2), addressed through its padded grid
    im->mcus_x = scan_mcus_x(f, sc);
    im->mcus_y = scan_mcus_y(f, sc);
    im->ncomp = (uint32_t)sc.ncomp;
    int k = 0;
    for (int i = 0; i < sc.ncomp; i++) {  // slot i of the scan = frame component sc.comp_index[i]
        const Component& fc = f.comp[sc.comp_index[i]];
        const int h = sc.ncomp == 1 ? 1 : fc.h, v = sc.ncomp == 1 ? 1 : fc.v;
        im->comp_h[i] = (uint8_t)h;
        im->comp_v[i] = (uint8_t)v;
        im->comp_k0[i] = (uint8_t)k;
        im->blocks_w[i] = (uint32_t)fc.blocks_w;
        for (int dy = 0; dy < v; dy++)
            for (int dx = 0; dx < h; dx++, k++) {
                HuffK& hk = im->k[k];
                hk.comp = (uint8_t)i;
                hk.blk0 = (uint32_t)(dy * fc.blocks_w + dx);
                hk.stride_y = (uint32_t)(v * fc.blocks_w);
                hk.stride_x = (uint8_t)h;
            }
    }
    im->blocks_per_mcu = (uint32_t)k;
    im->total_blocks = im->mcus_x * im->mcus_y * (uint32_t)k;
}

namespace {
// plain-memory accessors for decode_subsequence
struct HostEnv {
    const HuffImage* im;
    static constexpr uint32_t kCursorStep = 1;  // the cursor is the word index
    uint32_t cursor(uint32_t i) const { return i; }
    uint32_t fetch(uint32_t i) const { return word(i); }
    uint32_t word(uint32_t i) const
    {
        const uint8_t* p = im->stream + (size_t)i * 4;  // the slack behind the stream covers the reader's look-ahead
        return i < im->stream_words ? ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3] : ~0u;
    }
    uint32_t boundary(uint32_t i) const { return i < im->num_boundaries ? im->boundaries[i] : 0xFFFFFFFFu; }
    uint32_t lookup1(uint32_t t, uint32_t w) const { return im->pool[t + (w >> (32 - kHuffFastBits))]; }
    uint32_t lookup2(uint32_t e, uint32_t w) const { return im->pool[(e & 0x1FFu) * 64u + ((w >> 16) & ((1u << kHuffSubBits) - 1))]; }
    uint32_t lookup_pair(uint32_t t, uint32_t w) const
    {
        const size_t i = (size_t)t + kPairOffset + (w >> (32 - kHuffFastBits));
        return i < im->pool_words ? im->pool[i] : 0u;  // (behind the last DC table there may be nothing)
    }
    uint32_t tables(int k) const { return (uint32_t)im->k[k].tdc | ((uint32_t)im->k[k].tac << 16); }
    int16_t* block_ptr(int k, uint32_t mx, uint32_t my) const
    {
        const HuffK& hk = im->k[k];
        return im->coef[hk.comp] + ((size_t)hk.blk0 + (size_t)my * hk.stride_y + (size_t)mx * hk.stride_x) * 64;
    }
    int zigzag(int z) const { return kZigzagDeviceGpuHost[z]; }
    int16_t* buf;  // block buffer: 64 coefficients
    void put(int index, int value) const { buf[index] = (int16_t)value; }
    // the select step (select_walk): the tables from the classes as the kernels hold them, in the step's own position count
    StepTables step;
    void step_tables(uint32_t d, uint32_t* tdc, uint32_t* tac) const { select_halves<true>(step, d, tdc, tac); }
    uint32_t step_entry(uint32_t t, uint32_t w) const { return lookup1(t, w); }
    uint32_t step_pair(uint32_t t, uint32_t w) const { return lookup_pair(t, w); }
    uint32_t step_second(uint32_t e) const { return second_table_of(e, 6u, 0u); }
};

// The window of cooperative_subsequence (huffman_gpu_core.h) on the host: what the 64 lanes of the kernel's wave look up at once.
struct HostWindow {
    const HostEnv* env;
    uint32_t edc[64], eac[64];
    uint32_t tables(uint32_t k) const { return env->tables((int)k); }
    uint32_t entry(uint32_t table, uint32_t w) const
    {
        uint32_t e = env->lookup1(table, w);
        if ((e >> 9) == kZadvLong) e = env->lookup2(e, w);
        return e;
    }
    void open(uint32_t pos, uint32_t ts)
    {
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t b = pos + l, bit = b & 31u;
            const uint32_t w0 = env->word(b >> 5), w1 = env->word((b >> 5) + 1);
            const uint32_t w = bit ? (w0 << bit) | (w1 >> (32u - bit)) : w0;
            edc[l] = entry(ts & 0xFFFFu, w);
            eac[l] = entry(ts >> 16, w);
        }
    }
    uint32_t dc(uint32_t rel) const { return edc[rel]; }
    uint32_t ac(uint32_t rel) const { return eac[rel]; }
};

// Block-start records as the kernels keep them (huffman_gpu_core.h): kRecShorts uint16 per subsequence, the mark last.
struct HostRecorder {
    uint16_t* rec;  // the subsequence's record
    uint32_t bit0;  // its first bit
    void operator()(uint32_t i, uint32_t pos) const
    {
        rec[i < (uint32_t)kRecSlots ? i : (uint32_t)kRecSlots] = (uint16_t)(pos - bit0);
    }
};
}  // namespace

namespace {
// The first sync launch as its workgroups schedule it (gpu_huffman.hip), on one image: `units` sync units per workgroup -- 1:
// huff_sync_kernel's pass 0 and Jacobi rounds over kHuffOwn subsequences and the halo; 2: huff_sync_pair_kernel's phases A and B and
// rounds of alternating parity over twice as many -- each workgroup's rounds run to ITS fixpoint, then what the tail and ripple
// launches do to the workgroup seams: every subsequence whose start state is not the state in front of it is decoded again, in
// stream order, which ends in the image's fixpoint in one sweep.  walk(i, begin, z, k, record) decodes subsequence i and keeps the
// record where `record` is set, as the kernels' decodes do: all but those from the assumed state, and none with restart intervals
// (recording == false).  state[i] receives the end states.  counts: decodes per phase up to correction round 2, and the tasks that
// are left then (HIPJPEG_TAIL_AFTER's default: the tail kernel's share).  False if a workgroup's rounds do not end.
template <class Walk>
bool emulate_sync_launch(uint32_t ns, int units, bool recording, Walk& walk, SubseqState* state, SyncScheduleCounts* counts)
{
    const bool paired = units == 2;
    const uint32_t own = (uint32_t)units * kHuffOwn;
    std::vector<uint64_t> from(ns, 0);  // the (masked) state each subsequence was last decoded from
    std::vector<uint64_t> end, start;
    std::vector<int> tasks, next;
    const auto assumed = [](uint32_t j) { return (uint64_t)j * kSubseqBits; };
    for (uint32_t first = 0; first == 0 || first < ns; first += own) {
        if (first >= ns) break;  // (an empty stream)
        const int n_rows = (int)std::min<uint32_t>(own + 1, ns - first + 1);  // local row r = subsequence first - 1 + r; row 0: the halo
        end.assign((size_t)n_rows, 0);
        const auto decode = [&](int row, uint64_t at, bool record) {
            const SubseqState p = unpack_state(at);
            const uint32_t j = first - 1 + (uint32_t)row;
            if (row > 0) from[j] = at & kSyncMask;
            end[(size_t)row] = pack_state(walk(j, p.end_bit, p.zk & 255, p.zk >> 8, record));
        };
        // from the assumed state: every row (the even rows), no records; row 0 of the image's first workgroup is the exact initial state
        for (int r = first ? 0 : (paired ? 2 : 1); r < n_rows; r += paired ? 2 : 1, counts->phase[0]++) decode(r, assumed(first - 1 + (uint32_t)r), false);
        // phase B: the odd rows from their neighbour's end state
        for (int r = 1; paired && r < n_rows; r += 2, counts->phase[1]++) decode(r, end[(size_t)r - 1], recording);
        // round 1: with records every row decoded from the assumed state, else the wrong guesses
        tasks.clear();
        for (int r = paired ? 2 : 1; r < n_rows; r += paired ? 2 : 1)
            if (recording || (end[(size_t)r - 1] & kSyncMask) != assumed(first - 1 + (uint32_t)r)) tasks.push_back(r);
        for (int round = 1; !tasks.empty(); round++) {
            if (round > n_rows + 2) return false;
            if (round <= 2) counts->phase[round + 1] += tasks.size();
            if (round == 3) counts->tail += tasks.size();
            start.clear();
            for (int r : tasks) start.push_back(end[(size_t)r - 1]);  // Jacobi: every start state is read before any end state is replaced
            next.clear();
            for (size_t q = 0; q < tasks.size(); q++) {
                const int r = tasks[q];
                const uint64_t old = end[(size_t)r];
                decode(r, start[q], recording);
                if (((end[(size_t)r] ^ old) & kSyncMask) != 0 && r + 1 < n_rows) next.push_back(r + 1);
            }
            tasks.swap(next);
        }
        for (int r = 1; r < n_rows; r++) state[first - 1 + (uint32_t)r] = unpack_state(end[(size_t)r]);
    }
    // the seams: in stream order every start state is final when its subsequence is looked at
    for (uint32_t j = 1; j < ns; j++) {
        const uint64_t at = pack_state(state[j - 1]);
        if ((at & kSyncMask) == from[j]) continue;
        const SubseqState p = unpack_state(at);
        from[j] = at & kSyncMask;
        state[j] = walk(j, p.end_bit, p.zk & 255, p.zk >> 8, recording);
    }
    return true;
}

// One scan of the frame, as the kernels decode it from its own HuffImage.  Returns 0 or the status the kernels would report.
int emulate_scan(const uint8_t* data, const FrameInfo& f, const ScanHeader& sc, int16_t* const frame_coef[4], int* sync_passes,
                 SyncScheduleCounts* schedules)
{
    // (device scratch: destuff_compact_kernel writes the kept bytes and the 0xFF slack behind them, nothing else)
    std::vector<uint8_t> stream = device_scratch<uint8_t>(destuffed_capacity(sc));
    const size_t n = destuff_scan(data, sc, stream.data());
    std::vector<uint16_t> pool(gpu_pool_words(sc));
    HuffImage im;
    fill_huff_image(f, sc, (uint32_t)n, &im);
    build_gpu_pool(sc, &im, pool.data());
    std::vector<int16_t> dc_diff = device_scratch<int16_t>(im.total_blocks);  // WorkLayout::dc_diff: the block pass writes every block's
    std::vector<uint32_t> boundaries;
    for (uint32_t b : sc.rst_after) boundaries.push_back(b * 8u);
    im.stream = stream.data();
    im.pool = pool.data();
    im.dc_diff = dc_diff.data();
    im.boundaries = boundaries.data();
    im.num_boundaries = (uint32_t)boundaries.size();
    im.restart_interval = (uint32_t)sc.restart_interval;
    const bool rst = sc.restart_interval != 0;
    for (int i = 0; i < sc.ncomp; i++) {
        const int c = sc.comp_index[i];
        int16_t* const coef = frame_coef[c];
        im.coef[i] = coef;
        // every coded block must be written by the write pass; a one-component scan codes the real blocks only (T.81 A.2.2), the
        // padding blocks of its MCU-padded grid are zero as in the host decoder: the zero stands for the fills of
        // DecodeBatch::build_entropy_units() (decoder_core.cpp: huff_zero_, merged by merge_zero_fills(), issued as hipMemsetAsync /
        // hipMemset2DAsync in enqueue_gpu_entropy()) and covers what they cover -- the bottom rows alone when the real blocks fill whole
        // rows, else the whole component
        const size_t bw = (size_t)f.comp[c].blocks_w, bh = (size_t)f.comp[c].blocks_h, rows = sc.ncomp == 1 ? im.mcus_y : bh;
        const size_t cols = sc.ncomp == 1 ? im.mcus_x : bw;
        if (sc.ncomp == 1 && (im.mcus_x < bw || im.mcus_y < bh)) {
            const size_t first = im.mcus_x < bw ? 0 : (size_t)im.mcus_y * bw;
            memset(coef + first * 64, 0, (bw * bh - first) * 128);
        }
        for (size_t y = 0; y < rows; y++) memset(coef + y * bw * 64, 0x5A, cols * 128);
    }
    int16_t block_buffer[64] = {0};
    HostEnv env{&im, block_buffer, StepTables()};
    // The kernels select the tables of an MCU position from registers (TableClasses, in the select step's countdown order, split into
    // halves): the same builder, here, must reproduce env.tables() for every position (else return 5).  (The step's count itself is
    // checked with every walk below: its end state carries the position counted upwards again, recomputed from the countdown, and
    // must equal that of the branch form, which counts upwards.)
    {
        const TableClasses classes = make_countdown_classes(im.blocks_per_mcu, [&](uint32_t q) { return env.tables((int)q); });
        if (!classes.complete) return 5;
        env.step = split_classes(classes, 1u, 0u);
        for (uint32_t q = 0; q < im.blocks_per_mcu; q++) {
            uint32_t tdc, tac;
            env.step_tables(im.blocks_per_mcu - 1u - q, &tdc, &tac);
            if ((tdc | (tac << 16)) != env.tables((int)q)) return 5;
        }
    }
    const HuffGeom geom = make_geom(im);
    const uint32_t ns = im.num_subseq;
    std::vector<SubseqState> cur = device_scratch<SubseqState>(ns), nxt = device_scratch<SubseqState>(ns);  // the states, at 0 of work_
    uint32_t err = 0;
    // Block-start records, as the kernels take them: every decode from a start state that can be final records and writes the mark
    // (in pass 0 only subsequence 0, whose start state is exact: the kernels decode it once more in round 1, from the same state).
    // Not for restart intervals.
    std::vector<uint16_t> records = device_scratch<uint16_t>((size_t)ns * kRecShorts);  // WorkLayout::records
    // Every walk runs in the form huff_sync_kernel uses (select_walk) and again in the form of the tail kernels' lanes
    // (decode_subsequence): same end state and same record, from true and from wrong start states, or `forms_differ` (return 5).
    bool forms_differ = false;
    uint16_t other[kRecShorts];
    uint16_t* walk_records = records.data();  // (emulate_sync_launch's walks write records of their own)
    auto walk = [&](uint32_t i, uint32_t begin, int z, int k, bool record) {
        const uint32_t limit = (i + 1) * kSubseqBits;
        uint16_t* rec = &walk_records[(size_t)i * kRecShorts];
        SubseqState st, sb;
        uint32_t mark = kRecInvalid;
        size_t named = 0;  // bytes of the record the mark vouches for
        if (rst) {
            st = select_walk<true>(geom, env, begin, limit, z, k, 0);
            sb = decode_subsequence<true>(geom, env, begin, limit, z, k, 0);
        } else if (!record) {
            st = select_walk<false>(geom, env, begin, limit, z, k);
            sb = decode_subsequence<false>(geom, env, begin, limit, z, k);
        } else {
            st = select_walk<false>(geom, env, begin, limit, z, k, 0, HostRecorder{rec, i * kSubseqBits});
            sb = decode_subsequence<false>(geom, env, begin, limit, z, k, 0, HostRecorder{other, i * kSubseqBits});
            mark = record_mark(begin, limit < geom.total_bits ? limit : geom.total_bits, (uint32_t)z, st);
            named = mark_valid(mark) ? 2 * (mark & (kRecFresh - 1)) : 0;
        }
        if (pack_state(st) != pack_state(sb) || memcmp(other, rec, named) != 0) forms_differ = true;
        if (record) rec[kRecMark] = (uint16_t)mark;  // (as the kernels: a decode that does not record leaves the mark alone)
        return st;
    };
    // pass 0
    for (uint32_t i = 0; i < ns; i++) cur[i] = walk(i, i * kSubseqBits, 0, 0, i == 0);
    int passes = 0;
    for (;;) {
        bool changed = false;
        if (ns) nxt[0] = cur[0];
        for (uint32_t i = 1; i < ns; i++) {
            const SubseqState& prev = cur[i - 1];
            nxt[i] = walk(i, prev.end_bit, prev.zk & 255, prev.zk >> 8, true);
            if (pack_state(nxt[i]) != pack_state(cur[i])) changed = true;
        }
        cur.swap(nxt);
        passes++;
        if (!changed) break;
        if (passes > (int)ns + 2) return 3;  // cannot happen: the wave of corrections advances one subsequence per pass
    }
    if (sync_passes) *sync_passes = passes;
    if (forms_differ) return 5;
    // The kernels do not run the image-wide Jacobi above but a schedule of their own, workgroup by workgroup, and leave the rest to the
    // tail and ripple launches: emulated here for the paired first launch (and, where the counts are wanted, for one unit per
    // workgroup), followed to the fixpoint.  Same end state, same record for every subsequence, or return 5.
    for (int units = schedules ? 1 : 2; units <= 2; units++) {
        std::vector<SubseqState> got = device_scratch<SubseqState>(ns);
        std::vector<uint16_t> got_records = device_scratch<uint16_t>((size_t)ns * kRecShorts);
        walk_records = got_records.data();
        SyncScheduleCounts counts = {};
        const bool ok = emulate_sync_launch(ns, units, !rst, walk, got.data(), &counts);
        walk_records = records.data();
        if (forms_differ || !ok) return 5;
        for (uint32_t i = 0; i < ns; i++) {
            const uint16_t *a = &records[(size_t)i * kRecShorts], *b = &got_records[(size_t)i * kRecShorts];
            if (pack_state(got[i]) != pack_state(cur[i])) return 5;
            if (rst) continue;  // (no records)
            if (a[kRecMark] != b[kRecMark]) return 5;
            if (mark_valid(a[kRecMark]) && memcmp(a, b, 2 * (a[kRecMark] & (kRecFresh - 1))) != 0) return 5;
        }
        if (schedules) {
            for (int q = 0; q < 4; q++) schedules[units - 1].phase[q] += counts.phase[q];
            schedules[units - 1].tail += counts.tail;
        }
    }
    if (!rst) {
        // The kernels follow the last links of a correction chain with the whole wave on one subsequence (cooperative_subsequence):
        // the same routine, here, must reproduce the lane decoder's end state for every subsequence -- from its true start state and
        // from the state pass 0 assumes (a trajectory through garbage).  Its records must be the lane decoder's (return 5).
        HostWindow win;
        win.env = &env;
        const uint32_t changes = cooperative_table_changes(win, geom.blocks_per_mcu);
        std::vector<uint16_t> coop(kRecShorts), lane(kRecShorts);
        for (uint32_t i = 0; i < ns; i++) {
            const uint32_t begin = i ? cur[i - 1].end_bit : 0u, z = i ? (cur[i - 1].zk & 255u) : 0u, k = i ? (uint32_t)(cur[i - 1].zk >> 8) : 0u;
            const uint32_t limit = (i + 1) * kSubseqBits, end = limit < geom.total_bits ? limit : geom.total_bits;
            const uint16_t* final_rec = &records[(size_t)i * kRecShorts];
            const SubseqState cs = cooperative_subsequence(geom, win, changes, begin, limit, z, k, HostRecorder{coop.data(), i * kSubseqBits});
            if (pack_state(cs) != pack_state(cur[i])) return 4;
            const uint32_t final_mark = final_rec[kRecMark];
            if (record_mark(begin, end, z, cs) != final_mark) return 5;
            if (mark_valid(final_mark) && memcmp(coop.data(), final_rec, 2 * (final_mark & (kRecFresh - 1))) != 0) return 5;
            const SubseqState cg = cooperative_subsequence(geom, win, changes, i * kSubseqBits, limit, 0, 0, HostRecorder{coop.data(), i * kSubseqBits});
            const SubseqState lg = decode_subsequence<false>(geom, env, i * kSubseqBits, limit, 0, 0, 0, HostRecorder{lane.data(), i * kSubseqBits});
            if (pack_state(cg) != pack_state(lg)) return 4;
            const uint32_t mark = record_mark(i * kSubseqBits, end, 0, lg);
            if (mark_valid(mark) && memcmp(coop.data(), lane.data(), 2 * (mark & (kRecFresh - 1))) != 0) return 5;
        }
    }
    // block index of each subsequence's first symbol
    std::vector<uint32_t> first_block = device_scratch<uint32_t>(ns);  // WorkLayout::first_block
    uint32_t acc = 0;
    for (uint32_t i = 0; i < ns; i++) {
        first_block[i] = acc;
        acc += cur[i].nblocks;
    }
    if (acc < im.total_blocks) return 2;
    // write pass, step 1: block start positions.  A usable record must name exactly the blocks the position walk finds, at the
    // same positions (the kernels copy it instead of walking: huff_pos_kernel); else return 5.
    // (not scratch contents but a detector the kernels do not have: a block nobody positioned is reported below instead of decoded
    // from whatever WorkLayout::block_pos held)
    std::vector<uint32_t> block_pos(im.total_blocks, 0xFFFFFFFFu);
    std::vector<uint32_t> found_block, found_pos;
    for (uint32_t i = 0; i < ns; i++) {
        const uint32_t begin = i == 0 ? 0 : cur[i - 1].end_bit;
        const int z = i == 0 ? 0 : (cur[i - 1].zk & 255), k = i == 0 ? 0 : (cur[i - 1].zk >> 8);
        found_block.clear();
        found_pos.clear();
        auto rec = [&](uint32_t block, uint32_t pos) {
            found_block.push_back(block);
            found_pos.push_back(pos);
            if (block < im.total_blocks) block_pos[block] = pos;
        };
        if (rst) {
            uint32_t fault = 0;
            position_subsequence<true>(geom, env, begin, (i + 1) * kSubseqBits, z, k, first_block[i], rec, 0, &fault);
            if (fault) return 1;
        } else
            position_subsequence<false>(geom, env, begin, (i + 1) * kSubseqBits, z, k, first_block[i], rec);
        const uint16_t* r = &records[(size_t)i * kRecShorts];
        const uint32_t mark = r[kRecMark];
        if (rst || !mark_valid(mark)) {
            if (!rst && mark != kRecOverflow) return 5;  // every decode that can be final records
            if (mark == kRecOverflow && found_block.size() <= (size_t)kRecSlots) return 5;
            continue;
        }
        const uint32_t n = mark & (kRecFresh - 1), b0 = first_block[i] + ((mark & kRecFresh) ? 0u : 1u);
        if (n != found_block.size()) return 5;
        for (uint32_t s = 0; s < n; s++)
            if (found_block[s] != b0 + s || found_pos[s] != i * kSubseqBits + r[s]) return 5;
    }
    // restart intervals: the first block of interval j+1 starts exactly at boundary j (see huff_blocks_kernel)
    if (geom.interval_blocks)
        for (uint32_t j = 0; j < im.num_boundaries && (uint64_t)(j + 1) * geom.interval_blocks < im.total_blocks; j++)
            if (block_pos[(j + 1) * geom.interval_blocks] != im.boundaries[j]) return 1;
    // step 2: every block on its own
    for (uint32_t b = 0; b < im.total_blocks; b++) {
        if (block_pos[b] == 0xFFFFFFFFu) return 2;
        int k;
        int16_t* dst = block_address(geom, env, b, &k);
        memset(block_buffer, 0, sizeof block_buffer);
        dc_diff[b] = (int16_t)decode_block(geom, env, block_pos[b], k, &err);
        memcpy(dst, block_buffer, 128);
    }
    if (err) return 1;
    // DC integration, per component in MCU (scan) order
    int pred[4] = {0, 0, 0, 0};
    uint32_t block = 0, mcu = 0;
    for (uint32_t my = 0; my < im.mcus_y; my++)
        for (uint32_t mx = 0; mx < im.mcus_x; mx++, mcu++) {
            if (rst && mcu % im.restart_interval == 0) pred[0] = pred[1] = pred[2] = pred[3] = 0;  // DC predictors start over
            for (uint32_t k = 0; k < im.blocks_per_mcu; k++, block++) {
                const int c = im.k[k].comp;
                pred[c] += dc_diff[block];
                env.block_ptr((int)k, mx, my)[0] = (int16_t)pred[c];
            }
        }
    return 0;
}
}  // namespace

int emulate_gpu_entropy(const uint8_t* data, size_t size, const FrameInfo& f, int16_t* const coef[4], int* sync_passes, SyncScheduleCounts schedules[2])
{
    (void)size;
    // the coefficient blocks of a GPU-decoded picture lie in the device-only part of the arena, which nobody clears: emulate_scan()
    // zeroes what the planner's fills zero (the padding of a one-component scan's grid), the write pass writes every coded block
    for (int c = 0; c < f.ncomp; c++) fill_device_scratch(coef[c], (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 128);
    int passes = 0;
    if (schedules) schedules[0] = schedules[1] = SyncScheduleCounts{};
    for (const ScanHeader& sc : f.scans) {  // the scans are independent: each on its own, as the batched launches take them
        int p = 0;
        const int rc = emulate_scan(data, f, sc, coef, &p, schedules);
        passes = std::max(passes, p);
        if (rc != 0) return rc;
    }
    if (sync_passes) *sync_passes = passes;
    return 0;
}

}  // namespace hipjpeg
