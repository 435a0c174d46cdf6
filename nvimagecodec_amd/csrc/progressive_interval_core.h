// progressive_interval_core.h -- progressive (SOF2) scans WITH restart intervals on the GPU entropy stage: the parse logic shared by
// the kernels (progressive_intervals.hip) and their host emulation (progressive_gpu_host.cpp, used by the CPU tests).
//
// progressive_gpu_core.h explains why a refinement scan is a sequential chain.  A restart interval breaks the chain: every interval
// starts byte-aligned at a position the parser knows (ScanHeader::rst_after), with an end-of-band run of 0 and DC predictors of 0.
// So the block start positions the replay needs -- all the walk produces -- can be found by one LANE per restart interval instead of
// one wave per scan, and so can the DC planes:
//   AC item  (component, interval i): blocks [i N, min((i + 1) N, nbx nby)) of the component, N = the restart interval its AC scans
//            share.  For each scan of the component's chain, in file order, the lane parses its interval of that scan and records
//            block_pos exactly as prog_walk_scan defines it.  A refinement scan needs the block's non-zero bitmap from the scans before
//            (prog_replay_block's `nonzero`), no coefficient values: one uint64 per block in device scratch, written at stage s and read
//            back at stage s + 1 by the same lane.  The item never writes a coefficient.
//   DC item  (DC scan, interval i): first scans decode differences from predictors 0 and store pred << al into the compact DC planes,
//            refinement scans OR 1 << al into them (bit = interval start + index of the block within the interval).  A later DC scan may
//            cut the same blocks into other intervals, so the DC scans of an image run in order: one launch per DC-scan index.
// prog_replay_block then builds the coefficients from the recorded positions, unchanged.
// Vouching: an item returns false (the image's status becomes 1, the host decoder takes it and names the error) on whatever
// prog_walk_scan / prog_replay_block reject, when an interval's parse does not end in (end - 8, end] bits (end = the next interval's
// start, the scan's total_bits for the last one), and when an end-of-band run is still open at the interval's end.
#pragma once
#include <cstdint>

#include "progressive_gpu_core.h"

namespace hipjpeg {

constexpr int kProgIntervalLanes = 256;  // intervals per workgroup

// Beside a ProgImage: where the intervals of its scans start.  The kernels index these with wave-uniform run-time indices, so they hold
// 32- and 64-bit members only (the hazard note at ProgScan); the static_asserts below and
// tests/test_progressive_intervals.py::test_interval_descriptors_have_no_sub_dword_members keep it that way.
struct ProgIntervalScan {
    uint32_t first_start;  // index into the batch-wide array of interval starts (bits): entry k - 1 = start of interval k >= 1
    uint32_t interval;     // restart interval: MCUs of an interleaved scan, blocks of a single-component one
    uint32_t count;        // intervals of the scan (markers + 1)
    uint32_t pad;
};
struct alignas(16) ProgIntervalImage {
    ProgIntervalScan scan[kProgMaxScans];
    unsigned long long* hist[4];  // per component with more than one AC scan: non-zero bitmap of every real block (device scratch)
    uint32_t ac_interval[4];      // the restart interval the component's AC scans share, their interval count
    uint32_t ac_count[4];
};
static_assert(sizeof(ProgIntervalScan) == 4 * sizeof(uint32_t), "ProgIntervalScan: four 32-bit words, nothing smaller, no padding");
static_assert(sizeof(ProgIntervalImage) == kProgMaxScans * sizeof(ProgIntervalScan) + 4 * sizeof(unsigned long long*) + 8 * sizeof(uint32_t),
              "ProgIntervalImage: 32- and 64-bit members only, no padding");

// MSB-first reader that knows where it is.  `E` as for ProgBits: word(sc, i).
struct ProgIntervalBits {
    ProgBits br;
    uint32_t pos;
    template <class E>
    HJ_HD void start(const E& e, const ProgScan& sc, uint32_t at)
    {
        br.start(e, sc, at);
        pos = at;
    }
    template <class E>
    HJ_HD void take(const E& e, const ProgScan& sc, uint32_t n)  // any n < 128
    {
        pos += n;
        while (n > 31u) {
            br.consume(e, sc, 31u);
            n -= 31u;
        }
        br.consume(e, sc, n);
    }
};

// One interval of one component through all AC scans of the component.  `E` supplies per-lane accessors:
//   uint32_t word(const ProgScan&, uint32_t i)            32-bit word i of the scan's stream, MSB first (ones behind the end)
//   uint32_t lookup(const ProgScan&, uint32_t w)          lookup-table entry of an AC scan for the window w (next 32 bits)
//   uint32_t bound(uint32_t scan, uint32_t k)             start of interval k of scan[scan] in bits; k = count: the scan's total_bits
//   uint64_t hist(uint32_t b) / void set_hist(uint32_t b, uint64_t)   non-zero bitmap of block b of the component
//   void set_pos(const ProgScan&, uint32_t b, uint32_t)   block_pos of block b
template <class E>
HJ_HD bool prog_interval_ac(E& env, const ProgImage& im, const ProgIntervalImage& iv, int comp, uint32_t i)
{
    const uint32_t nb = im.nbx[comp] * im.nby[comp], n = iv.ac_interval[comp];
    const uint32_t b0 = i * n, b1 = nb - b0 < n ? nb : b0 + n;
    const int stages = (int)im.chain_len[comp];
    for (int st = 0; st < stages; st++) {
        const uint32_t sidx = im.chain[comp][st];
        const ProgScan& sc = im.scan[sidx];
        const int ss = (int)sc.ss, se = (int)sc.se;
        const bool refine = sc.ah != 0, track = st + 1 < stages;
        const uint64_t band = prog_band_mask(ss, se);
        const uint32_t end = env.bound(sidx, i + 1);
        ProgIntervalBits r;
        r.start(env, sc, env.bound(sidx, i));
        uint32_t eobrun = 0;
        for (uint32_t b = b0; b < b1; b++) {
            uint64_t h = st > 0 ? env.hist(b) : 0ull;
            if (eobrun != 0) {
                // inside an end-of-band run: a first scan has nothing for this block, a refinement scan one correction bit per
                // coefficient of the band that is already non-zero
                env.set_pos(sc, b, r.pos | kProgInRun);
                if (refine) r.take(env, sc, (uint32_t)prog_popc64(h & band));
                eobrun--;
            } else {
                env.set_pos(sc, b, r.pos);
                int k = ss;
                while (k <= se) {
                    const uint32_t e = env.lookup(sc, r.br.hi);
                    const uint32_t len = e & 31u, run = (e >> 9) & 15u, s = (e >> 5) & 15u;
                    if (len == 0 || (refine && s > 1)) return false;  // no such code / a refinement size other than 1
                    r.take(env, sc, len);
                    if (s == 0 && run != 15) {
                        // end of band: this block is the run's first; refinement: + a correction bit for every non-zero-history
                        // coefficient in the rest of the band
                        eobrun = (1u << run) - 1u + r.br.peek(run);
                        r.take(env, sc, run + (refine ? (uint32_t)prog_popc64(h & band & prog_from_mask(k)) : 0u));
                        break;
                    }
                    if (!refine) {
                        if (s == 0) {
                            k += 16;
                            continue;
                        }
                        k += (int)run;
                        if (k > se) return false;  // a run past the band
                        r.take(env, sc, s);
                        h |= 1ull << k;
                        k++;
                    } else {
                        if (s == 1) r.take(env, sc, 1);  // the new coefficient's sign
                        // the (run + 1)-th zero-history coefficient at or behind k
                        uint64_t z = ~h & band & prog_from_mask(k);
                        int t = se + 1;
                        for (uint32_t j = 0; j <= run && z; j++) {
#if defined(__HIP_DEVICE_COMPILE__)
                            const int p = __ffsll((unsigned long long)z) - 1;
#else
                            const int p = __builtin_ctzll(z);
#endif
                            z &= z - 1;
                            if (j == run) t = p;
                        }
                        if (t > se && s == 1) return false;  // fewer zero-history coefficients left than the run says
                        // one correction bit for every non-zero-history coefficient passed on the way
                        r.take(env, sc, (uint32_t)prog_popc64(h & band & prog_from_mask(k) & ~prog_from_mask(t > se ? se + 1 : t)));
                        if (s == 1) h |= 1ull << t;
                        k = t + 1;
                    }
                }
            }
            if (track) env.set_hist(b, h);
            if (r.pos > end) return false;  // the parse has left the interval
        }
        if (eobrun != 0 || end - r.pos >= 8u) return false;
    }
    return true;
}

// One interval of one DC scan.  `E` supplies, beside word() and bound():
//   uint32_t dc_lookup(const ProgScan&, uint32_t slot, uint32_t w)   lookup-table entry of the scan's slot-th component
//   void dc_store(uint32_t comp, uint32_t index, int v) / void dc_or(uint32_t comp, uint32_t index, int bits)
//                                                                    DC value of the block at `index` of the component's allocation grid
// An interleaved scan walks MCUs of the padded grid, a single-component scan its real blocks.
template <class E>
HJ_HD bool prog_interval_dc(E& env, const ProgImage& im, const ProgIntervalImage& iv, uint32_t sidx, uint32_t i)
{
    const ProgScan& sc = im.scan[sidx];
    const bool single = sc.ncomp == 1;
    const uint32_t c0 = sc.comps[0];
    const uint32_t across = single ? im.nbx[c0] : im.mcus_x;
    const uint32_t mcus = across * (single ? im.nby[c0] : im.mcus_y);
    const uint32_t n = iv.scan[sidx].interval;
    const uint32_t m0 = i * n, m1 = mcus - m0 < n ? mcus : m0 + n;
    const uint32_t start = env.bound(sidx, i), end = env.bound(sidx, i + 1);
    const bool refine = sc.ah != 0;
    const int al = (int)sc.al;
    ProgIntervalBits r;
    r.start(env, sc, start);
    int pred[4] = {0, 0, 0, 0};
    uint32_t my = m0 / across, mx = m0 - my * across;
    for (uint32_t m = m0; m < m1; m++) {
        for (uint32_t k = 0; k < sc.ncomp; k++) {
            const uint32_t c = sc.comps[k];
            const uint32_t h = single ? 1u : im.comp_h[c], v = single ? 1u : im.comp_v[c];
            for (uint32_t dy = 0; dy < v; dy++)
                for (uint32_t dx = 0; dx < h; dx++) {
                    const uint32_t index = (my * v + dy) * im.blocks_w[c] + mx * h + dx;
                    if (refine) {
                        if (r.br.peek(1)) env.dc_or(c, index, 1 << al);
                        r.take(env, sc, 1);
                    } else {
                        const uint32_t e = env.dc_lookup(sc, k, r.br.hi);
                        const uint32_t len = e & 31u, sz = (e >> 5) & 255u;
                        if (len == 0 || sz > 15) return false;
                        r.take(env, sc, len);
                        const uint32_t bits = r.br.peek(sz);
                        r.take(env, sc, sz);
                        pred[k] += sz == 0 ? 0 : bits < (1u << (sz - 1)) ? (int)bits - (int)(1u << sz) + 1 : (int)bits;
                        env.dc_store(c, index, pred[k] * (1 << al));
                    }
                }
        }
        if (r.pos > end) return false;
        if (++mx == across) {
            mx = 0;
            my++;
        }
    }
    return end - r.pos < 8u;
}

}  // namespace hipjpeg
