// progressive_encode_host.cpp -- scan descriptors of the GPU coder's progressive output, and its algorithm executed on the host
// with the kernels' per-block routines (progressive_encode_core.h): the encode counterpart of progressive_gpu_host.cpp.
#include <algorithm>
#include <cstring>

#include "huffman_encode_core.h"
#include "progressive_encode.h"
#include "scratch_fill.h"

namespace hipjpeg {

size_t penc_describe(const EncodeGeometry& g, const int16_t* const coef[3], size_t first_block, std::vector<PencScan>* scans, int restart_interval)
{
    const size_t start = first_block;
    for (const ScanSpec& s : simple_progression(g.ncomp)) {
        PencScan sc;
        memset(&sc, 0, sizeof sc);
        for (int c = 0; c < g.ncomp; c++) {
            sc.coef[c] = coef[c];
            sc.blocks_w[c] = (uint32_t)g.blocks_w[c];
            sc.real_w[c] = (uint32_t)g.real_w[c];
            sc.real_h[c] = (uint32_t)g.real_h[c];
        }
        sc.mcus_x = (uint32_t)g.mcus_x;
        sc.ncomp = (uint32_t)g.ncomp;
        sc.hs = g.ncomp == 3 ? (uint32_t)g.hs : 1u;
        sc.vs = g.ncomp == 3 ? (uint32_t)g.vs : 1u;
        sc.bpm = g.ncomp == 3 ? sc.hs * sc.vs + 2 : 1u;
        sc.ss = (uint32_t)s.ss;
        sc.se = (uint32_t)s.se;
        sc.al = (uint32_t)s.al;
        if (s.ss == 0) {
            sc.kind = s.ah == 0 ? kPencDcFirst : kPencDcRefine;
            // an interleaved scan runs over the MCUs, dummy blocks included; one component alone over its real blocks (gray: the same)
            sc.nblocks = g.ncomp == 3 ? (uint32_t)(g.mcus_x * g.mcus_y) * sc.bpm : (uint32_t)(g.real_w[0] * g.real_h[0]);
        } else {
            const int c = s.comp[0];
            sc.kind = s.ah == 0 ? kPencAcFirst : kPencAcRefine;
            sc.acoef = coef[c];
            sc.abw = (uint32_t)g.blocks_w[c];
            sc.arw = (uint32_t)g.real_w[c];
            sc.table = c == 0 ? 0u : 1u;
            sc.nblocks = (uint32_t)(g.real_w[c] * g.real_h[c]);
        }
        // an MCU is bpm blocks in an interleaved DC scan, one block in every other scan (jcmaster.c per_scan_setup)
        sc.rst_blocks = (uint32_t)restart_interval * (s.ss == 0 && g.ncomp == 3 ? sc.bpm : 1u);
        sc.first_block = (uint32_t)first_block;
        first_block += ((size_t)sc.nblocks + 63) & ~(size_t)63;
        scans->push_back(sc);
    }
    return first_block - start;
}

namespace {

struct HostCount {
    uint32_t* h;
    void sym(int s) const { h[s]++; }
    void bits(uint32_t, int) const {}
};

struct HostWords {  // big-endian words over a byte buffer
    uint8_t* p;
    void or_word(uint32_t i, uint32_t w) const
    {
        for (int k = 0; k < 4; k++) p[4 * (size_t)i + k] |= (uint8_t)(w >> (24 - 8 * k));
    }
};

constexpr uint32_t kLanes = 256;  // lanes of the scan kernel's workgroup: each takes a contiguous range of the scan's blocks

// One scan with the flavour the plan would launch; `dri`: the interval for the DRI segment in front of the file's first SOS, else 0.
template <bool RST>
void encode_scan(PencScan sc, const ScanSpec& spec, int dri, std::vector<uint8_t>* out)
{
    sc.first_block = 0;
    const uint32_t n = sc.nblocks;
    // hist: the zero stands for EncodeBatch::penc_statistics()'s hipMemsetAsync of PencLayout1::hist (encoder_core.cpp); codes is the
    // host's own table, uploaded whole
    uint32_t hist[256], codes[256];
    memset(hist, 0, sizeof hist);
    memset(codes, 0, sizeof codes);
    // pre, post: the zeros stand for the hipMemsetAsync of PencLayout1::pre / post in the same place (the run kernel stores only where a
    // run is flushed, every later kernel reads every block's).  Everything else is device scratch: sum, own, bits and off are written
    // for every block; piece, flusher and rel only where a block has them, and are read only there.
    std::vector<uint8_t> sum = device_scratch<uint8_t>(n);
    std::vector<uint32_t> pre(n), post(n);
    std::vector<uint32_t> piece = device_scratch<uint32_t>(n), flusher = device_scratch<uint32_t>(n), off = device_scratch<uint32_t>(n);
    std::vector<uint16_t> rel = device_scratch<uint16_t>(n), own = device_scratch<uint16_t>(n), bits = device_scratch<uint16_t>(n);
    // summary: lane per block
    const HostCount cnt{hist};
    for (uint32_t i = 0; i < n; i++) sum[i] = (uint8_t)penc_block_summary<RST>(sc, i, cnt);
    // runs: the wave's steps in order
    if (sc.kind >= kPencAcFirst) {
        PencRun r{0, 0, 0};
        PencIntervalEnds<RST> ends(sc.rst_blocks, n);
        for (uint32_t i = 0; i < n; i++) {
            const PencStep st = penc_run_step<RST>(r, i, sum[i], ends.at(i));
            if (st.pre) {
                pre[i] = st.pre;
                flusher[st.pre_ps] = i;
                hist[penc_eob_nbits(st.pre & 0xFFFF) << 4]++;
            }
            if (st.post) {
                post[i] = st.post;
                flusher[st.post_ps] = i;
                hist[penc_eob_nbits(st.post & 0xFFFF) << 4]++;
            }
            if ((sum[i] & 2) && (sum[i] >> 2)) {
                piece[i] = st.ps;
                rel[i] = (uint16_t)st.rel;
            }
        }
        if (const uint32_t e = penc_run_end(r)) {
            post[n - 1] = e;
            flusher[r.ps] = n - 1;
            hist[penc_eob_nbits(e & 0xFFFF) << 4]++;
        }
    }
    // tables, DHT, [DRI] and SOS on the host
    progressive_scan_header(spec, hist, codes, out, dri);
    // lengths
    for (uint32_t i = 0; i < n; i++) {
        uint32_t o;
        bits[i] = (uint16_t)penc_block_length<RST>(sc, i, codes, pre[i], post[i], &o);
        own[i] = (uint16_t)o;
    }
    // offsets: the prefix sum; with restart intervals the segmented scan as henc_scan_rst_kernel runs it -- every lane's range, the
    // workgroup's doubling steps over the lanes' spans, every lane's range again
    uint32_t total = 0;
    if (!RST) {
        for (uint32_t i = 0; i < n; i++) {
            off[i] = total;
            total += bits[i];
        }
    } else {
        const uint32_t per = (n + kLanes - 1) / kLanes;
        HencSpan span[kLanes];
        for (uint32_t t = 0; t < kLanes; t++) {
            const uint32_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
            HencSpan sp{0u, 0u, 0u};
            for (uint32_t i = lo; i < hi; i++) sp = henc_span_join(sp, henc_span_block(bits[i], penc_ends_interval<RST>(sc.rst_blocks, n, i)));
            span[t] = sp;
        }
        for (uint32_t d = 1; d < kLanes; d <<= 1) {
            HencSpan next[kLanes];
            for (uint32_t t = 0; t < kLanes; t++) next[t] = t >= d ? henc_span_join(span[t - d], span[t]) : span[t];
            memcpy(span, next, sizeof span);
        }
        for (uint32_t t = 0; t < kLanes; t++) {
            const uint32_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
            uint32_t run = t ? henc_span_apply(0u, span[t - 1]) : 0u;
            for (uint32_t i = lo; i < hi; i++) {
                off[i] = run;
                run = henc_span_apply(run, henc_span_block(bits[i], penc_ends_interval<RST>(sc.rst_blocks, n, i)));
            }
        }
        total = henc_span_apply(0u, span[kLanes - 1]);
    }
    // write: lane per block into the zeroed bit buffer, the marker bitmap behind it (the zero stands for henc_zero_kernel,
    // gpu_huffman_encode.hip, which EncodeBatch::henc_assemble() launches over all of HencLayout2::raw: bit buffers and bitmaps)
    const uint32_t raw_bytes = (total + 7) / 8;
    std::vector<uint8_t> raw((size_t)henc_map_offset(raw_bytes) + henc_map_bytes(raw_bytes), 0);
    uint8_t* map = raw.data() + henc_map_offset(raw_bytes);
    const PencBlockArrays a{sum.data(), pre.data(), post.data(), piece.data(), flusher.data(), rel.data(), own.data(), bits.data(), off.data()};
    const HostWords words{raw.data()};
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t marker = penc_block_write<RST>(sc, i, codes, words, a);
        if (RST && marker != ~0u) map[marker >> 3] |= (uint8_t)(1u << (marker & 7));  // bit `marker` of the little-endian dwords
    }
    // count / expand: a 0x00 behind every 0xFF that is data
    const uint16_t* pieces = reinterpret_cast<const uint16_t*>(map);  // halfword p: the 16-byte piece p
    for (uint32_t b = 0; b < raw_bytes; b++) {
        out->push_back(raw[b]);
        if (raw[b] == 0xFF && !(RST && henc_is_marker(pieces, b))) out->push_back(0);
    }
}

}  // namespace

void encode_progressive_gpu_algorithm(const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], const int16_t* const coef[3],
                                      int restart_interval, std::vector<uint8_t>* out)
{
    std::vector<PencScan> scans;
    penc_describe(g, coef, 0, &scans, restart_interval);
    const std::vector<ScanSpec> script = simple_progression(g.ncomp);
    write_progressive_frame_header(g, qlum, qchr, out);
    for (size_t k = 0; k < scans.size(); k++) {
        const int dri = k == 0 ? restart_interval : 0;
        // the flavour the plan would launch
        if (restart_interval)
            encode_scan<true>(scans[k], script[k], dri, out);
        else
            encode_scan<false>(scans[k], script[k], dri, out);
    }
    out->push_back(0xFF);
    out->push_back(0xD9);
}

}  // namespace hipjpeg
