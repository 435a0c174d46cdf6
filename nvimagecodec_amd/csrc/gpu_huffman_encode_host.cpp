// gpu_huffman_encode_host.cpp -- the GPU coder's baseline algorithm executed on the host with the kernels' own routines
// (huffman_encode_core.h): statistics, lengths, the (segmented) scan, bit emission with padding and restart markers, byte
// stuffing.  The encode counterpart of gpu_huffman_host.cpp; progressive output has progressive_encode_host.cpp.
#include <algorithm>
#include <cstring>

#include "huffman_encode_core.h"
#include "scratch_fill.h"

namespace hipjpeg {

namespace {

constexpr uint32_t kLanes = 256;  // lanes of the scan kernel's workgroup: each takes a contiguous range of the image's blocks

struct HostCount {
    uint32_t (*hist)[256];  // [0] DC categories, [1] AC run/size symbols
    void add(int dcac, int sym) const { hist[dcac][sym]++; }
};

struct HostWords {  // big-endian words over a byte buffer
    uint8_t* p;
    void or_word(uint32_t i, uint32_t w) const
    {
        for (int k = 0; k < 4; k++) p[4 * (size_t)i + k] |= (uint8_t)(w >> (24 - 8 * k));
    }
};

// What the kernels' fetch_block hands to the per-block routines
struct Fetched {
    uint32_t w[32];
    bool real;
    int diff, ti;
};

template <bool RST>
Fetched fetch_block(const HencImage& im, uint32_t s)
{
    Fetched f;
    const HencBlockRef r = henc_locate<RST>(im, s);
    f.ti = r.c == 0 ? 0 : 1;
    f.real = r.bx < im.real_w[r.c] && r.by < im.real_h[r.c];
    int dc;
    if (f.real) {
        memcpy(f.w, im.coef[r.c] + ((size_t)r.by * im.blocks_w[r.c] + r.bx) * 64, sizeof f.w);
        dc = (int)(short)(f.w[0] & 0xFFFF);
    } else {
        memset(f.w, 0, sizeof f.w);
        dc = henc_dc_value(im, r.c, r.bx, r.by);
    }
    f.diff = dc - (r.has_prev ? henc_dc_value(im, r.c, r.pbx, r.pby) : 0);
    return f;
}

template <bool RST>
void encode(HencImage im, const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], int restart_interval, bool optimized,
            std::vector<uint8_t>* out)
{
    const uint32_t n = im.total_blocks;
    // tables and SOI .. SOS: Annex K, or from the histogram step's counts
    StandardCodeTables T;
    if (optimized) {
        uint32_t counts[2][2][256];
        memset(counts, 0, sizeof counts);  // (stands for EncodeBatch::henc_histograms()'s hipMemsetAsync of HencLayout1::hist, encoder_core.cpp)
        for (uint32_t s = 0; s < n; s++) {
            const Fetched f = fetch_block<RST>(im, s);
            henc_count_block(f.w, f.real, f.diff, HostCount{counts[f.ti]});
        }
        optimal_code_tables(counts, g, qlum, qchr, &T, out, restart_interval);
    } else {
        standard_code_tables(&T);
        write_standard_headers(g, qlum, qchr, out, restart_interval);
    }
    // length: lane per block
    std::vector<uint16_t> bits = device_scratch<uint16_t>(n);  // HencLayout1::bits: henc_length_kernel stores every block's
    for (uint32_t s = 0; s < n; s++) {
        const Fetched f = fetch_block<RST>(im, s);
        bits[s] = (uint16_t)henc_code_block<false>(f.w, f.real, f.diff, &T, f.ti, (HencEmitter<HostWords>*)nullptr);
    }
    // scan: every lane's range, the workgroup's doubling steps over the lanes' spans, every lane's range again
    std::vector<uint32_t> off = device_scratch<uint32_t>(n);  // HencLayout1::off: the scan kernels store every block's
    const uint32_t per = (n + kLanes - 1) / kLanes;
    HencSpan sum[kLanes];
    for (uint32_t t = 0; t < kLanes; t++) {
        const uint32_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
        HencSpan sp{0u, 0u, 0u};
        for (uint32_t i = lo; i < hi; i++) sp = henc_span_join(sp, henc_span_block(bits[i], henc_ends_interval<RST>(im, i)));
        sum[t] = sp;
    }
    for (uint32_t d = 1; d < kLanes; d <<= 1) {
        HencSpan next[kLanes];
        for (uint32_t t = 0; t < kLanes; t++) next[t] = t >= d ? henc_span_join(sum[t - d], sum[t]) : sum[t];
        memcpy(sum, next, sizeof sum);
    }
    for (uint32_t t = 0; t < kLanes; t++) {
        const uint32_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
        uint32_t run = t ? henc_span_apply(0u, sum[t - 1]) : 0u;
        for (uint32_t i = lo; i < hi; i++) {
            off[i] = run;
            run = henc_span_apply(run, henc_span_block(bits[i], henc_ends_interval<RST>(im, i)));
        }
    }
    const uint32_t total = henc_span_apply(0u, sum[kLanes - 1]);
    // write: lane per block into the zeroed bit buffer, the marker bitmap behind it (the zero stands for henc_zero_kernel,
    // gpu_huffman_encode.hip, which EncodeBatch::henc_assemble() launches over all of HencLayout2::raw: bit buffers and bitmaps)
    im.raw_bytes = (total + 7) / 8;
    std::vector<uint8_t> raw((size_t)henc_map_offset(im.raw_bytes) + henc_map_bytes(im.raw_bytes), 0);
    im.raw = raw.data();
    uint8_t* map = raw.data() + henc_map_offset(im.raw_bytes);
    for (uint32_t s = 0; s < n; s++) {
        const Fetched f = fetch_block<RST>(im, s);
        HencEmitter<HostWords> em;
        em.start(HostWords{raw.data()}, off[s]);
        henc_code_block<true>(f.w, f.real, f.diff, &T, f.ti, &em);
        const uint32_t marker = henc_finish_block<RST>(im, s, off[s], &em);
        if (marker != ~0u) map[marker >> 3] |= (uint8_t)(1u << (marker & 7));  // bit `marker` of the little-endian dwords
        em.finish();
    }
    // count / expand: a 0x00 behind every 0xFF that is data
    const uint16_t* pieces = reinterpret_cast<const uint16_t*>(map);  // halfword p: the 16-byte piece p (16-byte aligned in the vector's block)
    for (uint32_t b = 0; b < im.raw_bytes; b++) {
        out->push_back(raw[b]);
        if (raw[b] == 0xFF && !(RST && henc_is_marker(pieces, b))) out->push_back(0);
    }
    out->push_back(0xFF);
    out->push_back(0xD9);
}

}  // namespace

void encode_baseline_gpu_algorithm(const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], const int16_t* const coef[3],
                                   int restart_interval, bool optimized, std::vector<uint8_t>* out)
{
    HencImage im;
    memset(&im, 0, sizeof im);
    for (int c = 0; c < g.ncomp; c++) {
        im.coef[c] = coef[c];
        im.blocks_w[c] = (uint32_t)g.blocks_w[c];
        im.real_w[c] = (uint32_t)g.real_w[c];
        im.real_h[c] = (uint32_t)g.real_h[c];
    }
    im.mcus_x = (uint32_t)g.mcus_x;
    im.mcus_y = (uint32_t)g.mcus_y;
    im.ncomp = (uint32_t)g.ncomp;
    im.hs = (uint32_t)g.hs;
    im.vs = (uint32_t)g.vs;
    im.bpm = g.ncomp == 3 ? (uint32_t)(g.hs * g.vs + 2) : 1u;
    im.total_blocks = im.mcus_x * im.mcus_y * im.bpm;
    im.rst_blocks = (uint32_t)restart_interval * im.bpm;
    im.nseg = im.last_seg = 1;
    // the flavour the plan would launch
    if (im.rst_blocks)
        encode<true>(im, g, qlum, qchr, restart_interval, optimized, out);
    else
        encode<false>(im, g, qlum, qchr, restart_interval, optimized, out);
}

}  // namespace hipjpeg
