// progressive_encode_host.cpp -- scan descriptors of the GPU coder's progressive output, and its algorithm executed on the host
// with the kernels' per-block routines (progressive_encode_core.h): the encode counterpart of progressive_gpu_host.cpp.
#include <cstring>

#include "progressive_encode.h"

namespace hipjpeg {

size_t penc_describe(const EncodeGeometry& g, const int16_t* const coef[3], size_t first_block, std::vector<PencScan>* scans)
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

}  // namespace

void encode_progressive_gpu_algorithm(const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], const int16_t* const coef[3],
                                      std::vector<uint8_t>* out)
{
    std::vector<PencScan> scans;
    penc_describe(g, coef, 0, &scans);
    const std::vector<ScanSpec> script = simple_progression(g.ncomp);
    write_progressive_frame_header(g, qlum, qchr, out);
    for (size_t k = 0; k < scans.size(); k++) {
        PencScan sc = scans[k];
        sc.first_block = 0;
        const uint32_t n = sc.nblocks;
        uint32_t hist[256], codes[256];
        memset(hist, 0, sizeof hist);
        memset(codes, 0, sizeof codes);
        std::vector<uint8_t> sum(n);
        std::vector<uint32_t> pre(n), post(n), piece(n), flusher(n), off(n);
        std::vector<uint16_t> rel(n), own(n), bits(n);
        // summary: lane per block
        const HostCount cnt{hist};
        for (uint32_t i = 0; i < n; i++) sum[i] = (uint8_t)penc_block_summary(sc, i, cnt);
        // runs: the wave's steps in order
        if (sc.kind >= kPencAcFirst) {
            PencRun r{0, 0, 0};
            for (uint32_t i = 0; i < n; i++) {
                const PencStep st = penc_run_step(r, i, sum[i]);
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
        // tables, DHT and SOS on the host
        progressive_scan_header(script[k], hist, codes, out);
        // lengths and their prefix sum
        uint32_t total = 0;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t o;
            bits[i] = (uint16_t)penc_block_length(sc, i, codes, pre[i], post[i], &o);
            own[i] = (uint16_t)o;
            off[i] = total;
            total += bits[i];
        }
        // write: lane per block into the zeroed bit buffer
        const uint32_t raw_bytes = (total + 7) / 8;
        std::vector<uint8_t> raw(((size_t)raw_bytes + 3) / 4 * 4 + 16, 0);
        const PencBlockArrays a{sum.data(), pre.data(), post.data(), piece.data(), flusher.data(), rel.data(), own.data(), bits.data(), off.data()};
        const HostWords words{raw.data()};
        for (uint32_t i = 0; i < n; i++) penc_block_write(sc, i, codes, words, a);
        // byte stuffing
        for (uint32_t b = 0; b < raw_bytes; b++) {
            out->push_back(raw[b]);
            if (raw[b] == 0xFF) out->push_back(0);
        }
    }
    out->push_back(0xFF);
    out->push_back(0xD9);
}

}  // namespace hipjpeg
