// progressive_encode_core.h -- the per-block routines of the GPU coder's progressive (SOF2) output.  Compiles for host and device:
// the kernels (progressive_encode.hip) and the host emulation (progressive_encode_host.cpp) run this very code.
//
// The specification is the host coder's ProgressiveScanCoder (entropy_encode.cpp, jcphuff.c), whose only sequential state in a
// scan without restart intervals is the end-of-band run: EOBRUN (n) and the correction bits buffered behind it (be).  Every block
// is summarised by three facts that do not depend on that state (penc_ac_first / penc_ac_refine):
//   content   the block codes a symbol of its own (a coefficient that becomes non-zero in this scan); before that symbol the
//             pending run is flushed
//   tail      the block ends in zeros or buffered correction bits: it extends the run by one
//   b         refinement scans: the correction bits behind its last new coefficient, buffered with the run
// penc_run_step resolves the run recurrence over these summaries (content flushes; n == 0x7FFF or be > 937 after a tail cuts);
// then every block knows the flush in front of its symbols (pre), the flush behind them (post), and, for a run block with b > 0,
// the run piece it belongs to (the piece's flushing block and the bits of earlier blocks of the piece: rel).  Every bit of the scan
// then has a position that one lane per block can compute, and the block's lane writes what it owns:
//   [pre: EOBn code, n bits, the piece's buffered bits] own symbols [post: EOBn code, n bits, the piece's buffered bits]
// A flush's buffered bits are written by the blocks that buffered them, each at flush position + EOBn length + rel.
//
// Restart intervals (jcphuff.c emit_restart; PencScan::rst_blocks, template <bool RST>) add three things and keep that shape:
//   predictor  DC first scans: the first block of each component in the MCU that opens an interval has no previous block
//   run        the last block of an interval that another one follows flushes what is pending behind its own tail step: a post
//              flush like a cut's, so that a run piece never spans an interval
//   marker     that block's lane also pads the byte behind everything it lays down and writes FF Dn there (huffman_encode_core.h has
//              the segmented offsets, the marker bitmap and the stuffing that spares the markers; they work per segment and are shared)
// RST = false compiles all of it away: scans without an interval run the code they always ran.
#pragma once
#include <cstdint>

#include "huffman_gpu_core.h"  // HJ_HD

namespace hipjpeg {

constexpr uint32_t kPencMaxRun = 0x7FFF;             // jcphuff.c: EOBRUN is flushed when it reaches 0x7FFF
constexpr uint32_t kPencMaxCorr = 1000 - 64 + 1;     // jcphuff.c: ... or when more than MAX_CORR_BITS - DCTSIZE2 + 1 bits are buffered
enum PencKind : uint32_t { kPencDcFirst = 0, kPencDcRefine = 1, kPencAcFirst = 2, kPencAcRefine = 3 };

// One scan of one image.  32- and 64-bit members only; the component a lane reads is chosen per lane (DC scans) or fixed by the
// descriptor (AC scans: acoef / abw / arw), never by indexing the descriptor with a uniform value.
struct alignas(16) PencScan {
    const int16_t* coef[3];  // the image's zigzag-ordered grids (encode_layout.h)
    const int16_t* acoef;    // AC scans: the grid of the scan's component
    uint32_t* hist;          // [256] symbol counts (DC first: [t * 16 + category]; AC: [run/size]); null for DC refinement
    const uint32_t* codes;   // [256] code | length << 16, same indexing
    uint32_t blocks_w[3], real_w[3], real_h[3];
    uint32_t mcus_x, ncomp, hs, bpm;
    uint32_t abw, arw;       // AC scans: grid width and real width (blocks per row) of the component
    uint32_t ss, se, al, kind;
    uint32_t table;          // AC scans: 0 luma, 1 chroma
    uint32_t nblocks;        // blocks in scan order: MCU order with the padding's dummy blocks (DC), real blocks in raster order (AC)
    uint32_t first_block;    // into the batch-wide per-block arrays
    uint32_t vs;
    uint32_t rst_blocks;     // the restart interval in blocks of this scan: restart_interval * bpm (interleaved DC scans), restart_interval
                             // (one block per MCU: AC scans, one-component frames); 0: none
};

// Block i opens an interval (i: the first block of its MCU in DC scans).
template <bool RST>
HJ_HD bool penc_starts_interval(const PencScan& sc, uint32_t i)
{
    return RST && sc.rst_blocks != 0 && i % sc.rst_blocks == 0;
}

// Block i is the last of an interval that another one follows (the scan's last block never is).
template <bool RST>
HJ_HD bool penc_ends_interval(uint32_t rst_blocks, uint32_t nblocks, uint32_t i)
{
    return RST && rst_blocks != 0 && i + 1 < nblocks && (i + 1) % rst_blocks == 0;
}

HJ_HD int penc_bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

HJ_HD int penc_coef(const uint32_t (&w)[32], int k) { return (k & 1) ? ((int)w[k >> 1] >> 16) : ((int)(w[k >> 1] << 16) >> 16); }

// ---- DC scans: where block s of the MCU order lives (gpu_huffman_encode.hip locate / dc_value, entropy_encode.cpp BlockSource)
struct PencDcRef {
    int c;
    int dc, prev;  // the block's DC and the DC of the same component's previous block in scan order (0 for the first)
};

HJ_HD int penc_dc_value(const PencScan& sc, int c, uint32_t bx, uint32_t by)
{
    const uint32_t mh = (c == 0 && sc.ncomp == 3) ? sc.hs : 1;
    const uint32_t rw = c == 0 ? sc.real_w[0] : c == 1 ? sc.real_w[1] : sc.real_w[2];
    const uint32_t rh = c == 0 ? sc.real_h[0] : c == 1 ? sc.real_h[1] : sc.real_h[2];
    const uint32_t bw = c == 0 ? sc.blocks_w[0] : c == 1 ? sc.blocks_w[1] : sc.blocks_w[2];
    const int16_t* p = c == 0 ? sc.coef[0] : c == 1 ? sc.coef[1] : sc.coef[2];
    while (by >= rh) {
        bx = (bx / mh) * mh + mh - 1;
        by--;
    }
    if (bx >= rw) bx = rw - 1;
    return p[((size_t)by * bw + bx) * 64];
}

template <bool RST>
HJ_HD PencDcRef penc_dc_locate(const PencScan& sc, uint32_t s)
{
    PencDcRef r;
    const uint32_t mcu = s / sc.bpm, k = s - mcu * sc.bpm;
    const uint32_t my = mcu / sc.mcus_x, mx = mcu - my * sc.mcus_x;
    uint32_t mh = 1, mv = 1, j = 0;
    r.c = 0;
    if (sc.ncomp == 3) {
        const uint32_t nl = sc.hs * sc.vs;
        if (k < nl) {
            j = k;
            mh = sc.hs;
            mv = sc.vs;
        } else {
            r.c = (int)(k - nl + 1);
        }
    }
    const uint32_t dy = j / mh, dx = j - dy * mh;
    r.dc = penc_dc_value(sc, r.c, mx * mh + dx, my * mv + dy);
    if (j > 0) {
        const uint32_t pj = j - 1, pdy = pj / mh, pdx = pj - pdy * mh;
        r.prev = penc_dc_value(sc, r.c, mx * mh + pdx, my * mv + pdy);
    } else if (mcu > 0 && !penc_starts_interval<RST>(sc, s - k)) {
        const uint32_t pm = mcu - 1, pmy = pm / sc.mcus_x, pmx = pm - pmy * sc.mcus_x;
        r.prev = penc_dc_value(sc, r.c, pmx * mh + (mh - 1), pmy * mv + (mv - 1));
    } else {
        r.prev = 0;
    }
    return r;
}

// ---- AC scans: one block's own symbols.  Out: sym(symbol), bits(value, n <= 32).  Returns the block's summary:
// bit 0 content, bit 1 tail, bits 2.. b (refinement: correction bits behind the last new coefficient, their values in *tail_bits).
template <class Out>
HJ_HD uint32_t penc_ac_first(const uint32_t (&w)[32], int ss, int se, int al, Out& o)
{
    int r = 0;
    uint32_t content = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
        if (k < ss || k > se) continue;
        const int v = penc_coef(w, k);
        const int t = v < 0 ? (-v) >> al : v >> al;
        if (t == 0) {
            r++;
            continue;
        }
        content = 1;
        while (r > 15) {
            o.sym(0xF0);
            r -= 16;
        }
        const int nb = penc_bit_length((uint32_t)t);
        o.sym((r << 4) + nb);
        o.bits((uint32_t)(v < 0 ? ~t : t), nb);
        r = 0;
    }
    return content | (r > 0 ? 2u : 0u);
}

template <class Out>
HJ_HD uint32_t penc_ac_refine(const uint32_t (&w)[32], int ss, int se, int al, Out& o, uint64_t* tail_bits)
{
    int eob = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
        if (k < ss || k > se) continue;
        const int v = penc_coef(w, k);
        if (((v < 0 ? -v : v) >> al) == 1) eob = k;
    }
    int r = 0;
    uint32_t br = 0;
    uint64_t corr = 0;  // buffered correction bits of this block, oldest first
#pragma unroll
    for (int k = 1; k < 64; k++) {
        if (k < ss || k > se) continue;
        const int v = penc_coef(w, k);
        const int t = (v < 0 ? -v : v) >> al;
        if (t == 0) {
            r++;
            continue;
        }
        while (r > 15 && k <= eob) {
            o.sym(0xF0);
            r -= 16;
            if (br > 32) o.bits((uint32_t)(corr >> 32), br - 32);
            o.bits((uint32_t)corr, br > 32 ? 32 : br);
            corr = 0;
            br = 0;
        }
        if (t > 1) {  // already non-zero: its next bit goes behind the coming symbol
            corr = (corr << 1) | (uint64_t)(t & 1);
            br++;
            continue;
        }
        o.sym((r << 4) + 1);
        o.bits(v < 0 ? 0u : 1u, 1);
        if (br > 32) o.bits((uint32_t)(corr >> 32), br - 32);
        o.bits((uint32_t)corr, br > 32 ? 32 : br);
        corr = 0;
        br = 0;
        r = 0;
    }
    *tail_bits = corr;
    return (eob > 0 ? 1u : 0u) | ((r > 0 || br > 0) ? 2u : 0u) | (br << 2);
}

// ---- the run recurrence: one step per block in scan order.  Flush words: n | be << 16 (0 = none).
struct PencRun {
    uint32_t n, be, ps;  // EOBRUN, buffered bits, first block of the pending piece
};
struct PencStep {
    uint32_t pre, pre_ps;    // flush in front of the block's symbols, and the first block of the piece it ends
    uint32_t post, post_ps;  // flush behind them (cut), likewise
    uint32_t rel, ps;        // tail blocks: bits buffered in front of this block's own, and the piece it joins
};

// The interval ends of a scan for a walk in scan order, without a division per block: at(i) for rising i says whether block i ends
// an interval (penc_ends_interval); blocks may be skipped as long as none in front of the next one asked for ends one (before).
template <bool RST>
struct PencIntervalEnds {
    uint32_t next, rst, n;  // next: the first block not yet passed that is the last of its interval
    HJ_HD PencIntervalEnds(uint32_t rst_blocks, uint32_t nblocks) : next(RST && rst_blocks ? rst_blocks - 1 : ~0u), rst(rst_blocks), n(nblocks) {}
    HJ_HD bool before(uint32_t end) const { return RST && next < end && next + 1 < n; }
    HJ_HD bool at(uint32_t i)
    {
        if (!RST || i != next) return false;
        next += rst;
        return i + 1 < n;
    }
};

// ends: block i ends an interval that another one follows (PencIntervalEnds::at); read with RST only.
template <bool RST>
HJ_HD PencStep penc_run_step(PencRun& r, uint32_t i, uint32_t summary, bool ends)
{
    PencStep o{0, 0, 0, 0, 0, 0};
    if (summary & 1) {
        if (r.n) {
            o.pre = r.n | (r.be << 16);
            o.pre_ps = r.ps;
        }
        r.n = r.be = 0;
    }
    if (summary & 2) {
        if (r.n == 0) r.ps = i;
        o.rel = r.be;
        o.ps = r.ps;
        r.n++;
        r.be += summary >> 2;
        if (r.n == kPencMaxRun || r.be > kPencMaxCorr) {
            o.post = r.n | (r.be << 16);
            o.post_ps = r.ps;
            r.n = r.be = 0;
        }
    }
    // emit_restart flushes the run in front of the next interval's first block; after a cut nothing is pending, so one post at most
    if (RST && ends && r.n) {
        o.post = r.n | (r.be << 16);
        o.post_ps = r.ps;
        r.n = r.be = 0;
    }
    return o;
}

// The end of the scan flushes what is pending (behind the last block's symbols).
HJ_HD uint32_t penc_run_end(const PencRun& r) { return r.n ? r.n | (r.be << 16) : 0u; }

HJ_HD int penc_eob_nbits(uint32_t n) { return 31 - __builtin_clz(n); }  // n >= 1

HJ_HD uint32_t penc_code_len(const uint32_t* codes, int sym) { return codes[sym] >> 16; }

// Bits a flush word occupies: EOBn code, n's low bits, the buffered correction bits.
HJ_HD uint32_t penc_flush_len(const uint32_t* codes, uint32_t f)
{
    if (!f) return 0;
    const int nb = penc_eob_nbits(f & 0xFFFF);
    return penc_code_len(codes, nb << 4) + nb + (f >> 16);
}

// Out policies of the AC routines.
struct PencLen {
    const uint32_t* codes;
    uint32_t len;
    HJ_HD void sym(int s) { len += codes[s] >> 16; }
    HJ_HD void bits(uint32_t, int n) { len += n; }
};
// Bit writer into a zeroed buffer of big-endian 32-bit words: W::or_word(index, bits in stream order).
template <class W>
struct PencBits {
    W words;
    const uint32_t* codes;
    uint64_t acc;
    uint32_t n, widx;
    HJ_HD void start(uint32_t pos)
    {
        acc = 0;
        n = pos & 31;
        widx = pos >> 5;
    }
    HJ_HD void put(uint32_t v, int size)  // size <= 32
    {
        if (!size) return;
        acc = (acc << size) | (size == 32 ? (uint64_t)v : (uint64_t)(v & ((1u << size) - 1)));
        n += size;
        if (n >= 32) {
            words.or_word(widx++, (uint32_t)(acc >> (n - 32)));
            n -= 32;
        }
    }
    HJ_HD void sym(int s) { put(codes[s] & 0xFFFF, (int)(codes[s] >> 16)); }
    HJ_HD void bits(uint32_t v, int nb) { put(v, nb); }
    HJ_HD void finish()
    {
        if (n > 0) words.or_word(widx, (uint32_t)(acc << (32 - n)));
        n = 0;
    }
    HJ_HD void flush(uint32_t f)  // EOBn code and n's low bits (the buffered bits follow from their owners)
    {
        const uint32_t run = f & 0xFFFF;
        const int nb = penc_eob_nbits(run);
        sym(nb << 4);
        if (nb) put(run, nb);
    }
};

// ---- one block of a scan, for the kernels and the host emulation alike

// The 64 coefficients of AC-scan block i (real blocks in raster order), two per word.
HJ_HD void penc_load_block(const PencScan& sc, uint32_t i, uint32_t (&w)[32])
{
    const uint32_t by = i / sc.arw, bx = i - by * sc.arw;
    const uint4* p = reinterpret_cast<const uint4*>(sc.acoef + ((size_t)by * sc.abw + bx) * 64);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 q = p[j];
        w[4 * j] = q.x;
        w[4 * j + 1] = q.y;
        w[4 * j + 2] = q.z;
        w[4 * j + 3] = q.w;
    }
}

// DC first scans: the category symbol (table slot * 16 + category), the value bits and their number.
struct PencDcSymbol {
    int sym, nb;
    uint32_t bits;
};
template <bool RST>
HJ_HD PencDcSymbol penc_dc_symbol(const PencScan& sc, uint32_t i)
{
    const PencDcRef r = penc_dc_locate<RST>(sc, i);
    const int d = (r.dc >> sc.al) - (r.prev >> sc.al);  // arithmetic shifts (IRIGHT_SHIFT)
    const int nb = penc_bit_length((uint32_t)(d < 0 ? -d : d));
    return PencDcSymbol{(r.c ? 16 : 0) + nb, nb, (uint32_t)(d < 0 ? d - 1 : d)};
}

// Symbol statistics of block i (Count: sym(symbol), bits() ignored); returns the summary of an AC-scan block (0 for DC scans).
template <bool RST, class Count>
HJ_HD uint32_t penc_block_summary(const PencScan& sc, uint32_t i, Count& cnt)
{
    if (sc.kind == kPencDcRefine) return 0;
    if (sc.kind == kPencDcFirst) {
        cnt.sym(penc_dc_symbol<RST>(sc, i).sym);
        return 0;
    }
    uint32_t w[32];
    penc_load_block(sc, i, w);
    uint64_t tail;
    return sc.kind == kPencAcFirst ? penc_ac_first(w, (int)sc.ss, (int)sc.se, (int)sc.al, cnt)
                                   : penc_ac_refine(w, (int)sc.ss, (int)sc.se, (int)sc.al, cnt, &tail);
}

// The run resolution's results, indexed by the block's position in its scan.
struct PencBlockArrays {
    const uint8_t* sum;      // summaries (AC scans)
    const uint32_t* pre;     // flush words
    const uint32_t* post;
    const uint32_t* piece;   // tail blocks with b > 0: first block of their piece ...
    const uint32_t* flusher; // ... and, indexed by that first block, the block that flushes the piece
    const uint16_t* rel;     // tail blocks with b > 0: buffered bits of the piece in front of theirs
    const uint16_t* own;     // bits of the block's own symbols
    const uint16_t* bits;    // bits the block's lane lays down in sequence: pre flush, own symbols, post flush
    const uint32_t* off;     // exclusive prefix sum of bits
};

// Bits of block i: own symbols (*own) plus the flushes in front of and behind them.
template <bool RST>
HJ_HD uint32_t penc_block_length(const PencScan& sc, uint32_t i, const uint32_t* codes, uint32_t pre, uint32_t post, uint32_t* own)
{
    if (sc.kind == kPencDcRefine) {
        *own = 1;
        return 1;
    }
    if (sc.kind == kPencDcFirst) {
        const PencDcSymbol d = penc_dc_symbol<RST>(sc, i);
        *own = (codes[d.sym] >> 16) + d.nb;
        return *own;
    }
    uint32_t w[32];
    penc_load_block(sc, i, w);
    PencLen o{codes, 0};
    uint64_t tail;
    if (sc.kind == kPencAcFirst)
        penc_ac_first(w, (int)sc.ss, (int)sc.se, (int)sc.al, o);
    else
        penc_ac_refine(w, (int)sc.ss, (int)sc.se, (int)sc.al, o, &tail);
    *own = o.len;
    return penc_flush_len(codes, pre) + o.len + penc_flush_len(codes, post);
}

// Writes everything block i owns into the scan's zeroed bit buffer (W: or_word), the final byte's padding included.  RST: the last
// block of an interval pads behind all it lays down (its flushes and the buffered bits other lanes OR into them lie in front of
// off + bits[i]) and writes RSTn at the byte boundary (jcphuff.c emit_restart).  Returns the byte of the bit buffer that holds the
// marker's FF, or ~0u when there is none.
template <bool RST, class W>
HJ_HD uint32_t penc_block_write(const PencScan& sc, uint32_t i, const uint32_t* codes, const W& words, const PencBlockArrays& a)
{
    PencBits<W> em{words, codes, 0, 0, 0};
    const uint32_t off = a.off[i];
    if (sc.kind == kPencDcRefine) {
        em.start(off);
        em.put((uint32_t)(penc_dc_locate<false>(sc, i).dc >> sc.al) & 1u, 1);
        em.finish();
    } else if (sc.kind == kPencDcFirst) {
        const PencDcSymbol d = penc_dc_symbol<RST>(sc, i);
        em.start(off);
        em.sym(d.sym);
        em.put(d.bits, d.nb);
        em.finish();
    } else {
        const uint32_t pre = a.pre[i], post = a.post[i];
        uint32_t w[32];
        penc_load_block(sc, i, w);
        uint32_t pos = off;
        if (pre) {
            em.start(pos);
            em.flush(pre);
            em.finish();
            pos += penc_flush_len(codes, pre);  // the piece's buffered bits come from their blocks
        }
        em.start(pos);
        uint64_t tail = 0;
        const uint32_t s = sc.kind == kPencAcFirst ? penc_ac_first(w, (int)sc.ss, (int)sc.se, (int)sc.al, em)
                                                   : penc_ac_refine(w, (int)sc.ss, (int)sc.se, (int)sc.al, em, &tail);
        if (post) em.flush(post);
        em.finish();
        const uint32_t b = s >> 2;
        if ((s & 2) && b) {  // this block's trailing correction bits, in its piece's flush
            const uint32_t f = a.flusher[a.piece[i]];
            uint32_t dst;
            if (f > i && (a.sum[f] & 1))
                dst = a.off[f] + penc_flush_len(codes, a.pre[f]) - (a.pre[f] >> 16);
            else
                dst = a.off[f] + penc_flush_len(codes, a.pre[f]) + a.own[f] + penc_flush_len(codes, a.post[f]) - (a.post[f] >> 16);
            em.start(dst + a.rel[i]);
            if (b > 32) em.put((uint32_t)(tail >> 32), (int)b - 32);
            em.put((uint32_t)tail, b > 32 ? 32 : (int)b);
            em.finish();
        }
    }
    const bool ends = penc_ends_interval<RST>(sc.rst_blocks, sc.nblocks, i);
    if (!ends && i != sc.nblocks - 1) return ~0u;
    // jchuff.c flush_bits: the last byte of the scan -- and of every restart interval -- is filled up with one-bits
    const uint32_t end = off + a.bits[i], padn = (8 - (end & 7)) & 7;
    if (padn || ends) {
        em.start(end);
        if (padn) em.put((1u << padn) - 1, (int)padn);
        if (ends) em.put(0xFF00u | (0xD0u + ((i / sc.rst_blocks) & 7u)), 16);  // n = interval index mod 8 (henc_marker_number)
        em.finish();
    }
    return ends ? (end + padn) >> 3 : ~0u;
}

}  // namespace hipjpeg
