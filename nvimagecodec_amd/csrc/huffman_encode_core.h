// huffman_encode_core.h -- the per-block routines and the restart-interval arithmetic of the GPU coder's baseline output.  Compiles
// for host and device: the kernels (gpu_huffman_encode.hip) and the host emulation (gpu_huffman_encode_host.cpp) run this very code.
//
// A scan with restart intervals (jchuff.c emit_restart) keeps the per-block independence of one without: an interval is a run of
// HencImage::rst_blocks blocks in scan order (whole MCUs), and
//   predictor  the first block of each component in an interval has no previous block (henc_locate<true>); the DC *value* of a
//              dummy block is still that of the preceding block in MCU order, wherever that block lies (henc_dc_value)
//   offsets    the bit offset behind an interval's last block is rounded up to a byte and 16 bits are added for the marker, which
//              lives in the bit buffer: HencSpan is the partial result of a range of blocks, henc_span_join its associative operator
//   padding    the lane of an interval's last block fills the byte with one-bits (data: a 0xFF that comes out of it is stuffed)
//              and writes FF Dn behind it, n = interval index mod 8 (henc_finish_block)
//   markers    that lane also sets the marker's bit in a bitmap, one bit per byte of the bit buffer, which lies behind the buffer
//              and is zeroed with it; the count / expand kernels mask their 0xFF tests with it (henc_marker_mask /
//              henc_is_marker), because all 256 byte values occur as data and a marker cannot be recognised in band
// Nothing follows the last interval: the image's last block only pads, as it does without restart intervals.
#pragma once
#include <cstdint>

#include "gpu_huffman_encode.h"
#include "huffman_gpu_core.h"  // HJ_HD

namespace hipjpeg {

// Where block s of the scan (MCU order) lives, and where the previous block of the same component is.
struct HencBlockRef {
    int c;              // component
    uint32_t bx, by;    // block coordinates in the component's grid
    bool has_prev;
    uint32_t pbx, pby;  // the same component's previous block in scan order (DC predictor)
};

// RST: the image may have restart intervals (rst_blocks != 0); false compiles the interval arithmetic away.
template <bool RST>
HJ_HD bool henc_starts_interval(const HencImage& im, uint32_t first_block_of_mcu)
{
    return RST && im.rst_blocks != 0 && first_block_of_mcu % im.rst_blocks == 0;
}

// Block s is the last of an interval that another one follows (the image's last block never is).
template <bool RST>
HJ_HD bool henc_ends_interval(const HencImage& im, uint32_t s)
{
    return RST && im.rst_blocks != 0 && s + 1 < im.total_blocks && (s + 1) % im.rst_blocks == 0;
}

// RSTn behind the interval that block s ends
HJ_HD uint32_t henc_marker_number(const HencImage& im, uint32_t s) { return (s / im.rst_blocks) & 7u; }

template <bool RST>
HJ_HD HencBlockRef henc_locate(const HencImage& im, uint32_t s)
{
    HencBlockRef r;
    const uint32_t mcu = s / im.bpm, k = s - mcu * im.bpm;
    const uint32_t my = mcu / im.mcus_x, mx = mcu - my * im.mcus_x;
    uint32_t mh = 1, mv = 1, j = 0;
    r.c = 0;
    if (im.ncomp == 3) {
        const uint32_t nl = im.hs * im.vs;
        if (k < nl) {
            j = k;
            mh = im.hs;
            mv = im.vs;
        } else {
            r.c = (int)(k - nl + 1);
        }
    }
    const uint32_t dy = j / mh, dx = j - dy * mh;
    r.bx = mx * mh + dx;
    r.by = my * mv + dy;
    if (j > 0) {
        const uint32_t pj = j - 1, pdy = pj / mh, pdx = pj - pdy * mh;
        r.has_prev = true;
        r.pbx = mx * mh + pdx;
        r.pby = my * mv + pdy;
    } else if (mcu > 0 && !henc_starts_interval<RST>(im, s - k)) {
        const uint32_t pm = mcu - 1, pmy = pm / im.mcus_x, pmx = pm - pmy * im.mcus_x;
        r.has_prev = true;
        r.pbx = pmx * mh + (mh - 1);
        r.pby = pmy * mv + (mv - 1);
    } else {
        r.has_prev = false;
        r.pbx = r.pby = 0;
    }
    return r;
}

// DC value libjpeg gives a block: real blocks their own; dummy blocks the DC of the preceding block in MCU order
// (entropy_encode.cpp BlockSource::dc_of).
HJ_HD int henc_dc_value(const HencImage& im, int c, uint32_t bx, uint32_t by)
{
    const uint32_t mh = (c == 0 && im.ncomp == 3) ? im.hs : 1;
    while (by >= im.real_h[c]) {
        bx = (bx / mh) * mh + mh - 1;
        by--;
    }
    if (bx >= im.real_w[c]) bx = im.real_w[c] - 1;
    return im.coef[c][((size_t)by * im.blocks_w[c] + bx) * 64];
}

HJ_HD int henc_bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// Bit sink of the write step: bits go into 32-bit words of the stream (most significant bit first), each handed to
// Words::or_word(word index, value) once full -- the block's first and last word are partial and shared with its neighbours.
template <class Words>
struct HencEmitter {
    Words words;
    unsigned long long acc;
    uint32_t n;        // valid bits at the low end of acc
    uint32_t widx;     // next word
    uint32_t emitted;  // bits of this block so far
    HJ_HD void start(const Words& w, uint32_t off)
    {
        words = w;
        acc = 0;
        n = off & 31;
        widx = off >> 5;
        emitted = 0;
    }
    HJ_HD void put(uint32_t bits, uint32_t size)  // size <= 16, bits already masked
    {
        acc = (acc << size) | bits;
        n += size;
        emitted += size;
        if (n >= 32) {
            words.or_word(widx++, (uint32_t)(acc >> (n - 32)));
            n -= 32;
        }
    }
    HJ_HD void finish()
    {
        if (n > 0) words.or_word(widx++, (uint32_t)(acc << (32 - n)));
    }
};

// One block.  w = its 64 coefficients in zigzag order (two per dword), ignored for dummy blocks.  Returns the bit length.
// Tables: StandardCodeTables' layout (in LDS on the device).
template <bool WRITE, class Tables, class Em>
HJ_HD uint32_t henc_code_block(const uint32_t (&w)[32], bool real, int diff, const Tables* T, int ti, Em* em)
{
    uint32_t len;
    {
        const unsigned t = (unsigned)(diff < 0 ? -diff : diff);
        const int nb = henc_bit_length(t);
        const uint32_t size = T->dc_size[ti][nb];
        len = size + nb;
        if (WRITE) {
            em->put(T->dc_code[ti][nb], size);
            if (nb) em->put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
        }
    }
    if (!real) {  // dummy block: all AC zero -> EOB
        const uint32_t size = T->ac_size[ti][0];
        if (WRITE) em->put(T->ac_code[ti][0], size);
        return len + size;
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
        const int v = (k & 1) ? ((int)w[k >> 1] >> 16) : ((int)(w[k >> 1] << 16) >> 16);
        if (v == 0) {
            run++;
            continue;
        }
        while (run > 15) {  // ZRL
            const uint32_t size = T->ac_size[ti][0xF0];
            len += size;
            if (WRITE) em->put(T->ac_code[ti][0xF0], size);
            run -= 16;
        }
        const int nb = henc_bit_length((unsigned)(v < 0 ? -v : v));
        const int sym = (run << 4) + nb;
        const uint32_t size = T->ac_size[ti][sym];
        len += size + nb;
        if (WRITE) {
            em->put(T->ac_code[ti][sym], size);
            em->put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1), nb);
        }
        run = 0;
    }
    if (run > 0) {
        const uint32_t size = T->ac_size[ti][0];
        len += size;
        if (WRITE) em->put(T->ac_code[ti][0], size);
    }
    return len;
}

// The symbols of one block, counted instead of coded (jchuff.c htest_one_block): Count::add(0, category) for the DC difference,
// Count::add(1, run/size) for the coefficients, ZRL and EOB included -- the same walk as henc_code_block.
template <class Count>
HJ_HD void henc_count_block(const uint32_t (&w)[32], bool real, int diff, const Count& count)
{
    count.add(0, henc_bit_length((unsigned)(diff < 0 ? -diff : diff)));
    if (!real) {
        count.add(1, 0);
        return;
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
        const int v = (k & 1) ? ((int)w[k >> 1] >> 16) : ((int)(w[k >> 1] << 16) >> 16);
        if (v == 0) {
            run++;
            continue;
        }
        while (run > 15) {
            count.add(1, 0xF0);
            run -= 16;
        }
        count.add(1, (run << 4) + henc_bit_length((unsigned)(v < 0 ? -v : v)));
        run = 0;
    }
    if (run > 0) count.add(1, 0);
}

// ---- offsets: the segmented scan
// What a range of consecutive blocks does to the running bit offset x.  No interval ends inside it: x + a.  Otherwise: a bits up
// to the end of the first interval's last block, where x + a is rounded up to a byte; from that byte boundary on the range is
// b bits long whatever x was (markers and later paddings included).
struct HencSpan {
    uint32_t a, b, cut;
};

HJ_HD uint32_t henc_byte_up(uint32_t bits) { return (bits + 7u) & ~7u; }

HJ_HD HencSpan henc_span_block(uint32_t bits, bool ends_interval) { return HencSpan{bits, ends_interval ? 16u : 0u, ends_interval ? 1u : 0u}; }

HJ_HD uint32_t henc_span_apply(uint32_t x, const HencSpan& r) { return r.cut ? henc_byte_up(x + r.a) + r.b : x + r.a; }

// l, then r
HJ_HD HencSpan henc_span_join(const HencSpan& l, const HencSpan& r)
{
    if (!l.cut) return HencSpan{l.a + r.a, r.b, r.cut};
    return HencSpan{l.a, henc_span_apply(l.b, r), 1u};
}

// ---- padding and markers
// What follows the symbols of block s, which start at bit `off` and have been put into em: jchuff.c flush_bits fills the last byte
// of an interval (or of the scan) with one-bits; emit_restart writes RSTn behind an interval.  Returns the byte of the bit buffer
// that holds the marker's FF, or ~0u when there is none.
template <bool RST, class Em>
HJ_HD uint32_t henc_finish_block(const HencImage& im, uint32_t s, uint32_t off, Em* em)
{
    const bool ends = henc_ends_interval<RST>(im, s);
    if (!ends && s != im.total_blocks - 1) return ~0u;
    const uint32_t end = off + em->emitted;
    const uint32_t padn = (8 - (end & 7)) & 7;
    if (padn) em->put((1u << padn) - 1, padn);
    if (!ends) return ~0u;
    em->put(0xFF00u | (0xD0u + henc_marker_number(im, s)), 16);
    return henc_byte_up(end) >> 3;
}

// The marker bitmap: bit i of dword i / 32 = byte i of the bit buffer is a marker's FF (little-endian, so that halfword p covers
// the 16-byte piece p).
HJ_HD uint32_t henc_map_offset(uint32_t raw_bytes) { return (raw_bytes + 16u + 15u) & ~15u; }  // behind the buffer and its slack
HJ_HD uint32_t henc_map_bytes(uint32_t raw_bytes) { return ((raw_bytes + 7u) / 8u + 4u + 15u) & ~15u; }
HJ_HD bool henc_is_marker(const uint16_t* map, uint32_t byte) { return (map[byte >> 4] >> (byte & 15)) & 1; }
// 0x80 in every byte of a dword whose bit in the four map bits `nib` is set (what ff_mask gives for a 0xFF byte)
HJ_HD uint32_t henc_marker_mask(uint32_t nib) { return ((nib * 0x00204081u) & 0x01010101u) << 7; }

}  // namespace hipjpeg
