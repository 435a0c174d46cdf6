// lossless_encode_core.h -- the per-sample routines of the lossless (SOF3) coder, as libjpeg-turbo's jclossls.c / jclhuff.c run them.
// Compiles for host and device: the kernels (lossless_encode_kernels.hip), their schedule run on the host and the plain host coder
// (lossless_encode_host.cpp) share this very code, as the decoder's sides share lossless_core.h.
//
// State x = sample >> Pt.  The prediction comes from the states a (left), b (above), c (above-left) of the INPUT, so every sample is
// independent: first sample of the picture and of every restart interval 1 << (P - Pt - 1), rest of that row a, column 0 of every
// other row b, elsewhere predictors 1..7 (lossless_core.h).  Difference = (x - prediction) & 0xFFFF; its category SSSS is 0 for 0,
// 16 for 32768 (no extra bits), otherwise the bit length of |d|, followed by SSSS extra bits (d, or d - 1 when negative).
// One scan holds all components, interleaved sample by sample; scan index s = (row * width + col) * ncomp + component.
//
// The kernels' shape: a lane codes a GROUP of kLencGroup consecutive samples of the scan, a workgroup kLencThreads groups.  Groups
// ignore rows and restart intervals, so an interval may end inside a group (several may: narrow pictures).  What a group does to the
// running bit offset is therefore a HencSpan (huffman_encode_core.h) and the offsets come from a segmented scan over spans.
#pragma once
#include <cstdint>

#include "huffman_encode_core.h"  // HencSpan, HencEmitter, henc_byte_up, henc_map_offset
#include "lossless_core.h"

// The samples are the caller's device memory, described by 64-bit addresses: in device code they are read through global-address-space
// pointers, so that the loads are global_load_* and not flat_load_*.
#if defined(__HIP_DEVICE_COMPILE__)
#define HJ_LL_GLOBAL __attribute__((address_space(1)))
#else
#define HJ_LL_GLOBAL
#endif

namespace hipjpeg {

typedef uint32_t lenc_vec16 __attribute__((vector_size(16)));
typedef lenc_vec16 lenc_vec16_u __attribute__((aligned(1)));  // 16 bytes at any alignment
typedef uint32_t lenc_vec8 __attribute__((vector_size(8)));
typedef lenc_vec8 lenc_vec8_u __attribute__((aligned(1)));
typedef uint16_t lenc_u16_u __attribute__((aligned(1)));

constexpr int kLencGroup = 8;      // samples per lane (G): at most 31 * 8 bits
constexpr int kLencThreads = 256;  // lanes of a workgroup of every coder kernel
constexpr int kLencWindowSamples = kLencGroup * kLencThreads;
// the write kernel's LDS window holds any workgroup's bits: 31 per sample, and behind a sample that ends an interval up to 7 padding
// bits and the marker's 16; two words for the ragged ends
constexpr int kLencWindowWords = (kLencWindowSamples * (31 + 7 + 16) + 31) / 32 + 2;
constexpr int kLencStatVector = 16;  // bytes a lane of the statistics pass loads at once

// One picture as the kernels see it.  32- and 64-bit members only (tests/test_code_object_hazards.py); the per-component members are
// read through lenc_plane / lenc_pitch, never with a computed index.
struct alignas(16) LencImage {
    uint64_t plane0, plane1, plane2, plane3;  // sample (0, 0) of each component
    uint32_t pitch0, pitch1, pitch2, pitch3;  // bytes from a row to the next
    uint32_t step;                            // bytes from a sample to the next of the same component
    uint32_t sample_bytes;                    // 1 or 2
    uint32_t width, height, ncomp;
    uint32_t ps, pt, init;      // init = 1 << (P - Pt - 1)
    uint32_t interval_rows;     // rows per restart interval; `height` when the file has none
    uint32_t row_samples;       // width * ncomp
    uint32_t total_samples;     // height * row_samples
    uint32_t interval_samples;  // interval_rows * row_samples
    uint32_t first_group;       // index of the picture's first group in the batch-wide per-group arrays
    uint32_t num_groups;
    uint32_t index;             // the picture's place in the per-image arrays (counts, codes, totals, HencImage)
    uint32_t pad0;
    uint64_t counts;            // uint32[kLencSymbols], zeroed by the batch
    uint64_t codes;             // uint32[kLencSymbols]: code | size << 16, there once the host has built the table
};
constexpr int kLencSymbols = 17;
constexpr int kLencCountStride = 32;  // words between two pictures' counters / codes

HJ_LL_HD uint64_t lenc_plane(const LencImage& im, uint32_t c) { return c == 0 ? im.plane0 : c == 1 ? im.plane1 : c == 2 ? im.plane2 : im.plane3; }
HJ_LL_HD uint32_t lenc_pitch(const LencImage& im, uint32_t c) { return c == 0 ? im.pitch0 : c == 1 ? im.pitch1 : c == 2 ? im.pitch2 : im.pitch3; }

// the state at (row, col) of component c
HJ_LL_HD int lenc_state(const LencImage& im, uint32_t c, uint32_t row, uint32_t col)
{
    const HJ_LL_GLOBAL uint8_t* p =
        reinterpret_cast<const HJ_LL_GLOBAL uint8_t*>(lenc_plane(im, c) + (uint64_t)row * lenc_pitch(im, c) + (uint64_t)col * im.step);
    const uint32_t v = im.sample_bytes == 1 ? (uint32_t)p[0] : (uint32_t)*reinterpret_cast<const HJ_LL_GLOBAL lenc_u16_u*>(p);  // any alignment
    return (int)(v >> im.pt);
}

// difference of a sample from its state x and its neighbours' states (those a sample does not have are not looked at)
HJ_LL_HD uint32_t lenc_difference(const LencImage& im, uint32_t row, uint32_t col, int x, int a, int b, int c)
{
    const bool first_row = row % im.interval_rows == 0;
    return (uint32_t)(x - lossless_predict_at((int)im.ps, first_row, col, (int)im.init, a, b, c)) & 0xFFFFu;
}

// difference of the sample at (row, col) of component c, everything loaded here
HJ_LL_HD uint32_t lenc_difference_at(const LencImage& im, uint32_t row, uint32_t col, uint32_t c)
{
    const bool first_row = row % im.interval_rows == 0;
    const int x = lenc_state(im, c, row, col);
    const int a = col ? lenc_state(im, c, row, col - 1) : 0;
    int b = 0, cc = 0;
    if (!first_row) {
        b = lenc_state(im, c, row - 1, col);
        if (col && im.ps >= 3) cc = lenc_state(im, c, row - 1, col - 1);
    }
    return lenc_difference(im, row, col, x, a, b, cc);
}

// difference of sample s of the scan
HJ_LL_HD uint32_t lenc_sample_difference(const LencImage& im, uint32_t s)
{
    const uint32_t row = s / im.row_samples, rem = s - row * im.row_samples;
    const uint32_t col = rem / im.ncomp, c = rem - col * im.ncomp;
    return lenc_difference_at(im, row, col, c);
}

// SSSS of a difference (0 .. 65535, read as -32767 .. 32768)
HJ_LL_HD uint32_t lenc_category(uint32_t d)
{
    const int v = d > 32768u ? (int)d - 65536 : (int)d;
    return (uint32_t)henc_bit_length((unsigned)(v < 0 ? -v : v));
}

// code word and extra bits of a difference as one bit string; entry = code | size << 16 of its category
HJ_LL_HD uint32_t lenc_symbol(uint32_t d, uint32_t entry, uint32_t* nbits)
{
    const uint32_t ssss = lenc_category(d);
    const uint32_t extra = ssss == 16 ? 0u : ssss;
    const int v = d > 32768u ? (int)d - 65536 : (int)d;
    const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << extra) - 1u);
    *nbits = (entry >> 16) + extra;  // at most 16 + 15
    return ((entry & 0xFFFFu) << extra) | low;
}

// ---- the statistics pass walks rows, not groups: a workgroup step takes a PIECE, kLencStatPiece bytes of one row of one plane (the
// one interleaved plane, or a component's), a lane kLencStatVector bytes of it -- one 16-byte load where the vector lies wholly inside
// the row's width * sample_bytes, single samples at the ragged end.  Nothing beyond the row's bytes is loaded.
constexpr int kLencStatPiece = kLencThreads * kLencStatVector;

HJ_LL_HD uint32_t lenc_planes(const LencImage& im) { return im.step == im.sample_bytes ? im.ncomp : 1u; }  // planes a row is spread over
HJ_LL_HD uint32_t lenc_row_bytes(const LencImage& im) { return im.width * im.step; }
HJ_LL_HD uint32_t lenc_row_pieces(const LencImage& im) { return (lenc_row_bytes(im) + kLencStatPiece - 1) / kLencStatPiece; }
HJ_LL_HD uint32_t lenc_pieces(const LencImage& im) { return im.height * lenc_planes(im) * lenc_row_pieces(im); }

// the sample of SB bytes at byte `off` (a compile-time value at every call) of little-endian words
template <int SB>
HJ_LL_HD int lenc_word_sample(const uint32_t* w, int off)
{
    return (int)((w[off >> 2] >> (8 * (off & 3))) & (SB == 1 ? 0xFFu : 0xFFFFu));
}

HJ_LL_HD void lenc_load16(uint64_t address, uint32_t* w)
{
    const lenc_vec16 v = *reinterpret_cast<const HJ_LL_GLOBAL lenc_vec16_u*>(address);
    w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
}
HJ_LL_HD void lenc_load8(uint64_t address, uint32_t* w)
{
    const lenc_vec8 v = *reinterpret_cast<const HJ_LL_GLOBAL lenc_vec8_u*>(address);
    w[0] = v[0], w[1] = v[1];
}

// A whole vector at byte o of plane q's row: SB = sample bytes, NS = samples between a sample and its left neighbour (the component
// count of an interleaved row, 1 in a plane of its own); NS * SB <= 8, so the eight bytes in front of the vector hold every left
// neighbour the vector itself does not.
template <int SB, int NS, class Count>
HJ_LL_HD void lenc_stat_vector(const LencImage& im, uint32_t row, uint32_t q, uint32_t o, const Count& count)
{
    const uint64_t cur = lenc_plane(im, q) + (uint64_t)row * lenc_pitch(im, q) + o;
    const bool first_row = row % im.interval_rows == 0;
    uint32_t wc[6] = {0u, 0u, 0u, 0u, 0u, 0u}, wu[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    lenc_load16(cur, &wc[2]);
    if (o) lenc_load8(cur - 8, &wc[0]);
    if (!first_row) {
        const uint64_t up = cur - lenc_pitch(im, q);
        lenc_load16(up, &wu[2]);
        if (o) lenc_load8(up - 8, &wu[0]);
    }
    const uint32_t e0 = o / SB;  // the vector's first sample in the row of this plane
#pragma unroll
    for (int j = 0; j < 16 / SB; j++) {
        const uint32_t col = (e0 + (uint32_t)j) / NS;
        const int x = lenc_word_sample<SB>(wc, 8 + j * SB) >> im.pt, a = lenc_word_sample<SB>(wc, 8 + (j - NS) * SB) >> im.pt;
        const int b = lenc_word_sample<SB>(wu, 8 + j * SB) >> im.pt, c = lenc_word_sample<SB>(wu, 8 + (j - NS) * SB) >> im.pt;
        count.add(lenc_category(lenc_difference(im, row, col, x, a, b, c)));
    }
}

// Lane t of the workgroup step that takes piece `piece` of the picture
template <class Count>
HJ_LL_HD void lenc_stat_lane(const LencImage& im, uint32_t piece, uint32_t t, const Count& count)
{
    const uint32_t planes = lenc_planes(im), per_row = lenc_row_pieces(im), row_bytes = lenc_row_bytes(im);
    const uint32_t row = piece / (planes * per_row), rem = piece - row * planes * per_row;
    const uint32_t q = rem / per_row, k = rem - q * per_row;
    const uint32_t o = k * (uint32_t)kLencStatPiece + t * (uint32_t)kLencStatVector;
    if (o >= row_bytes) return;
    const uint32_t ns = planes == 1 ? im.ncomp : 1u;
    if (o + kLencStatVector > row_bytes) {  // the ragged end: sample by sample
        for (uint32_t e = o / im.sample_bytes; e * im.sample_bytes < row_bytes; e++) {
            const uint32_t col = e / ns;
            count.add(lenc_category(lenc_difference_at(im, row, col, planes == 1 ? e - col * ns : q)));
        }
        return;
    }
    if (im.sample_bytes == 2) {
        if (ns == 1) lenc_stat_vector<2, 1>(im, row, q, o, count);
        else if (ns == 2) lenc_stat_vector<2, 2>(im, row, q, o, count);
        else if (ns == 3) lenc_stat_vector<2, 3>(im, row, q, o, count);
        else lenc_stat_vector<2, 4>(im, row, q, o, count);
    } else {
        if (ns == 1) lenc_stat_vector<1, 1>(im, row, q, o, count);
        else if (ns == 2) lenc_stat_vector<1, 2>(im, row, q, o, count);
        else if (ns == 3) lenc_stat_vector<1, 3>(im, row, q, o, count);
        else lenc_stat_vector<1, 4>(im, row, q, o, count);
    }
}

// sample s is the last of an interval that another one follows
HJ_LL_HD bool lenc_ends_interval(const LencImage& im, uint32_t s) { return (s + 1) % im.interval_samples == 0 && s + 1 < im.total_samples; }

// ---- spans packed into a word: a (bits 0..11), b (bits 12..30), cut (bit 31).  A group's a is at most 31 * G; its b at most
// (G - 1) * (31 + 7 + 16) + 16.
static_assert(31 * kLencGroup < (1 << 12) && kLencGroup * 54 < (1 << 19), "span packing");
HJ_LL_HD uint32_t lenc_pack_span(const HencSpan& s) { return s.a | (s.b << 12) | (s.cut << 31); }
HJ_LL_HD HencSpan lenc_unpack_span(uint32_t w) { return HencSpan{w & 0xFFFu, (w >> 12) & 0x7FFFFu, w >> 31}; }

// What group g does to the running bit offset (Codes: uint32[17] in LDS or host memory)
template <class Codes>
HJ_LL_HD HencSpan lenc_group_span(const LencImage& im, uint32_t g, const Codes* codes)
{
    HencSpan sp{0u, 0u, 0u};
    const uint32_t s0 = g * (uint32_t)kLencGroup;
    for (uint32_t k = 0; k < (uint32_t)kLencGroup && s0 + k < im.total_samples; k++) {
        const uint32_t d = lenc_sample_difference(im, s0 + k);
        uint32_t nbits;
        (void)lenc_symbol(d, codes[lenc_category(d)], &nbits);
        sp = henc_span_join(sp, henc_span_block(nbits, lenc_ends_interval(im, s0 + k)));
    }
    return sp;
}

// Writes group g, which starts at bit `off`, into em; behind a sample that ends an interval the padding and RSTn, behind the picture's
// last sample the padding.  mark(byte): that byte of the bit buffer holds a marker's FF.
template <class Codes, class Em, class Mark>
HJ_LL_HD void lenc_group_write(const LencImage& im, uint32_t g, uint32_t off, const Codes* codes, Em* em, const Mark& mark)
{
    const uint32_t s0 = g * (uint32_t)kLencGroup;
    for (uint32_t k = 0; k < (uint32_t)kLencGroup && s0 + k < im.total_samples; k++) {
        const uint32_t s = s0 + k;
        const uint32_t d = lenc_sample_difference(im, s);
        uint32_t nbits;
        const uint32_t bits = lenc_symbol(d, codes[lenc_category(d)], &nbits);
        if (nbits > 16) {
            em->put(bits >> 16, nbits - 16);
            em->put(bits & 0xFFFFu, 16);
        } else {
            em->put(bits, nbits);
        }
        const bool ends = lenc_ends_interval(im, s);
        if (!ends && s + 1 != im.total_samples) continue;
        const uint32_t end = off + em->emitted;
        const uint32_t padn = (8 - (end & 7)) & 7;
        if (padn) em->put((1u << padn) - 1, padn);
        if (ends) {
            em->put(0xFF00u | (0xD0u + ((s / im.interval_samples) & 7u)), 16);
            mark(henc_byte_up(end) >> 3);
        }
    }
}

// ---- the uint32 bit-offset predicate: 31 bits per sample and 24 per interval (7 padding bits, the marker, rounded up) must fit
HJ_LL_HD bool lenc_offsets_fit(uint64_t samples, uint64_t intervals) { return 31u * samples + 24u * intervals <= 0xFFFFFFFFull; }

}  // namespace hipjpeg
