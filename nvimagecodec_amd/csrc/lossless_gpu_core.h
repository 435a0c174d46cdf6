// lossless_gpu_core.h -- the GPU entropy stage of the lossless (SOF3) decoder: what a lane does, compiled once for the kernels
// (lossless_entropy_kernels.hip) and for their host twin (lossless_gpu_host.cpp), which runs the same schedule lane by lane.
//
// Stream model.  Behind the destuffing a scan is a run of samples: a Huffman code of up to 16 bits from the table of the component
// whose turn it is, then SSSS extra bits (none for SSSS 0 and 16), 31 bits at the most.  Components alternate per pixel, so a parser's
// state at a bit is (bit position, component phase).  Where every component names the same table the phase has no say in the parse:
// the walks then keep it at 0 (LlImage::ntables == 1), or a constant picture would never synchronise.
//
// Segments.  A file without restart intervals is one segment; with them every interval is one: byte-aligned, whole rows, entered at
// phase 0 with a known first sample.  The host finds the markers with a byte scan and checks their order; it decodes nothing.
// Subsequences (kLlSubseqBits bits, one per lane, kLlLanes per workgroup) never cross a segment's border.  The pad bits of a segment's
// last byte (fewer than 8, all ones) are no sample: no JPEG table has a code of ones only.
//
// Passes.
//   destuff   ll_destuff_mask per 16 raw bytes: count, then compact; the last chunk publishes the segment's bit count.
//   pass 0    every lane parses from its subsequence's first bit at phase 0 until it leaves the subsequence: end state, sample count
//             (ll_pass0: a guess that dies is followed by the next one).
//   rounds    a lane whose predecessor's end state differs from the state it started from starts again from there: inside the
//             workgroup through LDS until nothing moves (kLlMaxRounds at the most), then across workgroup borders in kLlMaxRipple
//             further launches.  A launch reads the border states the launch before it wrote (two buffers in turn), so what comes out
//             does not depend on the order in which workgroups run, and the twin gives exactly the kernels' answer.
//   write     checks first that every lane started from its predecessor's end state (a segment's first lane: bit 0, phase 0).  Then
//             every start state is proven by induction, and only then does the image count as converged.  The sample counts are
//             summed per segment, and every lane parses once more, from its proven state, and stores its differences.
// A parse that meets bits no code matches, or a sample that runs past the segment's end, ends in kLlInvalid.  From a guess that only
// ends the guess: the successor keeps what it has.  It is an error only when the start was proven, which is what the write pass sees:
// a converged image with an invalid end state, or with a segment whose sample count is not rows x width x ncomp, is flagged.  Flagged
// and unconverged images go to the host stage, which names the status.
//
// Bounds.  A stream word is read through Env::word(k), which answers ones for k >= the segment's word count; a sample is stored only
// when its index is below the segment's expected count, and the segment's rows lie inside the image's planes.
#pragma once
#include <cstdint>

#include "huffman_gpu_core.h"  // HJ_HD

namespace hipjpeg {

constexpr uint32_t kLlSubseqBits = 1024;  // S: 32 words per lane; a whole sample (31 bits) fits in the overshoot
constexpr uint32_t kLlLanes = 256;        // G: subsequences (lanes) per workgroup
constexpr uint32_t kLlMaxRounds = 12;     // correction rounds of a workgroup per launch
constexpr uint32_t kLlMaxRipple = 4;      // launches behind pass 0 that carry corrections across workgroup borders
constexpr uint32_t kLlDestuffLaneBytes = 16;
constexpr uint32_t kLlDestuffChunk = kLlLanes * kLlDestuffLaneBytes;  // raw bytes per workgroup of the destuff kernels

// verdict of an image (one word, or-ed together by the write pass)
constexpr uint32_t kLlUnconverged = 1u;  // a lane did not start from its predecessor's end state
constexpr uint32_t kLlInvalidCode = 2u;  // a proven parse met no code, or the segment's end inside a sample
constexpr uint32_t kLlBadCount = 4u;     // a segment's sample count is not rows x width x ncomp

// lookup table of one Huffman table, 32-bit words: LDS holds up to four of them
constexpr uint32_t kLlLookBits = 8;
constexpr uint32_t kLlTabLook = 0;       // 256 uint16, two per word: (length << 8) | symbol for codes of up to 8 bits, 0 for longer ones
constexpr uint32_t kLlTabMaxcode = 128;  // int32[17]: the largest code of each length, -1 where there is none
constexpr uint32_t kLlTabValoff = 145;   // int32[17]: index of a length's first symbol minus its first code
constexpr uint32_t kLlTabVals = 162;     // the symbols, four per word
constexpr uint32_t kLlTableWords = 256;

constexpr uint32_t kLlInvalid = 0xFFFFFFFFu;

struct LlState {
    uint32_t pos;    // bit position in the segment's destuffed stream; kLlInvalid: the parse failed
    uint32_t phase;  // position inside the pixel of the sample that starts at pos
};
HJ_HD uint64_t ll_pack(const LlState& s) { return (uint64_t)s.pos | ((uint64_t)s.phase << 32); }
HJ_HD LlState ll_unpack(uint64_t v) { return LlState{(uint32_t)v, (uint32_t)(v >> 32)}; }
constexpr uint64_t kLlInvalidPacked = 0xFFFFFFFFull;

// One restart interval (or the whole scan).  32- and 64-bit members only.
struct alignas(16) LlSegment {
    const uint8_t* raw;  // the interval's bytes as they are in the file, at a 16-byte boundary; whole 16-byte pieces are readable
    uint8_t* stream;     // destuffed bytes: room for raw_bytes rounded up to 4
    uint32_t raw_bytes;
    uint32_t image;
    uint32_t first_subseq;  // index of the segment's first subsequence in the batch-wide state arrays
    uint32_t max_subseq;    // subsequences it has room for there: ceil(8 raw_bytes / kLlSubseqBits)
    uint32_t first_chunk;   // index of its first destuff chunk in the batch-wide drop counts
    uint32_t first_unit;    // index of its first workgroup unit
    uint32_t samples;       // rows x width x ncomp of the interval
    uint32_t first_row;     // picture row of its first sample
};
static_assert(sizeof(LlSegment) == 48, "LlSegment: 32- and 64-bit members only, no padding");

struct alignas(16) LlImage {
    uint16_t* plane[4];      // difference plane of the component coded at each position of a pixel
    const uint32_t* specs;   // ntables table specifications of kLlSpecWords words
    uint32_t ncomp;
    uint32_t ntables;  // 1: every position names the same table, else ncomp
    uint32_t width;
    uint32_t pitch;    // samples per row of a difference plane
    uint32_t height;
    uint32_t pad;
};
static_assert(sizeof(LlImage) == 64, "LlImage: 32- and 64-bit members only, no padding");

struct LlUnit {
    uint32_t segment;
    uint32_t first;  // sync / write kernels: first subsequence inside the segment, a multiple of kLlLanes; destuff kernels: chunk index
};

// ---------------------------------------------------------------------------------------------------------------- destuffing
// The bytes to drop among a lane's kLlDestuffLaneBytes: a zero behind an FF.  (A segment holds no marker: the host cut it there.)
// bytes[-1 .. n) must be readable through `byte(i)`; returns the mask of dropped bytes.
template <class Byte>
HJ_HD uint32_t ll_destuff_mask(const Byte& byte, uint32_t first, uint32_t n)
{
    uint32_t mask = 0, prev = first > 0 ? byte(first - 1) : 0u;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t b = byte(first + i);
        if (b == 0u && prev == 0xFFu) mask |= 1u << i;
        prev = b;
    }
    return mask;
}

// ---------------------------------------------------------------------------------------------------------------- lookup tables
// What travels is a table's specification as the DHT segment has it, kLlSpecBytes bytes: the sixteen counts, then the symbols (a table
// of more than kLlSpecSymbols symbols is left to the host stage; a lossless table has 17 at the most unless it repeats itself).
// Every workgroup builds the lookup tables it reads from that, a word per lane: word w of the table of `spec` (byte i through spec(i)).
constexpr uint32_t kLlSpecSymbols = 32;
constexpr uint32_t kLlSpecBytes = 16 + kLlSpecSymbols;
constexpr uint32_t kLlSpecWords = kLlSpecBytes / 4;

template <class Spec>
HJ_HD uint32_t ll_look_entry(const Spec& spec, uint32_t idx)  // idx: the next kLlLookBits bits
{
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= kLlLookBits; l++) {
        const uint32_t n = spec(l - 1), c = idx >> (kLlLookBits - l);
        if (c - code < n) return (l << 8) | spec(16 + ((k + c - code) & (kLlSpecSymbols - 1)));
        k += n;
        code = (code + n) << 1;
    }
    return 0;
}

template <class Spec>
HJ_HD uint32_t ll_table_word(const Spec& spec, uint32_t w)
{
    if (w < kLlTabMaxcode) return ll_look_entry(spec, 2 * w) | (ll_look_entry(spec, 2 * w + 1) << 16);
    if (w < kLlTabVals) {
        const bool want_max = w < kLlTabValoff;
        const uint32_t len = w - (want_max ? kLlTabMaxcode : kLlTabValoff);
        if (len == 0) return 0;
        uint32_t code = 0, k = 0;
        for (uint32_t l = 1; l < len; l++) {
            k += spec(l - 1);
            code = (code + spec(l - 1)) << 1;
        }
        const uint32_t n = spec(len - 1);
        return want_max ? (n ? code + n - 1u : 0xFFFFFFFFu) : k - code;
    }
    const uint32_t i = (w - kLlTabVals) * 4;
    if (i >= kLlSpecSymbols) return 0;
    return spec(16 + i) | (spec(17 + i) << 8) | (spec(18 + i) << 16) | (spec(19 + i) << 24);
}

// ---------------------------------------------------------------------------------------------------------------- the parse
// Env:  uint32_t word(uint32_t k)               word k of the segment's stream, most significant bit first, ones behind its end
//       uint32_t tab(uint32_t t, uint32_t w)    word w of lookup table t
// The window: the 32 bits from a bit position on, from two words held in registers.
template <class Env>
struct LlBits {
    uint32_t idx, w0, w1;
    HJ_HD void start(const Env& env, uint32_t pos)
    {
        idx = pos >> 5;
        w0 = env.word(idx);
        w1 = env.word(idx + 1);
    }
    HJ_HD uint32_t window(const Env& env, uint32_t pos)  // pos >> 5 is idx or idx + 1
    {
        if ((pos >> 5) != idx) {
            idx++;
            w0 = w1;
            w1 = env.word(idx + 1);
        }
        const uint32_t s = pos & 31u;
        return s ? (w0 << s) | (w1 >> (32u - s)) : w0;
    }
};

struct LlNoSink {
    HJ_HD void operator()(uint32_t) const {}
};

// Parses samples from *st while they start in front of `limit` (the subsequence's end or the segment's, whichever comes first;
// total_bits: the segment's).  ncomp: positions of a pixel that the phase runs through; shared: all of them read table 0.  Every
// difference goes to sink(value).  Returns the samples parsed; *st: where the parse left, or kLlInvalid.
template <class Env, class Sink>
HJ_HD uint32_t ll_parse(const Env& env, uint32_t ncomp, bool shared, uint32_t total_bits, uint32_t limit, LlState* st, Sink& sink)
{
    uint32_t pos = st->pos, phase = st->phase, n = 0;
    if (pos >= limit) return 0;
    LlBits<Env> bits;
    bits.start(env, pos);
    while (pos < limit) {
        const uint32_t win = bits.window(env, pos);
        const uint32_t rem = total_bits - pos;  // >= 1
        if (rem < 8u && (win >> (32u - rem)) == (1u << rem) - 1u) {  // the pad bits of the segment's last byte
            pos = total_bits;
            break;
        }
        const uint32_t t = shared ? 0u : phase;
        const uint32_t peek = win >> 16;
        const uint32_t idx = peek >> (16u - kLlLookBits);
        const uint32_t e = (env.tab(t, kLlTabLook + (idx >> 1)) >> (16u * (idx & 1u))) & 0xFFFFu;
        uint32_t len, sym;
        if (e) {
            len = e >> 8;
            sym = e & 255u;
        } else {
            len = kLlLookBits + 1u;
            while (len <= 16u && (int32_t)(peek >> (16u - len)) > (int32_t)env.tab(t, kLlTabMaxcode + len)) len++;
            if (len > 16u) {
                pos = kLlInvalid;
                break;
            }
            const uint32_t at = (env.tab(t, kLlTabValoff + len) + (peek >> (16u - len))) & (kLlSpecSymbols - 1u);
            sym = (env.tab(t, kLlTabVals + (at >> 2)) >> (8u * (at & 3u))) & 255u;
        }
        const uint32_t extra = sym >= 16u ? 0u : sym;  // (a table of this decoder has no symbol above 16)
        if (len + extra > rem) {
            pos = kLlInvalid;
            break;
        }
        uint32_t v;
        if (sym == 0u) {
            v = 0u;
        } else if (sym >= 16u) {
            v = 32768u;
        } else {
            v = (win << len) >> (32u - sym);
            if (v < (1u << (sym - 1u))) v += (0xFFFFFFFFu << sym) + 1u;
        }
        sink(v & 0xFFFFu);
        pos += len + extra;
        n++;
        phase = phase + 1u == ncomp ? 0u : phase + 1u;
    }
    st->pos = pos;
    st->phase = pos == kLlInvalid ? 0u : phase;
    return n;
}

// Pass 0 of subsequence i > 0: the guess is "a sample of phase 0 starts at the subsequence's first bit".  Where that parse meets bits
// no code matches the guess is dead, and the next one is tried: the same bit at the other phases, then the bits behind it, up to
// kLlGuessBits of them -- a sample does start within 31 bits, and under a table that leaves codes unused (the tests' flat table leaves
// 15 of 32) every other guess dies within a few samples, where under a full table it would have drifted onto the true samples instead.
// *start: the guess that lived (the last one tried if none did).  Returns the samples parsed; *end as ll_parse leaves it.
constexpr uint32_t kLlGuessBits = 32;
template <class Env>
HJ_HD uint32_t ll_pass0(const Env& env, uint32_t phases, bool shared, uint32_t total_bits, uint32_t i, uint32_t limit, LlState* start, LlState* end)
{
    LlNoSink none;
    const uint32_t first = i * kLlSubseqBits;
    uint32_t n = 0;
    for (uint32_t k = 0; k < kLlGuessBits && first + k < limit; k++)
        for (uint32_t phase = 0; phase < phases; phase++) {
            *start = LlState{first + k, phase};
            *end = *start;
            n = ll_parse(env, phases, shared, total_bits, limit, end, none);
            if (end->pos != kLlInvalid) return n;
        }
    return n;
}

// The subsequences a segment of total_bits has, and the limit of subsequence i
HJ_HD uint32_t ll_num_subseq(uint32_t total_bits) { return total_bits / kLlSubseqBits + (total_bits % kLlSubseqBits ? 1u : 0u); }
HJ_HD uint32_t ll_limit(uint32_t i, uint32_t total_bits)
{
    // (i + 1) * kLlSubseqBits does not wrap: i < ll_num_subseq(total_bits) <= 2^22
    const uint64_t end = (uint64_t)(i + 1u) * kLlSubseqBits;
    return end < total_bits ? (uint32_t)end : total_bits;
}

// Where the write pass puts sample k of a segment
struct LlCursor {
    uint32_t comp, x, row;
    HJ_HD void start(uint32_t ncomp, uint32_t width, uint32_t first_row, uint32_t k)
    {
        const uint32_t pixel = k / ncomp;
        comp = k - pixel * ncomp;
        row = pixel / width;
        x = pixel - row * width;
        row += first_row;
    }
    HJ_HD void next(uint32_t ncomp, uint32_t width)
    {
        if (++comp == ncomp) {
            comp = 0;
            if (++x == width) {
                x = 0;
                row++;
            }
        }
    }
};

}  // namespace hipjpeg
