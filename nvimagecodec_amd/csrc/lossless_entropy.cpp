// lossless_entropy.cpp -- see lossless_entropy.h
#include "lossless_entropy.h"

#include <cstring>
#include <memory>

namespace hipjpeg {

hipjpegStatus_t lossless_frame(const uint8_t* data, size_t size, LosslessFrame* out)
{
    *out = LosslessFrame();
    FrameInfo f;
    const ParseStatus ps = parse_lossless_jpeg(data, size, &f);
    if (ps != kParseOk)
        return ps == kParseUnsupported ? HIPJPEG_STATUS_UNSUPPORTED : ps == kParseTruncated ? HIPJPEG_STATUS_TRUNCATED : HIPJPEG_STATUS_BAD_JPEG;
    out->width = f.width;
    out->height = f.height;
    out->ncomp = f.ncomp;
    out->precision = f.precision;
    for (int c = 0; c < f.ncomp; c++) out->comp_id[c] = f.comp[c].id;
    // valid files this decoder does not take: subsampled components, one scan per component
    for (int c = 0; c < f.ncomp; c++)
        if (f.comp[c].h != 1 || f.comp[c].v != 1) return HIPJPEG_STATUS_UNSUPPORTED;
    const ScanHeader& sc = f.scans[0];
    if (f.scans.size() != 1 || sc.ncomp != f.ncomp) return HIPJPEG_STATUS_UNSUPPORTED;
    // the scan header of a lossless frame: Ss = predictor 1..7 (0 belongs to hierarchical frames), Se = Ah = 0, Al = point transform
    if (sc.ss < 1 || sc.ss > 7 || sc.se != 0 || sc.ah != 0 || sc.al >= f.precision) return HIPJPEG_STATUS_BAD_JPEG;
    out->ps = sc.ss;
    out->pt = sc.al;
    for (int i = 0; i < sc.ncomp; i++) {
        const HuffSpec& t = sc.dc[sc.td[i]];
        if (!t.present) return HIPJPEG_STATUS_BAD_JPEG;
        int n = 0;
        for (int l = 1; l <= 16; l++) n += t.bits[l];
        for (int k = 0; k < n; k++)
            if (t.vals[k] > 16) return HIPJPEG_STATUS_BAD_JPEG;
        out->scan_comp[i] = sc.comp_index[i];
        out->table[i] = t;
    }
    // a restart interval counts pixels; only whole rows are taken (what libjpeg-turbo takes too)
    if (sc.restart_interval % f.width != 0) return HIPJPEG_STATUS_UNSUPPORTED;
    out->restart_rows = sc.restart_interval / f.width;
    out->data_begin = sc.data_begin;
    out->data_end = sc.data_end;
    return HIPJPEG_STATUS_SUCCESS;
}

namespace {

constexpr int kLookBits = 10;

struct DecodeTable {
    uint16_t look[1 << kLookBits];  // (length << 8) | symbol for codes of up to kLookBits bits, 0 for longer ones
    int32_t maxcode[17], valoff[17];
    uint8_t vals[256];
    void build(const HuffSpec& t)
    {
        memset(look, 0, sizeof look);
        memcpy(vals, t.vals, sizeof vals);
        int code = 0, k = 0;
        for (int l = 1; l <= 16; l++) {
            valoff[l] = k - code;
            for (int i = 0; i < t.bits[l]; i++, k++, code++)
                if (l <= kLookBits) {
                    const int first = code << (kLookBits - l);
                    for (int j = 0; j < (1 << (kLookBits - l)); j++) look[first + j] = (uint16_t)((l << 8) | t.vals[k]);
                }
            maxcode[l] = t.bits[l] ? code - 1 : -1;
            code <<= 1;
        }
    }
};

// Bits of the entropy-coded segment, stuffed zeros removed, most significant first.  `acc` holds the next bits left-aligned; `nbits` of
// them are counted.  (The fast refill also leaves the leading bits of the next, not yet counted byte behind the counted ones: they
// are the true bits of that byte, so or-ing the byte in again later changes nothing.)
struct BitReader {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int nbits = 0;
    bool marker = false;  // the supply stopped at an FF that opens a marker or a fill byte
    inline void refill()  // called with nbits < 32
    {
        if (end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            w = __builtin_bswap64(w);
            const uint64_t v = ~w;
            if (!((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull)) {  // no FF among the eight bytes
                const int k = (64 - nbits) >> 3;
                acc |= w >> nbits;
                p += k;
                nbits += 8 * k;
                return;
            }
        }
        while (nbits <= 56 && p < end) {
            const uint8_t b = *p;
            if (b == 0xFF) {
                if (p + 1 >= end) break;  // a lone FF closes the data
                if (p[1] != 0) {
                    marker = true;
                    break;
                }
                p += 2;
            } else {
                p++;
            }
            acc |= (uint64_t)b << (56 - nbits);
            nbits += 8;
        }
    }
    inline void drop(int n)
    {
        acc <<= n;
        nbits -= n;
    }
};

// one difference; false: the bits ran out or no code matches (*corrupt)
inline bool decode_difference(BitReader& br, const DecodeTable& t, uint16_t* out, bool* corrupt)
{
    if (br.nbits < 32) br.refill();
    const uint32_t peek = (uint32_t)(br.acc >> 48);
    uint32_t e = t.look[peek >> (16 - kLookBits)];
    int len, sym;
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255);
    } else {
        len = kLookBits + 1;
        while (len <= 16 && (int32_t)(peek >> (16 - len)) > t.maxcode[len]) len++;
        if (len > 16) {
            // the zeros behind the last counted bit match no code either: a stream that simply ends is not called corrupt
            *corrupt = br.nbits >= 16 || br.marker;
            return false;
        }
        sym = t.vals[t.valoff[len] + (int32_t)(peek >> (16 - len))];
    }
    const int extra = sym == 16 ? 0 : sym;
    if (len + extra > br.nbits) {
        *corrupt = br.marker;  // a marker where bits should be
        return false;
    }
    br.drop(len);
    if (sym == 0) {
        *out = 0;
    } else if (sym == 16) {
        *out = 32768;
    } else {
        int v = (int)(br.acc >> (64 - sym));
        br.drop(sym);
        if (v < (1 << (sym - 1))) v += (int)((~0u) << sym) + 1;
        *out = (uint16_t)v;
    }
    return true;
}

}  // namespace

hipjpegStatus_t lossless_entropy_decode(const uint8_t* data, const LosslessFrame& f, uint16_t* const planes[4], size_t pitch)
{
    std::unique_ptr<DecodeTable[]> tables(new DecodeTable[(size_t)f.ncomp]);
    for (int i = 0; i < f.ncomp; i++) tables[(size_t)i].build(f.table[i]);
    BitReader br;
    br.p = data + f.data_begin;
    br.end = data + f.data_end;
    const int rows = f.interval_rows();
    int markers = 0;
    for (int row0 = 0; row0 < f.height; row0 += rows) {
        if (row0 > 0) {
            // the interval's last byte is padded out; behind it the marker, RST0 .. RST7 in turn (fill bytes may precede it)
            br.acc = 0;
            br.nbits = 0;
            br.marker = false;
            if (br.p >= br.end) return HIPJPEG_STATUS_TRUNCATED;
            if (*br.p != 0xFF) return HIPJPEG_STATUS_CORRUPT;
            while (br.p < br.end && *br.p == 0xFF) br.p++;
            if (br.p >= br.end) return HIPJPEG_STATUS_TRUNCATED;
            if (*br.p != 0xD0 + (markers & 7)) return HIPJPEG_STATUS_CORRUPT;
            br.p++;
            markers++;
        }
        const int row1 = row0 + rows < f.height ? row0 + rows : f.height;
        bool corrupt = false;
        for (int row = row0; row < row1; row++) {
            if (f.ncomp == 1) {
                uint16_t* d = planes[f.scan_comp[0]] + (size_t)row * pitch;
                const DecodeTable& t = tables[0];
                for (int x = 0; x < f.width; x++)
                    if (!decode_difference(br, t, d + x, &corrupt)) return corrupt ? HIPJPEG_STATUS_CORRUPT : HIPJPEG_STATUS_TRUNCATED;
            } else {
                uint16_t* d[4];
                for (int i = 0; i < f.ncomp; i++) d[i] = planes[f.scan_comp[i]] + (size_t)row * pitch;
                for (int x = 0; x < f.width; x++)
                    for (int i = 0; i < f.ncomp; i++)
                        if (!decode_difference(br, tables[(size_t)i], d[i] + x, &corrupt))
                            return corrupt ? HIPJPEG_STATUS_CORRUPT : HIPJPEG_STATUS_TRUNCATED;
            }
        }
    }
    return HIPJPEG_STATUS_SUCCESS;
}

}  // namespace hipjpeg
