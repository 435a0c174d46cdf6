// transcode_crop_fuzz.cpp -- AddressSanitizer / UBSan harness for the crop, drop-chroma and copy-markers steps of the lossless transcode
// on the host: hipjpegTranscodeHostRegion with random regions and flag sets, HIPJPEG_TRANSCODE_COPY_MARKERS among them, so that the
// segment collector and the EXIF patch (jpeg_syntax.cpp) read lengths and offsets an attacker controls.  CPU only, a stand-alone program;
// tests/test_transcode_crop_sanitizers.py builds and runs it.
// usage: transcode_crop_fuzz <iterations> <seed> file.jpg...   -- every file as it is and with metadata segments spliced in behind SOI
// (EXIF in both byte orders, ICC-sized APP2, COM, fill bytes), then mutated copies (bit flips, truncation, header bytes overwritten, TIFF
// fields overwritten).  A file that comes out must parse and decode to the expected size and component count; when it is not turned, the
// blocks it carries must equal the source's at the crop's origin, tables included; with COPY_MARKERS it must not be shorter than without.
// Prints a summary line, exits non-zero only if a sanitizer aborts or such a check fails.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <vector>

#include "entropy_decode.h"
#include "hipjpeg.h"
#include "jpeg_syntax.h"

using namespace hipjpeg;

static long g_calls = 0, g_files = 0, g_refused = 0, g_wrong = 0, g_with_markers = 0;

static bool decode(const std::vector<uint8_t>& bytes, FrameInfo* f, std::vector<int16_t>* coef, int16_t* ptr[4])
{
    if (parse_jpeg(bytes.data(), bytes.size(), f) != kParseOk) return false;
    coef->assign(f->total_blocks() * 64, 0);
    size_t off = 0;
    for (int c = 0; c < 4; c++) ptr[c] = nullptr;
    for (int c = 0; c < f->ncomp; c++) {
        ptr[c] = coef->data() + off;
        off += (size_t)f->comp[c].blocks_w * f->comp[c].blocks_h * 64;
    }
    return decode_coefficients(bytes.data(), bytes.size(), *f, ptr) == kEntropyOk;
}

static bool transcode(const std::vector<uint8_t>& src, const hipjpegTranscodeParams_t& p, const hipjpegTranscodeRegion_t* r, std::vector<uint8_t>* out)
{
    size_t need = 0, length = 0;
    g_calls++;
    hipjpegStatus_t st = hipjpegTranscodeHostRegion(src.data(), src.size(), &p, r, nullptr, 0, &need);
    if (st != HIPJPEG_STATUS_BUFFER_TOO_SMALL) {
        if (st == HIPJPEG_STATUS_SUCCESS) g_wrong++;  // no file fits into no buffer
        g_refused++;
        return false;
    }
    out->assign(need, 0);  // exact size: a write past the end lands in ASan's red zone
    st = hipjpegTranscodeHostRegion(src.data(), src.size(), &p, r, out->data(), out->size(), &length);
    if (st != HIPJPEG_STATUS_SUCCESS || length != need) {
        g_wrong++;
        fprintf(stderr, "second call: status %d, length %zu for %zu\n", (int)st, length, need);
        return false;
    }
    return true;
}

static void run_one(const std::vector<uint8_t>& bytes, std::mt19937& rng)
{
    std::vector<uint8_t> copy(bytes);  // exact-size heap copy: a read one byte past the end lands in ASan's red zone
    FrameInfo fs;
    const bool parses = parse_jpeg(copy.data(), copy.size(), &fs) == kParseOk;
    if (parses && fs.total_blocks() * 128 > (64u << 20)) return;  // forged sizes: keep the campaign quick
    const int w = parses ? fs.width : 64, h = parses ? fs.height : 64;
    for (int round = 0; round < 3; round++) {
        hipjpegTranscodeParams_t p = {(int32_t)(rng() % 2), (int32_t)(rng() % 4 == 0), (int32_t)(rng() % 3 == 0 ? rng() % 5 : 0), 0};
        const bool gray = rng() % 3 == 0, expand = rng() % 2 == 0, markers = rng() % 4 != 0;
        int orientation = rng() % 3 == 0 ? 2 + (int)(rng() % 7) : 0;
        if (orientation) p.orientation |= HIPJPEG_TRANSCODE_TRIM;
        if (rng() % 8 == 0) {
            orientation = -1;  // whatever the EXIF says
            p.orientation |= HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF;
        } else
            p.orientation |= orientation;
        p.orientation |= (gray ? HIPJPEG_TRANSCODE_GRAYSCALE : 0) | (expand ? HIPJPEG_TRANSCODE_CROP_EXPAND : 0) | (markers ? HIPJPEG_TRANSCODE_COPY_MARKERS : 0);
        hipjpegTranscodeRegion_t r = {0, 0, 0, 0};
        const hipjpegTranscodeRegion_t* region = &r;
        switch (rng() % 6) {
        case 0: region = nullptr; break;
        case 1: break;  // all zeros
        case 2: r = {(int32_t)rng(), (int32_t)rng(), (int32_t)rng(), (int32_t)rng()}; break;  // anything at all
        case 3: r = {(int32_t)(rng() % (w + 2)) - 1, (int32_t)(rng() % (h + 2)) - 1, (int32_t)(rng() % (w + 2)), (int32_t)(rng() % (h + 2))}; break;
        default: {  // an origin on a grid of 8, 16 or 32, an end anywhere behind it
            const int step = 8 << (rng() % 3);
            r.x0 = (int32_t)(rng() % (unsigned)(w / step + 1)) * step;
            r.y0 = (int32_t)(rng() % (unsigned)(h / step + 1)) * step;
            r.x1 = r.x0 + 1 + (int32_t)(rng() % (unsigned)std::max(1, w - r.x0));
            r.y1 = r.y0 + 1 + (int32_t)(rng() % (unsigned)std::max(1, h - r.y0));
        }
        }
        std::vector<uint8_t> out;
        if (!transcode(copy, p, region, &out)) continue;
        g_files++;
        FrameInfo fo;
        std::vector<int16_t> cs, co;
        int16_t *ps[4], *po[4];
        if (!decode(copy, &fs, &cs, ps) || !decode(out, &fo, &co, po)) {
            g_wrong++;
            fprintf(stderr, "the transcoded file does not decode\n");
            continue;
        }
        const int ncomp = gray ? 1 : fs.ncomp;
        const int hs = ncomp == 1 ? 1 : fs.comp[0].h, vs = ncomp == 1 ? 1 : fs.comp[0].v;
        int x0 = 0, y0 = 0, x1 = fs.width, y1 = fs.height;
        if (region && (r.x0 | r.y0 | r.x1 | r.y1)) {
            x0 = r.x0 - r.x0 % (8 * hs);
            y0 = r.y0 - r.y0 % (8 * vs);
            x1 = r.x1;
            y1 = r.y1;
            if ((x0 != r.x0 || y0 != r.y0) && !expand) g_wrong++;  // an origin off the grid must have been refused
        }
        if (fo.ncomp != ncomp) g_wrong++;
        if (markers) {
            g_with_markers++;
            hipjpegTranscodeParams_t bare = p;
            bare.orientation &= ~HIPJPEG_TRANSCODE_COPY_MARKERS;
            std::vector<uint8_t> plain;
            if (!transcode(copy, bare, region, &plain) || plain.size() > out.size()) g_wrong++;
            int32_t o = 0;
            if (hipjpegGetExifOrientation(out.data(), out.size(), &o) != HIPJPEG_STATUS_SUCCESS || o < 1 || o > 8) g_wrong++;
        }
        if (orientation != 0) continue;  // turned (or turned by the EXIF's word): size and blocks are the turn tests' business
        if (fo.width != x1 - x0 || fo.height != y1 - y0) {
            g_wrong++;
            fprintf(stderr, "size %d x %d for region %d %d %d %d\n", fo.width, fo.height, x0, y0, x1, y1);
            continue;
        }
        for (int c = 0; c < ncomp; c++) {
            if (memcmp(fs.qtab[c], fo.qtab[c], sizeof fs.qtab[c]) != 0) g_wrong++;
            const int ox = c == 0 ? x0 / 8 : x0 / (8 * hs), oy = c == 0 ? y0 / 8 : y0 / (8 * vs);
            const int rw = (fo.comp[c].samp_w + 7) / 8, rh = (fo.comp[c].samp_h + 7) / 8;
            for (int by = 0; by < rh; by++)
                for (int bx = 0; bx < rw; bx++)
                    if (memcmp(ps[c] + ((size_t)(oy + by) * fs.comp[c].blocks_w + ox + bx) * 64, po[c] + ((size_t)by * fo.comp[c].blocks_w + bx) * 64, 128) != 0) {
                        g_wrong++;
                        fprintf(stderr, "component %d block (%d, %d) is not the source's\n", c, bx, by);
                        by = rh;
                        break;
                    }
        }
    }
}

static void put_segment(std::vector<uint8_t>* o, int marker, const std::vector<uint8_t>& payload)
{
    o->push_back(0xFF);
    o->push_back((uint8_t)marker);
    o->push_back((uint8_t)((payload.size() + 2) >> 8));
    o->push_back((uint8_t)((payload.size() + 2) & 0xFF));
    o->insert(o->end(), payload.begin(), payload.end());
}

// the file with metadata behind SOI: EXIF (one IFD0 entry: orientation), a large APP2, an APP1 that is not EXIF, COM behind fill bytes
static std::vector<uint8_t> with_metadata(const std::vector<uint8_t>& jpeg, std::mt19937& rng)
{
    if (jpeg.size() < 4) return jpeg;
    const bool le = rng() % 2 != 0;
    const uint8_t value = (uint8_t)(rng() % 10);
    std::vector<uint8_t> exif = {'E', 'x', 'i', 'f', 0, 0};
    const uint8_t tiff_le[] = {'I', 'I', 42, 0, 8, 0, 0, 0, 1, 0, 0x12, 0x01, 3, 0, 1, 0, 0, 0, value, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t tiff_be[] = {'M', 'M', 0, 42, 0, 0, 0, 8, 0, 1, 0x01, 0x12, 0, 3, 0, 0, 0, 1, 0, value, 0, 0, 0, 0, 0, 0};
    exif.insert(exif.end(), le ? tiff_le : tiff_be, (le ? tiff_le : tiff_be) + 26);
    std::vector<uint8_t> icc(rng() % 2 ? 65533 : 300, 0x5A), xmp = {'h', 't', 't', 'p', ':', '/', '/'}, com = {'h', 'i', 0xFF, 0xD8};
    std::vector<uint8_t> extra;
    if (rng() % 2) put_segment(&extra, 0xE1, xmp);
    put_segment(&extra, 0xE1, exif);
    put_segment(&extra, 0xE2, icc);
    extra.insert(extra.end(), 2, 0xFF);  // fill bytes in front of the next marker
    put_segment(&extra, 0xFE, com);
    std::vector<uint8_t> out(jpeg.begin(), jpeg.begin() + 2);
    out.insert(out.end(), extra.begin(), extra.end());
    out.insert(out.end(), jpeg.begin() + 2, jpeg.end());
    return out;
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const long iterations = atol(argv[1]);
    std::mt19937 rng((unsigned)atol(argv[2]));
    std::vector<std::vector<uint8_t>> seeds;
    for (int i = 3; i < argc; i++) {
        std::ifstream in(argv[i], std::ios::binary);
        std::vector<uint8_t> plain((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        seeds.push_back(with_metadata(plain, rng));
        run_one(plain, rng);
        run_one(seeds.back(), rng);
    }
    for (long it = 0; it < iterations; it++) {
        std::vector<uint8_t> m = seeds[rng() % seeds.size()];
        if (m.size() < 80) continue;
        switch (rng() % 5) {
        case 0:  // bit flips anywhere
            for (unsigned k = 0, n = 1 + rng() % 4; k < n; k++) m[rng() % m.size()] ^= (uint8_t)(1u << (rng() % 8));
            break;
        case 1:  // truncation
            m.resize(2 + rng() % (m.size() - 2));
            break;
        case 2:  // a byte of the first segments overwritten: markers, segment lengths, the TIFF header, the IFD's count and entries
            m[2 + rng() % 60] = (uint8_t)rng();
            break;
        case 3:  // two of them, one a length byte's worth of 0xFF or 0
            m[2 + rng() % 60] = (uint8_t)(rng() % 2 ? 0xFF : 0);
            m[2 + rng() % 60] = (uint8_t)rng();
            break;
        default:  // a byte anywhere in the headers
            m[2 + rng() % std::min<size_t>(m.size() - 2, 66500)] = (uint8_t)rng();
        }
        run_one(m, rng);
    }
    printf("transcode_crop_fuzz: %ld calls, %ld files written and checked (%ld with markers), %ld refusals, %ld wrong results\n", g_calls, g_files,
           g_with_markers, g_refused, g_wrong);
    return g_wrong ? 1 : 0;
}
