// transcode_fuzz.cpp -- AddressSanitizer / UBSan harness for the host side of the lossless transcode: hipjpegTranscodeHost (the
// eligibility rules, the relayout from the decoder's blocks to the coder's, the range guard) with the host entropy decoder in front of
// it and the host coder behind it, on the CPU only.  tests/test_transcode_sanitizers.py builds and runs it.
// usage: transcode_fuzz <iterations> <seed> file.jpg...   -- every file as it is, then mutated copies (bit flips, truncation, header
// bytes overwritten, a marker spliced into the scan); every target for each.  A file that comes out must parse, decode, and hold the
// coefficients and tables of its source; prints a summary line, exits non-zero only if a sanitizer aborts or such a check fails.
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

static long g_calls = 0, g_files = 0, g_unsupported = 0, g_wrong = 0;

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

static void run_one(const std::vector<uint8_t>& bytes)
{
    // exact-size heap copy: a read one byte past the end lands in ASan's red zone
    std::vector<uint8_t> copy(bytes);
    {
        FrameInfo probe;  // forged sizes: the device route has its own cap (max_image_samples), this harness keeps the campaign quick
        if (parse_jpeg(copy.data(), copy.size(), &probe) == kParseOk && probe.total_blocks() * 128 > (64u << 20)) return;
    }
    static const hipjpegTranscodeParams_t targets[4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 3, 0}};
    for (const hipjpegTranscodeParams_t& t : targets) {
        size_t need = 0;
        g_calls++;
        hipjpegStatus_t st = hipjpegTranscodeHost(copy.data(), copy.size(), &t, nullptr, 0, &need);
        if (st == HIPJPEG_STATUS_UNSUPPORTED) g_unsupported++;
        if (st != HIPJPEG_STATUS_BUFFER_TOO_SMALL) {
            if (st == HIPJPEG_STATUS_SUCCESS) g_wrong++;  // no file fits into no buffer
            return;                                       // refused: the other targets are refused alike
        }
        std::vector<uint8_t> out(need);  // exact size again
        size_t length = 0;
        st = hipjpegTranscodeHost(copy.data(), copy.size(), &t, out.data(), out.size(), &length);
        if (st != HIPJPEG_STATUS_SUCCESS || length != need) {
            g_wrong++;
            fprintf(stderr, "second call: status %d, length %zu for %zu\n", (int)st, length, need);
            return;
        }
        g_files++;
        FrameInfo fs, fo;
        std::vector<int16_t> cs, co;
        int16_t *ps[4], *po[4];
        if (!decode(copy, &fs, &cs, ps) || !decode(out, &fo, &co, po) || fs.ncomp != fo.ncomp || fo.width != fs.width || fo.height != fs.height) {
            g_wrong++;
            fprintf(stderr, "the transcoded file does not decode like its source\n");
            return;
        }
        for (int c = 0; c < fs.ncomp; c++) {
            if (memcmp(fs.qtab[c], fo.qtab[c], sizeof fs.qtab[c]) != 0) g_wrong++;
            const int rw = (fs.comp[c].samp_w + 7) / 8, rh = (fs.comp[c].samp_h + 7) / 8;
            for (int by = 0; by < rh; by++)
                for (int bx = 0; bx < rw; bx++)
                    if (memcmp(ps[c] + ((size_t)by * fs.comp[c].blocks_w + bx) * 64, po[c] + ((size_t)by * fo.comp[c].blocks_w + bx) * 64, 128) != 0) {
                        g_wrong++;
                        fprintf(stderr, "component %d block (%d, %d) changed\n", c, bx, by);
                        return;
                    }
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const long iterations = atol(argv[1]);
    std::mt19937 rng((unsigned)atol(argv[2]));
    std::vector<std::vector<uint8_t>> seeds;
    for (int i = 3; i < argc; i++) {
        std::ifstream in(argv[i], std::ios::binary);
        seeds.emplace_back(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        run_one(seeds.back());
    }
    for (long it = 0; it < iterations; it++) {
        std::vector<uint8_t> m = seeds[rng() % seeds.size()];
        if (m.size() < 8) continue;
        switch (rng() % 5) {
        case 0:  // bit flips anywhere
            for (unsigned k = 0, n = 1 + rng() % 4; k < n; k++) m[rng() % m.size()] ^= (uint8_t)(1u << (rng() % 8));
            break;
        case 1:  // truncation
            m.resize(2 + rng() % (m.size() - 2));
            break;
        case 2:  // byte overwrite inside the headers: sampling factors, table entries, component ids
            m[2 + rng() % std::min<size_t>(m.size() - 2, 700)] = (uint8_t)rng();
            break;
        case 3:  // a marker spliced into the entropy-coded data
            if (m.size() > 700) {
                const size_t p = 650 + rng() % (m.size() - 652);
                m[p] = 0xFF;
                m[p + 1] = (uint8_t)(0xC0 + rng() % 0x3F);
            }
            break;
        default:  // bytes of the scan overwritten: other symbols, other magnitudes (what the range guard is for)
            for (unsigned k = 0, n = 1 + rng() % 8; k < n && m.size() > 700; k++) m[650 + rng() % (m.size() - 650)] = (uint8_t)rng();
        }
        run_one(m);
    }
    printf("transcode_fuzz: %ld calls, %ld files written and checked, %ld refusals as unsupported, %ld wrong results\n", g_calls, g_files, g_unsupported, g_wrong);
    return g_wrong ? 1 : 0;
}
