// coefficient_pixels_host.cpp -- AddressSanitizer / UBSan harness for the host rules of the coefficient <-> pixel calls:
// hipjpegGetEncodeCoefficientInfo and coefficient_frame() (coefficients_core.h: the frame an `info` describes, as
// hipjpegCoefficientsToPixelsBatch plans it).  CPU only, a stand-alone program; tests/test_coefficient_pixels_sanitizers.py builds and
// runs it.
// usage: coefficient_pixels_host file.jpg...
//   1. every size of a sweep x every subsampling value -1..8 x qualities 1, 50, 90, 100: the info (an exact-size heap object) of the
//      file the encoder would write; the frame built from it must give the same info back (coefficient_info is the inverse);
//   2. every file: the frame built from hipjpegGetCoefficientInfo's info equals the parser's frame in everything the decoder plans by
//      (one and three components), or is refused as UNSUPPORTED (four components);
//   3. every file's info with one field bent at a time: refused, and the output frame is left alone.
// Prints a summary line, exits non-zero only if a sanitizer aborts or such a check fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "coefficients_core.h"

using namespace hipjpeg;

static long g_infos = 0, g_frames = 0, g_refused = 0, g_wrong = 0;

static void wrong(const char* what, const char* where)
{
    g_wrong++;
    fprintf(stderr, "%s: %s\n", where, what);
}

// planes nobody dereferences here: aligned, with the tight pitch
static hipjpegCoefficientPlanes_t planes_for(const hipjpegCoefficientInfo_t& info, void* memory)
{
    hipjpegCoefficientPlanes_t p;
    memset(&p, 0, sizeof p);
    for (int c = 0; c < info.num_components && c < 4; c++) {
        p.coef[c] = memory;
        p.pitch_blocks[c] = (uint32_t)info.blocks_w[c];
    }
    return p;
}

static void sweep(void* memory)
{
    const int sizes[][2] = {{1, 1}, {7, 9}, {8, 8}, {17, 13}, {50, 37}, {2056, 8}, {65535, 1}, {1, 65535}, {65535, 65535}, {0, 4}, {4, 0}, {65536, 4}, {-3, 4}};
    const int qualities[] = {1, 50, 90, 100, 0, 101, -7};
    for (const auto& size : sizes)
        for (int sub = -1; sub <= 8; sub++)
            for (int q : qualities) {
                std::unique_ptr<hipjpegCoefficientInfo_t> info(new hipjpegCoefficientInfo_t);
                const hipjpegEncodeParams_t p = {q, sub, HIPJPEG_OUTPUT_RGBI, 0, 0, 0};
                const hipjpegStatus_t st = hipjpegGetEncodeCoefficientInfo(size[0], size[1], &p, info.get());
                g_infos++;
                const bool known = sub >= 0 && sub <= 6, legal = size[0] >= 1 && size[1] >= 1 && size[0] <= 65535 && size[1] <= 65535;
                const hipjpegStatus_t expect = !known ? HIPJPEG_STATUS_UNSUPPORTED : !legal ? HIPJPEG_STATUS_INVALID_ARGUMENT : HIPJPEG_STATUS_SUCCESS;
                if (st != expect) wrong("unexpected status", "sweep");
                if (st != HIPJPEG_STATUS_SUCCESS) {
                    g_refused++;
                    continue;
                }
                FrameInfo f;
                if (coefficient_frame(*info, planes_for(*info, memory), &f) != HIPJPEG_STATUS_SUCCESS) {
                    wrong("the encoder's own info is refused", "sweep");
                    continue;
                }
                g_frames++;
                hipjpegCoefficientInfo_t back;
                coefficient_info(f, &back);
                if (memcmp(&back, info.get(), sizeof back) != 0) wrong("frame -> info is not the info", "sweep");
            }
    if (hipjpegGetEncodeCoefficientInfo(8, 8, nullptr, nullptr) != HIPJPEG_STATUS_INVALID_ARGUMENT) wrong("null arguments", "sweep");
}

static bool same_frame(const FrameInfo& a, const FrameInfo& b)
{
    if (a.width != b.width || a.height != b.height || a.ncomp != b.ncomp || a.hmax != b.hmax || a.vmax != b.vmax || a.mcus_x != b.mcus_x ||
        a.mcus_y != b.mcus_y || a.color != b.color || a.precision != b.precision)
        return false;
    for (int c = 0; c < a.ncomp; c++) {
        const Component &x = a.comp[c], &y = b.comp[c];
        if (x.h != y.h || x.v != y.v || x.blocks_w != y.blocks_w || x.blocks_h != y.blocks_h || x.samp_w != y.samp_w || x.samp_h != y.samp_h) return false;
        if (memcmp(a.qtab[c], b.qtab[c], sizeof a.qtab[c]) != 0) return false;
    }
    return true;
}

static void run_one(const std::vector<uint8_t>& bytes, const char* file, void* memory)
{
    std::vector<uint8_t> copy(bytes);
    hipjpegCoefficientInfo_t info;
    if (hipjpegGetCoefficientInfo(copy.data(), copy.size(), &info) != HIPJPEG_STATUS_SUCCESS) {
        g_refused++;
        return;
    }
    FrameInfo parsed, built;
    if (parse_jpeg(copy.data(), copy.size(), &parsed) != kParseOk) return wrong("the parser refuses what hipjpegGetCoefficientInfo read", file);
    const hipjpegStatus_t st = coefficient_frame(info, planes_for(info, memory), &built);
    if (info.num_components == 4) {
        if (st != HIPJPEG_STATUS_UNSUPPORTED) wrong("four components must be UNSUPPORTED", file);
        g_refused++;
        return;
    }
    if (st != HIPJPEG_STATUS_SUCCESS) return wrong("a decodable frame's info is refused", file);
    if (!same_frame(parsed, built)) wrong("the frame built from the info is not the parser's", file);
    g_frames++;
    // one field bent at a time
    for (int bend = 0; bend < 12; bend++) {
        hipjpegCoefficientInfo_t bad = info;
        hipjpegCoefficientPlanes_t planes = planes_for(info, memory);
        hipjpegStatus_t expect = HIPJPEG_STATUS_INVALID_ARGUMENT;
        const int last = info.num_components - 1;
        switch (bend) {
        case 0: bad.width = 0; break;
        case 1: bad.height = 65536; break;
        case 2: bad.num_components = 0; break;
        case 3: bad.num_components = 5; break;
        case 4: bad.h[last] = 5; break;
        case 5: bad.v[0] = 0; break;
        case 6: bad.blocks_w[last] += 1; break;
        case 7: bad.blocks_h[0] -= 1; break;
        case 8: planes.coef[last] = nullptr; break;
        case 9: planes.coef[0] = static_cast<char*>(memory) + 2; break;
        case 10: planes.pitch_blocks[last] -= 1; break;
        default:
            if (info.num_components != 3) continue;
            bad.color_model = 3;
            expect = HIPJPEG_STATUS_UNSUPPORTED;
        }
        FrameInfo out;
        out.width = -77;
        if (coefficient_frame(bad, planes, &out) != expect) wrong("a bent info is not refused as it should be", file);
        if (out.width != -77) wrong("a refused info wrote the frame", file);
        g_refused++;
    }
}

int main(int argc, char** argv)
{
    void* memory = aligned_alloc(16, 128);
    if (!memory) abort();
    sweep(memory);
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (bytes.empty()) {
            wrong("cannot read", argv[i]);
            continue;
        }
        run_one(bytes, argv[i], memory);
    }
    free(memory);
    printf("%ld infos, %ld frames, %ld refused, %ld wrong results\n", g_infos, g_frames, g_refused, g_wrong);
    return g_wrong == 0 ? 0 : 1;
}
