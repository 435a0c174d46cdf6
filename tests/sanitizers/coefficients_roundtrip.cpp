// coefficients_roundtrip.cpp -- AddressSanitizer / UBSan harness for the coefficient-tensor host routes: hipjpegGetCoefficientInfo,
// hipjpegDecodeCoefficientsHost and hipjpegEncodeCoefficientsHost.  CPU only, a stand-alone program; tests/test_coefficients_host.py builds
// and runs it.
// usage: coefficients_roundtrip file.jpg...   -- every file is read into planes of exactly the size its info asks for (16-byte aligned heap
// blocks: a write or read one byte past the end lands in ASan's red zone), once tight and once with a padded pitch whose padding must keep
// its fill; what was read is written with every coding target and must equal hipjpegTranscodeHost's file byte for byte, or be refused
// with the status hipjpegTranscodeHost gives that source.  A file that does not decode must leave the planes untouched.
// Prints a summary line, exits non-zero only if a sanitizer aborts or such a check fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "hipjpeg.h"

static long g_files = 0, g_written = 0, g_refused = 0, g_wrong = 0;
static const int16_t kFill = 0x5A5A;

struct Planes {
    hipjpegCoefficientPlanes_t p;
    size_t values[4];
    Planes(const hipjpegCoefficientInfo_t& info, int extra)
    {
        memset(&p, 0, sizeof p);
        for (int c = 0; c < 4; c++) values[c] = 0;
        for (int c = 0; c < info.num_components; c++) {
            p.pitch_blocks[c] = (uint32_t)(info.blocks_w[c] + extra);
            values[c] = (size_t)p.pitch_blocks[c] * (size_t)info.blocks_h[c] * 64;
            int16_t* m = static_cast<int16_t*>(aligned_alloc(16, values[c] * 2));  // (a multiple of 128 bytes)
            if (!m) abort();
            for (size_t k = 0; k < values[c]; k++) m[k] = kFill;
            p.coef[c] = m;
        }
    }
    ~Planes()
    {
        for (int c = 0; c < 4; c++) free(p.coef[c]);
    }
    const int16_t* block(int c, int by, int bx) const { return static_cast<const int16_t*>(p.coef[c]) + ((size_t)by * p.pitch_blocks[c] + bx) * 64; }
    bool untouched() const
    {
        for (int c = 0; c < 4; c++)
            for (size_t k = 0; k < values[c]; k++)
                if (static_cast<const int16_t*>(p.coef[c])[k] != kFill) return false;
        return true;
    }
};

static void wrong(const char* what, const char* file)
{
    g_wrong++;
    fprintf(stderr, "%s: %s\n", file, what);
}

static hipjpegStatus_t transcode(const std::vector<uint8_t>& src, const hipjpegTranscodeParams_t& p, std::vector<uint8_t>* out)
{
    size_t need = 0, length = 0;
    hipjpegStatus_t st = hipjpegTranscodeHost(src.data(), src.size(), &p, nullptr, 0, &need);
    if (st != HIPJPEG_STATUS_BUFFER_TOO_SMALL) return st;
    out->assign(need, 0);
    return hipjpegTranscodeHost(src.data(), src.size(), &p, out->data(), out->size(), &length);
}

static void run_one(const std::vector<uint8_t>& bytes, const char* file)
{
    std::vector<uint8_t> copy(bytes);  // exact-size heap copy: a read one byte past the end lands in ASan's red zone
    g_files++;
    const hipjpegTranscodeParams_t plain = {0, 0, 0, 0};
    std::vector<uint8_t> reference;
    const hipjpegStatus_t transcodable = transcode(copy, plain, &reference);
    hipjpegCoefficientInfo_t info;
    hipjpegStatus_t st = hipjpegGetCoefficientInfo(copy.data(), copy.size(), &info);
    if (st != HIPJPEG_STATUS_SUCCESS) {
        if (st != transcodable) wrong("the header is refused with another status than the transcode's", file);
        g_refused++;
        return;
    }
    Planes tight(info, 0), padded(info, 3);
    st = hipjpegDecodeCoefficientsHost(copy.data(), copy.size(), &tight.p);
    if (hipjpegDecodeCoefficientsHost(copy.data(), copy.size(), &padded.p) != st) wrong("the pitch changes the status", file);
    if (st != HIPJPEG_STATUS_SUCCESS) {
        if (st != transcodable) wrong("the stream is refused with another status than the transcode's", file);
        if (!tight.untouched() || !padded.untouched()) wrong("a failing image wrote into its planes", file);
        g_refused++;
        return;
    }
    for (int c = 0; c < info.num_components; c++)
        for (int by = 0; by < info.blocks_h[c]; by++) {
            for (int bx = 0; bx < info.blocks_w[c]; bx++)
                if (memcmp(tight.block(c, by, bx), padded.block(c, by, bx), 128) != 0) wrong("tight and padded planes differ", file);
            for (int bx = info.blocks_w[c]; bx < (int)padded.p.pitch_blocks[c]; bx++)
                for (int k = 0; k < 64; k++)
                    if (padded.block(c, by, bx)[k] != kFill) wrong("the padding was written", file);
        }
    bool any = false;
    for (int target = 0; target < 4; target++) {
        const hipjpegTranscodeParams_t p = {target == 1, target == 2, target == 3 ? 3 : 0, 0};
        std::vector<uint8_t> want;
        const hipjpegStatus_t expect = transcode(copy, p, &want);
        for (const Planes* planes : {&tight, &padded}) {
            size_t need = 0, length = 0;
            st = hipjpegEncodeCoefficientsHost(&info, &planes->p, &p, nullptr, 0, &need);
            if (expect != HIPJPEG_STATUS_SUCCESS) {
                if (st != expect) wrong("a picture the transcode refuses is refused with another status", file);
                continue;
            }
            if (st != HIPJPEG_STATUS_BUFFER_TOO_SMALL || need != want.size()) {
                wrong("the needed size is not the transcode's", file);
                continue;
            }
            std::vector<uint8_t> out(need, 0);  // exact size: a write past the end lands in ASan's red zone
            st = hipjpegEncodeCoefficientsHost(&info, &planes->p, &p, out.data(), out.size(), &length);
            if (st != HIPJPEG_STATUS_SUCCESS || length != need || out != want) wrong("the file is not the transcode's", file);
            any = true;
        }
    }
    if (any)
        g_written++;
    else
        g_refused++;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (bytes.empty()) {
            wrong("cannot read", argv[i]);
            continue;
        }
        run_one(bytes, argv[i]);
    }
    printf("%ld files, %ld written, %ld refused, %ld wrong results\n", g_files, g_written, g_refused, g_wrong);
    return g_wrong == 0 ? 0 : 1;
}
