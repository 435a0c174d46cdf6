// lossless_fuzz.cpp -- stand-alone harness for the sanitizer build of the lossless decoder's host side (tests/test_lossless_sanitizers.py):
// the parser's SOF3 path, the entropy stage, the plain reconstruction and the two kernel schedules.
//
//   lossless_fuzz ROUNDS SEED file.jpg...
//
// Every seed file must decode, and the three reconstructions must agree sample for sample.  Then ROUNDS mutated copies (bytes
// overwritten, removed, inserted; files cut short) go through hipjpegGetLosslessInfo and, where that takes them, through all three
// again: whatever the status, they agree with each other, and nothing reads or writes outside its buffers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hipjpeg.h"

namespace {

std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> v;
    if (FILE* f = fopen(path, "rb")) {
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
        fclose(f);
    }
    return v;
}

struct Result {
    hipjpegStatus_t status;
    std::vector<uint8_t> samples;
};

// which: -1 = hipjpegDecodeLosslessHost, 0..2 = hipjpegLosslessReconstructAlgorithmHost(kernel)
Result decode(const std::vector<uint8_t>& file, const hipjpegLosslessInfo_t& info, int which, int sample_bytes, bool planar, uint32_t extra_pitch)
{
    Result r;
    const size_t row = (size_t)info.width * (size_t)sample_bytes * (size_t)(planar ? 1 : info.num_components);
    const size_t pitch = row + extra_pitch, plane = pitch * (size_t)info.height;
    r.samples.assign(plane * (size_t)(planar ? info.num_components : 1), 0xA5);  // exactly as large as the pitches say
    hipjpegLosslessOutput_t o;
    memset(&o, 0, sizeof o);
    o.sample_bytes = sample_bytes;
    o.planar = planar ? 1 : 0;
    for (int c = 0; c < (planar ? info.num_components : 1); c++) {
        o.plane[c] = r.samples.data() + plane * (size_t)c;
        o.pitch[c] = (uint32_t)pitch;
    }
    r.status = which < 0 ? hipjpegDecodeLosslessHost(file.data(), file.size(), &o)
                         : hipjpegLosslessReconstructAlgorithmHost(file.data(), file.size(), &o, which);
    return r;
}

// all the decodes of one file; false = they disagree
bool agree(const std::vector<uint8_t>& file, const hipjpegLosslessInfo_t& info, std::mt19937& rng, bool must_succeed, long* decoded)
{
    const int sample_bytes = info.precision <= 8 && (rng() & 1) ? 1 : 2;
    const bool planar = (rng() & 1) != 0;
    const uint32_t extra = rng() % 5;
    const Result plain = decode(file, info, -1, sample_bytes, planar, extra);
    if (must_succeed && plain.status != HIPJPEG_STATUS_SUCCESS) return false;
    for (int which = 0; which <= 2; which++) {
        if (which == 1 && info.predictor != 1) continue;
        const Result other = decode(file, info, which, sample_bytes, planar, extra);
        if (other.status != plain.status) return false;
        if (plain.status == HIPJPEG_STATUS_SUCCESS && other.samples != plain.samples) return false;
    }
    if (plain.status == HIPJPEG_STATUS_SUCCESS) ++*decoded;
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s ROUNDS SEED file.jpg...\n", argv[0]);
        return 2;
    }
    const long rounds = atol(argv[1]);
    std::mt19937 rng((unsigned)atol(argv[2]));
    std::vector<std::vector<uint8_t>> seeds;
    for (int i = 3; i < argc; i++) {
        seeds.push_back(read_file(argv[i]));
        if (seeds.back().size() < 4) {
            fprintf(stderr, "cannot read %s\n", argv[i]);
            return 2;
        }
    }
    long wrong = 0, decoded = 0, calls = 0, reached = 0;
    for (size_t i = 0; i < seeds.size(); i++) {
        hipjpegLosslessInfo_t info;
        if (hipjpegGetLosslessInfo(seeds[i].data(), seeds[i].size(), &info) != HIPJPEG_STATUS_SUCCESS || !agree(seeds[i], info, rng, true, &decoded)) {
            fprintf(stderr, "seed %s does not decode alike\n", argv[3 + i]);
            wrong++;
        }
        calls++;
    }
    for (long r = 0; r < rounds; r++) {
        std::vector<uint8_t> file = seeds[rng() % seeds.size()];
        const int edits = 1 + (int)(rng() % 5);
        for (int e = 0; e < edits && file.size() > 4; e++) {
            const size_t at = 2 + rng() % (file.size() - 2);
            switch (rng() % 4) {
            case 0: file[at] = (uint8_t)rng(); break;
            case 1: file.erase(file.begin() + (long)at, file.begin() + (long)std::min(file.size(), at + 1 + rng() % 8)); break;
            case 2: file.insert(file.begin() + (long)at, (size_t)(1 + rng() % 4), (uint8_t)rng()); break;
            default: file.resize(at); break;
            }
        }
        calls++;
        hipjpegLosslessInfo_t info;
        if (hipjpegGetLosslessInfo(file.data(), file.size(), &info) != HIPJPEG_STATUS_SUCCESS) continue;
        if ((int64_t)info.width * info.height * info.num_components > (1 << 22)) continue;  // a damaged size field: a huge empty picture teaches nothing
        reached++;
        if (!agree(file, info, rng, false, &decoded)) {
            fprintf(stderr, "round %ld: the decodes disagree\n", r);
            wrong++;
        }
    }
    printf("%ld calls, %ld files decoded, %ld damaged files reached the entropy stage, %ld wrong results\n", calls, decoded, reached, wrong);
    return wrong ? 1 : 0;
}
