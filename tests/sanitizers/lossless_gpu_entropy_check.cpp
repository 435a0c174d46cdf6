// lossless_gpu_entropy_check.cpp -- stand-alone driver for tests/test_lossless_gpu_entropy_sanitizers.py: every file named on the
// command line goes through hipjpegLosslessEntropyAlgorithmHost (the GPU entropy stage's schedule on the CPU) and through
// hipjpegLosslessEntropyHost (the host stage), into planes that end exactly behind the last sample, so that AddressSanitizer sees a
// store one sample too far.  The two must agree on status and planes.  Built with -fsanitize=address,undefined; no GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "hipjpeg.h"

int main(int argc, char** argv)
{
    int wrong = 0, decoded = 0, refused = 0, unconverged = 0;
    for (int a = 1; a < argc; a++) {
        std::ifstream in(argv[a], std::ios::binary);
        std::vector<uint8_t> whole((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        // an exact-size copy: a read behind the file's last byte is a finding too
        std::unique_ptr<uint8_t[]> data(new uint8_t[whole.size() ? whole.size() : 1]);
        if (!whole.empty()) memcpy(data.get(), whole.data(), whole.size());
        hipjpegLosslessInfo_t info;
        if (hipjpegGetLosslessInfo(data.get(), whole.size(), &info) != HIPJPEG_STATUS_SUCCESS) {
            refused++;
            continue;
        }
        const size_t pitch = (size_t)info.width, samples = pitch * (size_t)info.height;
        std::unique_ptr<uint16_t[]> twin[4], host[4];
        uint16_t *tp[4] = {nullptr, nullptr, nullptr, nullptr}, *hp[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int c = 0; c < info.num_components; c++) {
            twin[c].reset(new uint16_t[samples]());
            host[c].reset(new uint16_t[samples]());
            tp[c] = twin[c].get();
            hp[c] = host[c].get();
        }
        int32_t converged = -1;
        const hipjpegStatus_t st = hipjpegLosslessEntropyAlgorithmHost(data.get(), whole.size(), tp, pitch, &converged);
        const hipjpegStatus_t sh = hipjpegLosslessEntropyHost(data.get(), whole.size(), hp, pitch);
        if (converged == 0) unconverged++;
        if (st != sh || converged < 0) {
            printf("%s: status %d, host stage %d\n", argv[a], (int)st, (int)sh);
            wrong++;
            continue;
        }
        if (st != HIPJPEG_STATUS_SUCCESS) {
            refused++;
            continue;
        }
        decoded++;
        for (int c = 0; c < info.num_components; c++)
            if (memcmp(tp[c], hp[c], samples * sizeof(uint16_t)) != 0) {
                printf("%s: component %d differs\n", argv[a], c);
                wrong++;
                break;
            }
    }
    printf("%d files, %d decoded, %d refused, %d unconverged, %d wrong results\n", argc - 1, decoded, refused, unconverged, wrong);
    return wrong ? 1 : 0;
}
