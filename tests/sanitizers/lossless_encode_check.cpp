// lossless_encode_check.cpp -- the host side of the lossless coder under AddressSanitizer + UBSan (tests/test_lossless_encode_sanitizers.py):
// hipjpegEncodeLosslessHost and hipjpegEncodeLosslessGpuAlgorithmHost over the cases the test wrote into a file.  Every plane is copied
// into an allocation of exactly the bytes the input promises (offset + rows * pitch, the last row without its padding), so a load
// beyond a row's width * sample_bytes in the last row, or in front of the first, is an error the sanitizer reports.
//
// File: per case 11 int32 (precision, predictor, point_transform, restart_rows, components, width, height, sample_bytes, planar, pad,
// offset), uint32 length of the expected file, the samples (H x W x N, interleaved, contiguous), the expected file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hipjpeg.h"

static bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0, wrong = 0;
    int32_t h[11];
    while (read_exact(f, h, sizeof h)) {
        uint32_t want_len;
        if (!read_exact(f, &want_len, 4)) return 2;
        const int n = h[4], w = h[5], rows = h[6], sb = h[7], planar = h[8], pad = h[9], offset = h[10];
        std::vector<uint8_t> samples((size_t)rows * w * n * sb), want(want_len);
        if (!read_exact(f, samples.data(), samples.size()) || !read_exact(f, want.data(), want.size())) return 2;
        hipjpegLosslessEncodeParams_t p = {h[0], h[1], h[2], h[3], n};
        hipjpegLosslessEncodeInput_t in;
        memset(&in, 0, sizeof in);
        in.sample_bytes = sb;
        in.planar = planar;
        in.width = w;
        in.height = rows;
        std::vector<uint8_t*> owned;
        const int planes = planar ? n : 1, per_row = planar ? 1 : n;
        for (int c = 0; c < planes; c++) {
            const size_t row_bytes = (size_t)w * per_row * sb, pitch = row_bytes + pad;
            uint8_t* buf = (uint8_t*)malloc(offset + (size_t)(rows - 1) * pitch + row_bytes);
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < w; x++)
                    for (int k = 0; k < per_row; k++)
                        memcpy(buf + offset + y * pitch + ((size_t)x * per_row + k) * sb,
                               samples.data() + (((size_t)y * w + x) * n + (planar ? c : k)) * sb, sb);
            // the padding between rows is readable memory; fill it so that a coder that looks at it changes its output
            for (int y = 0; y + 1 < rows; y++) memset(buf + offset + y * pitch + row_bytes, 0xA5, pad);
            memset(buf, 0xA5, offset);
            in.plane[c] = buf + offset;
            in.pitch[c] = (uint32_t)pitch;
            owned.push_back(buf);
        }
        for (int twin = 0; twin < 2; twin++) {
            std::vector<uint8_t> out(want_len);
            size_t len = 0;
            const hipjpegStatus_t st = twin ? hipjpegEncodeLosslessGpuAlgorithmHost(&in, &p, out.data(), out.size(), &len)
                                            : hipjpegEncodeLosslessHost(&in, &p, out.data(), out.size(), &len);
            if (st != HIPJPEG_STATUS_SUCCESS || len != want_len || memcmp(out.data(), want.data(), len) != 0) {
                printf("case %d (%s): status %d, %zu bytes, expected %u\n", cases, twin ? "twin" : "host", (int)st, len, want_len);
                wrong++;
            }
            // one byte short: the length is named and nothing is written beyond the capacity
            if (want_len > 0) {
                std::vector<uint8_t> small(want_len - 1);
                if ((twin ? hipjpegEncodeLosslessGpuAlgorithmHost(&in, &p, small.data(), small.size(), &len)
                          : hipjpegEncodeLosslessHost(&in, &p, small.data(), small.size(), &len)) != HIPJPEG_STATUS_BUFFER_TOO_SMALL || len != want_len)
                    wrong++;
            }
        }
        for (uint8_t* b : owned) free(b);
        cases++;
    }
    fclose(f);
    printf("%d cases, %d wrong results\n", cases, wrong);
    return wrong ? 1 : 0;
}
