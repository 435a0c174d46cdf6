// lossless_core.cpp -- the lossless decoder's host side: what an output must look like, the plane descriptors, the plain
// reconstruction, the kernels' schedule run lane by lane on the host, and the C entry points that need no GPU.
// (These live here, not in hipjpeg_api.cpp, so that they link without the HIP runtime: tests, sanitizer programs.)
#include "lossless_host.h"

#include <cstring>
#include <new>
#include <vector>

namespace hipjpeg {

hipjpegStatus_t lossless_output_ok(const LosslessFrame& f, const hipjpegLosslessOutput_t& o)
{
    if (o.sample_bytes != 1 && o.sample_bytes != 2) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (o.sample_bytes == 1 && f.precision > 8) return HIPJPEG_STATUS_UNSUPPORTED;
    const uint64_t row_bytes = (uint64_t)f.width * (uint64_t)o.sample_bytes * (uint64_t)(o.planar ? 1 : f.ncomp);
    for (int c = 0; c < (o.planar ? f.ncomp : 1); c++)
        if (!o.plane[c] || o.pitch[c] < row_bytes) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return HIPJPEG_STATUS_SUCCESS;
}

void lossless_planes(const LosslessFrame& f, const hipjpegLosslessOutput_t& o, const uint64_t diff[4], const uint64_t scratch[4], LosslessPlane out[4])
{
    for (int c = 0; c < f.ncomp; c++) {
        LosslessPlane& p = out[c];
        memset(&p, 0, sizeof p);
        p.diff = diff[c];
        p.scratch = scratch[c];
        p.width = (uint32_t)f.width;
        p.height = (uint32_t)f.height;
        p.diff_pitch = lossless_diff_pitch((uint32_t)f.width);
        p.out_bytes = (uint32_t)o.sample_bytes;
        if (o.planar) {
            p.out = (uint64_t)reinterpret_cast<uintptr_t>(o.plane[c]);
            p.out_pitch = o.pitch[c];
            p.out_step = p.out_bytes;
        } else {
            p.out = (uint64_t)reinterpret_cast<uintptr_t>(o.plane[0]) + (uint64_t)c * p.out_bytes;
            p.out_pitch = o.pitch[0];
            p.out_step = p.out_bytes * (uint32_t)f.ncomp;
        }
        p.ps = (uint32_t)f.ps;
        p.pt = (uint32_t)f.pt;
        p.init = (uint32_t)f.init();
        p.restart_rows = (uint32_t)f.interval_rows();
    }
}

namespace {

inline void put_sample(uint64_t addr, uint32_t v, uint32_t out_bytes)
{
    uint8_t* q = reinterpret_cast<uint8_t*>((uintptr_t)addr);
    q[0] = (uint8_t)v;
    if (out_bytes == 2) q[1] = (uint8_t)(v >> 8);
}

inline const uint16_t* diff_row(const LosslessPlane& p, uint32_t row) { return reinterpret_cast<const uint16_t*>((uintptr_t)p.diff) + (size_t)row * p.diff_pitch; }

// the shuffle ladder of wave_inclusive_sum (lossless_kernels.hip)
void wave_inclusive_sum(uint32_t v[64])
{
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t n[64];
        for (int l = 0; l < 64; l++) n[l] = v[l >= d ? l - d : l];
        for (int l = d; l < 64; l++) v[l] += n[l];
    }
}

}  // namespace

void lossless_reconstruct_plain(const LosslessPlane& p)
{
    std::vector<uint16_t> above(p.width, 0), line(p.width, 0);
    for (uint32_t row = 0; row < p.height; row++) {
        const uint16_t* d = diff_row(p, row);
        const bool first_row = row % p.restart_rows == 0;
        for (uint32_t col = 0; col < p.width; col++) {
            const int a = col ? line[col - 1] : 0, b = above[col], c = col ? above[col - 1] : 0;
            line[col] = (uint16_t)lossless_state(lossless_predict_at((int)p.ps, first_row, col, (int)p.init, a, b, c), d[col]);
            put_sample(p.out + (uint64_t)row * p.out_pitch + (uint64_t)col * p.out_step, lossless_sample(line[col], p.pt, p.out_bytes), p.out_bytes);
        }
        above.swap(line);
    }
}

// lossless_col0_kernel + lossless_rows_kernel, lane by lane
void lossless_rows_schedule(const LosslessPlane& p)
{
    std::vector<uint16_t> sums(p.height);
    uint32_t carry0 = 0;
    for (uint32_t row0 = 0; row0 < p.height; row0 += 64) {
        uint32_t v[64];
        for (uint32_t lane = 0; lane < 64; lane++) v[lane] = row0 + lane < p.height ? diff_row(p, row0 + lane)[0] : 0u;
        wave_inclusive_sum(v);
        for (uint32_t lane = 0; lane < 64; lane++) {
            v[lane] = (v[lane] + carry0) & 0xFFFFu;
            if (row0 + lane < p.height) sums[row0 + lane] = (uint16_t)v[lane];
        }
        carry0 = v[63];
    }
    constexpr int kWaves = kLosslessRowThreads / 64;
    for (uint32_t row = 0; row < p.height; row++) {
        const uint32_t first = row - row % p.restart_rows;
        uint32_t carry = lossless_row_base(p.init, sums[row], first ? sums[first - 1] : 0u);
        const uint16_t* d = diff_row(p, row);
        for (uint32_t chunk0 = 0; chunk0 < p.width; chunk0 += kLosslessChunkSamples) {
            uint32_t v[kLosslessRowThreads][kLosslessLaneSamples], inclusive[kLosslessRowThreads], wave_total[kWaves];
            for (int t = 0; t < kLosslessRowThreads; t++) {
                const uint32_t col = chunk0 + (uint32_t)t * kLosslessLaneSamples;
                for (int i = 0; i < kLosslessLaneSamples; i++) {
                    v[t][i] = (col + i < p.width && col + i != 0) ? d[col + i] : 0u;
                    if (i) v[t][i] += v[t][i - 1];
                }
                inclusive[t] = v[t][kLosslessLaneSamples - 1];
            }
            for (int w = 0; w < kWaves; w++) {
                wave_inclusive_sum(inclusive + 64 * w);
                wave_total[w] = inclusive[64 * w + 63];
            }
            uint32_t all = 0;
            for (int w = 0; w < kWaves; w++) all += wave_total[w];
            for (int t = 0; t < kLosslessRowThreads; t++) {
                uint32_t before = 0;
                for (int w = 0; w < t / 64; w++) before += wave_total[w];
                const uint32_t offset = carry + before + inclusive[t] - v[t][kLosslessLaneSamples - 1];
                const uint32_t col = chunk0 + (uint32_t)t * kLosslessLaneSamples;
                for (int i = 0; i < kLosslessLaneSamples; i++)
                    if (col + i < p.width)
                        put_sample(p.out + (uint64_t)row * p.out_pitch + (uint64_t)(col + i) * p.out_step,
                                   lossless_sample((offset + v[t][i]) & 0xFFFFu, p.pt, p.out_bytes), p.out_bytes);
            }
            carry = (carry + all) & 0xFFFFu;
        }
    }
}

// lossless_wavefront_kernel, lane by lane: bands, the skew of one column per row, two tile slots, the row carried in scratch
void lossless_wavefront_schedule(const LosslessPlane& p)
{
    constexpr int B = kLosslessBandRows, T = kLosslessTileCols;
    std::vector<uint16_t> tile(2 * (B + 1) * T, 0);
    auto at = [&](uint32_t slot, uint32_t r, uint32_t col) -> uint16_t& { return tile[(slot * (B + 1) + r) * T + col]; };
    std::vector<uint16_t> above(p.diff_pitch, 0);
    const uint32_t ntiles = (p.width + T - 1) / T;
    for (uint32_t band0 = 0; band0 < p.height; band0 += B) {
        const bool carries = band0 + B < p.height;
        int a[B] = {0}, b[B] = {0}, c[B] = {0};
        for (uint32_t g = 0; g <= ntiles + 1; g++) {
            if (g >= 2) {
                const uint32_t slot = g & 1, rows = p.height - band0 < (uint32_t)B ? p.height - band0 : (uint32_t)B;
                for (uint32_t lane = 0; lane < (uint32_t)T; lane++) {
                    const uint32_t col = (g - 2) * T + lane;
                    if (col >= p.width) continue;
                    for (uint32_t r = 0; r < rows; r++)
                        put_sample(p.out + (uint64_t)(band0 + r) * p.out_pitch + (uint64_t)col * p.out_step,
                                   lossless_sample(at(slot, r + 1, lane), p.pt, p.out_bytes), p.out_bytes);
                    if (carries) above[col] = at(slot, B, lane);
                }
            }
            if (g < ntiles) {
                const uint32_t slot = g & 1;
                for (uint32_t r = 0; r < (uint32_t)B; r++)
                    for (uint32_t k = 0; k < (uint32_t)T; k++) {
                        const uint32_t col = g * T + k;
                        // (the kernel loads whole 16-byte pieces: the row's padding rides along and is never used)
                        at(slot, r + 1, k) = band0 + r < p.height && col < p.width ? diff_row(p, band0 + r)[col] : (uint16_t)0;
                    }
                for (uint32_t k = 0; k < (uint32_t)T; k++) {
                    const uint32_t col = g * T + k;
                    at(slot, 0, k) = band0 > 0 && col < p.width ? above[col] : (uint16_t)0;
                }
            }
            if (g > ntiles) continue;
            for (int k = 0; k < T; k++) {
                int moved[B];
                for (int lane = 0; lane < B; lane++) moved[lane] = a[lane ? lane - 1 : 0];  // __shfl_up(a, 1)
                for (int lane = 0; lane < B; lane++) {
                    const int j = (int)(g * T) + k - lane;
                    const bool in_row = j >= 0 && j < (int)p.width;
                    const uint32_t slot = ((uint32_t)j >> 6) & 1, col = (uint32_t)j & 63;
                    int above_now = moved[lane];
                    if (lane == 0 && in_row) above_now = at(slot, 0, col);
                    c[lane] = b[lane];
                    b[lane] = above_now;
                    const uint32_t row = band0 + (uint32_t)lane;
                    if (row < p.height && in_row) {
                        const bool first_row = row % p.restart_rows == 0;
                        a[lane] = (int)lossless_state(lossless_predict_at((int)p.ps, first_row, (uint32_t)j, (int)p.init, a[lane], b[lane], c[lane]),
                                                      at(slot, (uint32_t)lane + 1, col));
                        at(slot, (uint32_t)lane + 1, col) = (uint16_t)a[lane];
                    }
                }
            }
        }
    }
}

hipjpegStatus_t lossless_decode_host(const uint8_t* data, size_t length, const hipjpegLosslessOutput_t& output, int schedule)
{
    LosslessFrame f;
    hipjpegStatus_t st = lossless_frame(data, length, &f);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = lossless_output_ok(f, output)) != HIPJPEG_STATUS_SUCCESS) return st;
    if (schedule == 1 && f.ps != 1) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    const size_t pitch = lossless_diff_pitch((uint32_t)f.width), plane_samples = pitch * (size_t)f.height;
    std::vector<uint16_t> diffs(plane_samples * (size_t)f.ncomp);
    uint16_t* planes[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t diff[4] = {0, 0, 0, 0}, scratch[4] = {0, 0, 0, 0};
    for (int c = 0; c < f.ncomp; c++) {
        planes[c] = diffs.data() + plane_samples * (size_t)c;
        diff[c] = (uint64_t)reinterpret_cast<uintptr_t>(planes[c]);
    }
    if ((st = lossless_entropy_decode(data, f, planes, pitch)) != HIPJPEG_STATUS_SUCCESS) return st;
    LosslessPlane p[4];
    lossless_planes(f, output, diff, scratch, p);
    for (int c = 0; c < f.ncomp; c++) {
        if (schedule < 0)
            lossless_reconstruct_plain(p[c]);
        else if (schedule == 1 || (schedule == 0 && lossless_takes_rows_kernel(p[c].ps, p[c].width)))
            lossless_rows_schedule(p[c]);
        else
            lossless_wavefront_schedule(p[c]);
    }
    return HIPJPEG_STATUS_SUCCESS;
}

}  // namespace hipjpeg

using namespace hipjpeg;

namespace {
template <class F>
hipjpegStatus_t guarded(F&& body) noexcept  // no C++ exception crosses the C boundary
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return HIPJPEG_STATUS_ALLOC_FAILED;
    } catch (...) {
        return HIPJPEG_STATUS_INTERNAL_ERROR;
    }
}
}  // namespace

extern "C" hipjpegStatus_t hipjpegLosslessKernelShape(hipjpegLosslessKernelShape_t* shape)
{
    if (!shape) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    shape->band_rows = kLosslessBandRows;
    shape->tile_columns = kLosslessTileCols;
    shape->chunk_samples = kLosslessChunkSamples;
    shape->rows_min_width = kLosslessRowsMinWidth;
    return HIPJPEG_STATUS_SUCCESS;
}

extern "C" hipjpegStatus_t hipjpegGetLosslessInfo(const uint8_t* data, size_t length, hipjpegLosslessInfo_t* info)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!data || !info) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        memset(info, 0, sizeof *info);
        LosslessFrame f;
        const hipjpegStatus_t st = lossless_frame(data, length, &f);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        info->width = f.width;
        info->height = f.height;
        info->num_components = f.ncomp;
        info->precision = f.precision;
        info->predictor = f.ps;
        info->point_transform = f.pt;
        info->restart_rows = f.restart_rows;
        for (int c = 0; c < f.ncomp; c++) info->component_id[c] = f.comp_id[c];
        return HIPJPEG_STATUS_SUCCESS;
    });
}

extern "C" hipjpegStatus_t hipjpegDecodeLosslessHost(const uint8_t* data, size_t length, const hipjpegLosslessOutput_t* output)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!data || !output) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        return lossless_decode_host(data, length, *output, /*schedule=*/-1);
    });
}

extern "C" hipjpegStatus_t hipjpegLosslessReconstructAlgorithmHost(const uint8_t* data, size_t length, const hipjpegLosslessOutput_t* output, int kernel)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!data || !output || kernel < 0 || kernel > 2) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        return lossless_decode_host(data, length, *output, kernel);
    });
}
