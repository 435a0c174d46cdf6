// lossless_encode_host.cpp -- see lossless_encode_host.h.  Header rules: libjpeg-turbo's jcmarker.c in lossless mode (jcparam.c
// jpeg_set_colorspace for the component ids and the APPn choice); table: jchuff.c jpeg_gen_optimal_table (entropy_encode.cpp).
#include "lossless_encode_host.h"

#include <algorithm>
#include <cstring>

#include "entropy_encode.h"
#include "scratch_fill.h"

namespace hipjpeg {

hipjpegStatus_t lossless_encode_describe(const hipjpegLosslessEncodeInput_t& in, const hipjpegLosslessEncodeParams_t& p, LencImage* im)
{
    if (p.precision < 2 || p.precision > 16 || p.predictor < 1 || p.predictor > 7 || p.point_transform < 0 || p.point_transform >= p.precision ||
        p.num_components < 1 || p.num_components > 4 || p.restart_rows < 0)
        return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (in.width < 1 || in.width > 65535 || in.height < 1 || in.height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if ((int64_t)p.restart_rows * in.width > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (in.sample_bytes != 1 && in.sample_bytes != 2) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (in.sample_bytes == 1 && p.precision > 8) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    const int n = p.num_components;
    const uint64_t row_bytes = (uint64_t)in.width * (uint64_t)in.sample_bytes * (uint64_t)(in.planar ? 1 : n);
    for (int c = 0; c < (in.planar ? n : 1); c++)
        if (!in.plane[c] || in.pitch[c] < row_bytes) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    *im = LencImage();
    uint64_t plane[4] = {0, 0, 0, 0};
    uint32_t pitch[4] = {0, 0, 0, 0};
    for (int c = 0; c < n; c++) {
        plane[c] = in.planar ? (uint64_t)reinterpret_cast<uintptr_t>(in.plane[c])
                             : (uint64_t)reinterpret_cast<uintptr_t>(in.plane[0]) + (uint64_t)c * (uint64_t)in.sample_bytes;
        pitch[c] = in.planar ? in.pitch[c] : in.pitch[0];
    }
    im->plane0 = plane[0], im->plane1 = plane[1], im->plane2 = plane[2], im->plane3 = plane[3];
    im->pitch0 = pitch[0], im->pitch1 = pitch[1], im->pitch2 = pitch[2], im->pitch3 = pitch[3];
    im->step = (uint32_t)in.sample_bytes * (uint32_t)(in.planar ? 1 : n);
    im->sample_bytes = (uint32_t)in.sample_bytes;
    im->width = (uint32_t)in.width;
    im->height = (uint32_t)in.height;
    im->ncomp = (uint32_t)n;
    im->ps = (uint32_t)p.predictor;
    im->pt = (uint32_t)p.point_transform;
    im->init = 1u << (p.precision - p.point_transform - 1);
    im->interval_rows = p.restart_rows ? std::min((uint32_t)p.restart_rows, im->height) : im->height;
    im->row_samples = im->width * im->ncomp;
    // 65535 * 65535 * 4 does not fit 32 bits: such pictures are described (the host coders count in 64 bits below) but the kernels'
    // predicate turns them away long before
    const uint64_t total = (uint64_t)im->row_samples * im->height;
    im->total_samples = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
    const uint64_t iv = (uint64_t)im->interval_rows * im->row_samples;
    im->interval_samples = iv > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)iv;
    im->num_groups = (uint32_t)((total + kLencGroup - 1) / kLencGroup);
    return HIPJPEG_STATUS_SUCCESS;
}

namespace {

void put16(std::vector<uint8_t>* o, int v)
{
    o->push_back((uint8_t)(v >> 8));
    o->push_back((uint8_t)v);
}

struct HostWords {  // big-endian words in an array of host-order words, as the kernel's LDS window holds them
    uint32_t* window;
    uint32_t word0;
    void or_word(uint32_t i, uint32_t w) const { window[i - word0] |= w; }
};

// the plain coder's bit sink: bytes as they complete, a zero behind every FF
struct ByteSink {
    std::vector<uint8_t>* out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t bits, uint32_t size)
    {
        acc = (acc << size) | bits;
        n += (int)size;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            out->push_back(b);
            if (b == 0xFF) out->push_back(0);
            n -= 8;
        }
    }
    void pad()
    {
        if (n) put((1u << (8 - n)) - 1, (uint32_t)(8 - n));
    }
};

}  // namespace

void lossless_encode_headers(const LencImage& im, const hipjpegLosslessEncodeParams_t& p, const uint32_t counts[kLencSymbols],
                             uint32_t codes[kLencSymbols], std::vector<uint8_t>* o)
{
    uint8_t bits[17], vals[17];
    int nvals = 0;
    lossless_optimal_table(counts, bits, vals, &nvals, codes);
    const int n = (int)im.ncomp;
    static const uint8_t kIds[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}, {0x52, 0x47, 0x42, 0}, {0x43, 0x4D, 0x59, 0x4B}};
    put16(o, 0xFFD8);
    if (n == 1) {  // JCS_GRAYSCALE: JFIF 1.01, no units, 1:1, no thumbnail
        static const uint8_t kJfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        put16(o, 0xFFE0);
        put16(o, 16);
        o->insert(o->end(), kJfif, kJfif + 14);
    } else if (n >= 3) {  // JCS_RGB / JCS_CMYK: Adobe version 100, no flags, transform 0
        static const uint8_t kAdobe[12] = {'A', 'd', 'o', 'b', 'e', 0, 100, 0, 0, 0, 0, 0};
        put16(o, 0xFFEE);
        put16(o, 14);
        o->insert(o->end(), kAdobe, kAdobe + 12);
    }
    put16(o, 0xFFC3);
    put16(o, 8 + 3 * n);
    o->push_back((uint8_t)p.precision);
    put16(o, (int)im.height);
    put16(o, (int)im.width);
    o->push_back((uint8_t)n);
    for (int c = 0; c < n; c++) {
        o->push_back(kIds[n][c]);
        o->push_back(0x11);
        o->push_back(0);
    }
    put16(o, 0xFFC4);
    put16(o, 2 + 1 + 16 + nvals);
    o->push_back(0);
    o->insert(o->end(), bits + 1, bits + 17);
    o->insert(o->end(), vals, vals + nvals);
    if (p.restart_rows) {
        put16(o, 0xFFDD);
        put16(o, 4);
        put16(o, (int)((uint32_t)p.restart_rows * im.width));
    }
    put16(o, 0xFFDA);
    put16(o, 6 + 2 * n);
    o->push_back((uint8_t)n);
    for (int c = 0; c < n; c++) {
        o->push_back(kIds[n][c]);
        o->push_back(0);
    }
    o->push_back((uint8_t)p.predictor);
    o->push_back(0);
    o->push_back((uint8_t)p.point_transform);
}

namespace {

// sample (row, col, c) by coordinates: the plain coder counts in 64 bits and never forms a scan index
uint32_t plain_difference(const LencImage& im, uint32_t row, uint32_t col, uint32_t c)
{
    const bool first_row = row % im.interval_rows == 0;
    const int x = lenc_state(im, c, row, col);
    const int a = col ? lenc_state(im, c, row, col - 1) : 0;
    const int b = first_row ? 0 : lenc_state(im, c, row - 1, col);
    const int cc = !first_row && col ? lenc_state(im, c, row - 1, col - 1) : 0;
    return lenc_difference(im, row, col, x, a, b, cc);
}

}  // namespace

void lossless_encode_plain(const LencImage& im, const hipjpegLosslessEncodeParams_t& p, std::vector<uint8_t>* out)
{
    uint32_t counts[kLencSymbols] = {0};
    for (uint32_t row = 0; row < im.height; row++)
        for (uint32_t col = 0; col < im.width; col++)
            for (uint32_t c = 0; c < im.ncomp; c++) counts[lenc_category(plain_difference(im, row, col, c))]++;
    uint32_t codes[kLencSymbols];
    lossless_encode_headers(im, p, counts, codes, out);
    ByteSink sink{out};
    for (uint32_t row = 0; row < im.height; row++) {
        if (row && row % im.interval_rows == 0) {  // jclhuff.c emit_restart: flush, RSTn
            sink.pad();
            out->push_back(0xFF);
            out->push_back((uint8_t)(0xD0 + ((row / im.interval_rows - 1) & 7)));
        }
        for (uint32_t col = 0; col < im.width; col++)
            for (uint32_t c = 0; c < im.ncomp; c++) {
                const uint32_t d = plain_difference(im, row, col, c);
                uint32_t nbits;
                const uint32_t bits = lenc_symbol(d, codes[lenc_category(d)], &nbits);
                sink.put(bits, nbits);
            }
    }
    sink.pad();
    put16(out, 0xFFD9);
}

// The kernels' schedule (lossless_encode_kernels.hip), lane by lane.  Callers make sure lenc_offsets_fit holds.
void lossless_encode_gpu_algorithm(const LencImage& im, const hipjpegLosslessEncodeParams_t& p, std::vector<uint8_t>* out)
{
    constexpr uint32_t kLanes = kLencThreads;
    const uint32_t ngroups = im.num_groups;
    const uint32_t nwg = (ngroups + kLanes - 1) / kLanes;
    // statistics: 17 counters per workgroup in LDS, flushed with one atomic per counter into memory the batch cleared
    uint32_t counts[kLencSymbols];
    memset(counts, 0, sizeof counts);  // (stands for the hipMemsetAsync of the counters in LosslessEncodeBatch::encode())
    // (the kernel's workgroups stride over the pieces; which workgroup takes which piece changes no sum)
    for (uint32_t piece = 0; piece < lenc_pieces(im); piece++) {
        uint32_t lds[kLencSymbols] = {0};  // zeroed LDS
        struct Count {
            uint32_t* lds;
            void add(uint32_t ssss) const { lds[ssss]++; }
        };
        for (uint32_t t = 0; t < kLanes; t++) lenc_stat_lane(im, piece, t, Count{lds});
        for (int i = 0; i < kLencSymbols; i++) counts[i] += lds[i];
    }
    uint32_t codes[kLencSymbols];
    std::vector<uint8_t> header;
    lossless_encode_headers(im, p, counts, codes, &header);
    // length: a span per group
    std::vector<uint32_t> spans = device_scratch<uint32_t>(ngroups);  // lenc_length_kernel stores every group's
    for (uint32_t g = 0; g < ngroups; g++) spans[g] = lenc_pack_span(lenc_group_span(im, g, codes));
    // scan: every lane's range, the doubling steps over the lanes' spans, every lane's range again
    std::vector<uint32_t> off = device_scratch<uint32_t>(ngroups);  // lenc_scan_kernel stores every group's
    const uint32_t per = (ngroups + kLanes - 1) / kLanes;
    HencSpan sum[kLanes];
    for (uint32_t t = 0; t < kLanes; t++) {
        const uint32_t lo = std::min(ngroups, t * per), hi = std::min(ngroups, lo + per);
        HencSpan sp{0u, 0u, 0u};
        for (uint32_t i = lo; i < hi; i++) sp = henc_span_join(sp, lenc_unpack_span(spans[i]));
        sum[t] = sp;
    }
    for (uint32_t d = 1; d < kLanes; d <<= 1) {
        HencSpan next[kLanes];
        for (uint32_t t = 0; t < kLanes; t++) next[t] = t >= d ? henc_span_join(sum[t - d], sum[t]) : sum[t];
        memcpy(sum, next, sizeof sum);
    }
    for (uint32_t t = 0; t < kLanes; t++) {
        const uint32_t lo = std::min(ngroups, t * per), hi = std::min(ngroups, lo + per);
        uint32_t run = t ? henc_span_apply(0u, sum[t - 1]) : 0u;
        for (uint32_t i = lo; i < hi; i++) {
            off[i] = run;
            run = henc_span_apply(run, lenc_unpack_span(spans[i]));
        }
    }
    const uint32_t total = henc_span_apply(0u, sum[kLanes - 1]);
    // write: per workgroup a zeroed window over [offset of its first group, offset of the next workgroup's first group); whole words
    // out, the two end words OR-ed.  The bit buffer and the bitmap behind it are zeroed (henc_zero_kernel over all bit buffers).
    const uint32_t raw_bytes = (total + 7) / 8;
    std::vector<uint32_t> raw(((size_t)henc_map_offset(raw_bytes) + henc_map_bytes(raw_bytes)) / 4, 0u);
    uint8_t* const rawb = reinterpret_cast<uint8_t*>(raw.data());
    uint8_t* const map = rawb + henc_map_offset(raw_bytes);
    std::vector<uint32_t> window((size_t)kLencWindowWords);
    for (uint32_t wg = 0; wg < nwg; wg++) {
        const uint32_t g0 = wg * kLanes;
        const uint32_t first_bit = off[g0], end_bit = g0 + kLanes < ngroups ? off[g0 + kLanes] : raw_bytes * 8u;
        if (end_bit == first_bit) continue;
        const uint32_t w0 = first_bit >> 5, nwin = ((end_bit - 1) >> 5) - w0 + 1;
        std::fill(window.begin(), window.begin() + nwin, 0u);
        for (uint32_t t = 0; t < kLanes && g0 + t < ngroups; t++) {
            HencEmitter<HostWords> em;
            em.start(HostWords{window.data(), w0}, off[g0 + t]);
            lenc_group_write(im, g0 + t, off[g0 + t], codes, &em, [&](uint32_t byte) { map[byte >> 3] |= (uint8_t)(1u << (byte & 7)); });
            em.finish();
        }
        for (uint32_t i = 0; i < nwin; i++) {
            const uint32_t w = __builtin_bswap32(window[i]);
            if (i == 0 || i == nwin - 1)
                raw[w0 + i] |= w;
            else
                raw[w0 + i] = w;
        }
    }
    // count / layout / expand: chunk by chunk, a 0x00 behind every 0xFF that is no marker's
    const uint32_t nchunks = (raw_bytes + kHencChunk - 1) / kHencChunk;
    const bool rst = lenc_intervals(im) > 1;
    const uint16_t* pieces = reinterpret_cast<const uint16_t*>(map);
    auto stuffed = [&](uint32_t b) { return rawb[b] == 0xFF && !(rst && henc_is_marker(pieces, b)); };
    std::vector<uint32_t> ff = device_scratch<uint32_t>(nchunks), before = device_scratch<uint32_t>(nchunks);  // every chunk's is stored
    for (uint32_t c = 0; c < nchunks; c++) {
        uint32_t n = 0;
        for (uint32_t b = c * kHencChunk; b < std::min(raw_bytes, (c + 1) * (uint32_t)kHencChunk); b++) n += stuffed(b);
        ff[c] = n;
    }
    uint32_t run = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        before[c] = run;
        run += ff[c];
    }
    const size_t base = out->size(), hb = header.size();
    out->resize(base + hb + raw_bytes + run + 2);
    uint8_t* file = out->data() + base;
    memcpy(file, header.data(), hb);
    for (uint32_t c = 0; c < nchunks; c++) {
        size_t o = hb + (size_t)c * kHencChunk + before[c];
        for (uint32_t b = c * kHencChunk; b < std::min(raw_bytes, (c + 1) * (uint32_t)kHencChunk); b++) {
            file[o++] = rawb[b];
            if (stuffed(b)) file[o++] = 0;
        }
    }
    file[hb + raw_bytes + run] = 0xFF;
    file[hb + raw_bytes + run + 1] = 0xD9;
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

hipjpegStatus_t encode_host(const hipjpegLosslessEncodeInput_t* input, const hipjpegLosslessEncodeParams_t* params, uint8_t* out, size_t capacity,
                            size_t* out_length, bool twin)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!input || !params || !out_length || (!out && capacity)) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        LencImage im;
        const hipjpegStatus_t st = lossless_encode_describe(*input, *params, &im);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        std::vector<uint8_t> file;
        if (twin) {
            if (!lenc_offsets_fit((uint64_t)im.row_samples * im.height, lenc_intervals(im))) return HIPJPEG_STATUS_UNSUPPORTED;
            lossless_encode_gpu_algorithm(im, *params, &file);
        } else {
            lossless_encode_plain(im, *params, &file);
        }
        *out_length = file.size();
        if (file.size() > capacity) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
        memcpy(out, file.data(), file.size());
        return HIPJPEG_STATUS_SUCCESS;
    });
}
}  // namespace

extern "C" hipjpegStatus_t hipjpegLosslessEncodeShape(hipjpegLosslessEncodeShape_t* shape)
{
    if (!shape) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    shape->group_samples = kLencGroup;
    shape->window_samples = kLencWindowSamples;
    shape->chunk_bytes = kHencChunk;
    return HIPJPEG_STATUS_SUCCESS;
}

extern "C" int hipjpegLosslessEncodeFitsGpu(uint64_t samples, uint64_t intervals)
{
    // 31 * samples must not wrap either: 2^59 samples is far beyond any picture the argument rules allow
    return samples < (1ull << 58) && intervals < (1ull << 58) && lenc_offsets_fit(samples, intervals) ? 1 : 0;
}

extern "C" hipjpegStatus_t hipjpegEncodeLosslessHost(const hipjpegLosslessEncodeInput_t* input, const hipjpegLosslessEncodeParams_t* params, uint8_t* out,
                                                     size_t capacity, size_t* out_length)
{
    return encode_host(input, params, out, capacity, out_length, false);
}

extern "C" hipjpegStatus_t hipjpegEncodeLosslessGpuAlgorithmHost(const hipjpegLosslessEncodeInput_t* input, const hipjpegLosslessEncodeParams_t* params,
                                                                 uint8_t* out, size_t capacity, size_t* out_length)
{
    return encode_host(input, params, out, capacity, out_length, true);
}
