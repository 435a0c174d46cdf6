// lossless_gpu_host.cpp -- see lossless_gpu_host.h
#include "lossless_gpu_host.h"
#include "scratch_fill.h"

#include <cstring>
#include <new>

#include "../../include/hipjpeg.h"

namespace hipjpeg {

bool lossless_gpu_segments(const uint8_t* data, const LosslessFrame& f, std::vector<LlRawSegment>* out)
{
    out->clear();
    if (f.data_end <= f.data_begin || f.data_end - f.data_begin >= ((size_t)1 << 29)) return false;
    const size_t rows = (size_t)f.interval_rows();
    const size_t expected = ((size_t)f.height + rows - 1) / rows;
    if (lossless_gpu_samples(f, 0) > 0xFFFFFFFFull) return false;  // (more samples than a scan below 2^32 bits can hold)
    for (int i = 0; i < f.ncomp; i++) {
        uint32_t symbols = 0;
        for (int l = 1; l <= 16; l++) symbols += f.table[i].bits[l];
        if (symbols > kLlSpecSymbols) return false;
    }
    const uint8_t *p = data + f.data_begin, *end = data + f.data_end;
    const uint8_t* begin = p;
    int markers = 0;
    while (p < end) {
        const uint8_t* q = (const uint8_t*)memchr(p, 0xFF, (size_t)(end - p));
        if (!q || q + 1 >= end) {  // no further FF, or a lone one that closes the data
            p = q ? q : end;
            break;
        }
        if (q[1] == 0) {
            p = q + 2;
            continue;
        }
        // a marker, or fill bytes in front of one: the interval ends here
        const uint8_t* r = q;
        while (r < end && *r == 0xFF) r++;
        if (r >= end || *r != 0xD0 + (markers & 7)) return false;
        if (q == begin) return false;
        out->push_back(LlRawSegment{(size_t)(begin - data), (size_t)(q - data)});
        markers++;
        begin = p = r + 1;
    }
    if (p == begin) return false;
    out->push_back(LlRawSegment{(size_t)(begin - data), (size_t)(p - data)});
    return out->size() == expected;
}

uint32_t lossless_gpu_tables(const LosslessFrame& f, uint32_t* specs)
{
    bool shared = true;
    for (int i = 1; i < f.ncomp; i++)
        if (memcmp(f.table[i].bits, f.table[0].bits, sizeof f.table[0].bits) || memcmp(f.table[i].vals, f.table[0].vals, sizeof f.table[0].vals))
            shared = false;
    const uint32_t n = shared ? 1u : (uint32_t)f.ncomp;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t bytes[kLlSpecBytes];
        memcpy(bytes, f.table[i].bits + 1, 16);
        memcpy(bytes + 16, f.table[i].vals, kLlSpecSymbols);
        for (uint32_t w = 0; w < kLlSpecWords; w++)
            specs[i * kLlSpecWords + w] = (uint32_t)bytes[4 * w] | ((uint32_t)bytes[4 * w + 1] << 8) | ((uint32_t)bytes[4 * w + 2] << 16) | ((uint32_t)bytes[4 * w + 3] << 24);
    }
    return n;
}

namespace {

struct HostEnv {
    const uint8_t* stream;
    uint32_t nwords;
    const uint32_t* tables;
    uint32_t word(uint32_t k) const
    {
        if (k >= nwords) return 0xFFFFFFFFu;
        const uint8_t* b = stream + (size_t)k * 4;
        return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
    }
    uint32_t tab(uint32_t t, uint32_t w) const { return tables[t * kLlTableWords + w]; }
};

struct HostSink {
    uint16_t* const* plane;
    size_t pitch;
    uint32_t ncomp, width, height;
    LlCursor cur;
    uint32_t k, samples;
    void operator()(uint32_t v)
    {
        if (k < samples && cur.row < height) plane[cur.comp][(size_t)cur.row * pitch + cur.x] = (uint16_t)v;
        k++;
        cur.next(ncomp, width);
    }
};

// One segment through the kernels' schedule.  Returns its verdict bits.
uint32_t segment_schedule(const uint8_t* raw, uint32_t raw_bytes, const uint32_t* tables, uint32_t ntables, uint32_t ncomp, uint32_t width,
                          uint32_t height, uint32_t first_row, uint32_t samples, uint16_t* const plane[4], size_t pitch)
{
    // ---- destuff: count per chunk, then compact
    const uint32_t nchunks = (raw_bytes + kLlDestuffChunk - 1) / kLlDestuffChunk;
    std::vector<uint32_t> drops = device_scratch<uint32_t>(nchunks);  // ll_destuff_count_kernel stores every chunk's count
    const auto byte = [&](uint32_t i) -> uint32_t { return i < raw_bytes ? raw[i] : 0x01u; };
    const auto lane_mask = [&](uint32_t off) -> uint32_t {
        if (off >= raw_bytes) return 0u;
        const uint32_t len = raw_bytes - off < kLlDestuffLaneBytes ? raw_bytes - off : kLlDestuffLaneBytes;
        return ll_destuff_mask(byte, off, kLlDestuffLaneBytes) & ((1u << len) - 1u);
    };
    for (uint32_t c = 0; c < nchunks; c++) {
        uint32_t total = 0;  // (the workgroup's sum: registers and LDS)
        for (uint32_t t = 0; t < kLlLanes; t++) total += (uint32_t)__builtin_popcount(lane_mask(c * kLlDestuffChunk + t * kLlDestuffLaneBytes));
        drops[c] = total;
    }
    // the destuffed stream: the kept bytes, and ones up to the end of the last word (ll_destuff_compact_kernel's last chunk, below)
    std::vector<uint8_t> stream = device_scratch<uint8_t>(((size_t)raw_bytes + 3) & ~(size_t)3);
    uint32_t before = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        uint32_t excl = 0;
        for (uint32_t t = 0; t < kLlLanes; t++) {
            const uint32_t off = c * kLlDestuffChunk + t * kLlDestuffLaneBytes;
            if (off >= raw_bytes) break;
            const uint32_t mask = lane_mask(off);
            const uint32_t len = raw_bytes - off < kLlDestuffLaneBytes ? raw_bytes - off : kLlDestuffLaneBytes;
            uint8_t* dst = stream.data() + (off - before - excl);
            for (uint32_t i = 0; i < len; i++)
                if (!((mask >> i) & 1u)) *dst++ = raw[off + i];
            excl += (uint32_t)__builtin_popcount(mask);
        }
        before += drops[c];
    }
    const uint32_t total_bits = (raw_bytes - before) * 8u;
    for (uint32_t b = raw_bytes - before; b < ((raw_bytes - before + 3u) & ~3u); b++) stream[b] = 0xFF;

    // ---- pass 0, rounds, ripple launches
    const uint32_t nsub = ll_num_subseq(total_bits);
    const uint32_t nunits = (nsub + kLlLanes - 1) / kLlLanes;
    // (device scratch, all five: launch 0 writes start / end / count of every subsequence, and unit_out[0 ..] and unit_count of every unit)
    std::vector<uint64_t> start = device_scratch<uint64_t>(nsub), end = device_scratch<uint64_t>(nsub),
                          unit_out = device_scratch<uint64_t>(2 * (size_t)nunits);
    std::vector<uint32_t> count = device_scratch<uint32_t>(nsub), unit_count = device_scratch<uint32_t>(nunits);
    HostEnv env{stream.data(), (total_bits + 31u) / 32u, tables};
    const bool shared = ntables == 1u;
    const uint32_t phases = shared ? 1u : ncomp;
    LlNoSink none;
    for (uint32_t launch = 0; launch <= kLlMaxRipple; launch++)
        for (uint32_t unit = 0; unit < nunits; unit++) {
            const uint32_t first = unit * kLlLanes;
            const uint32_t lanes = nsub - first < kLlLanes ? nsub - first : kLlLanes;
            const size_t out_now = (size_t)(launch & 1u) * nunits + unit, out_before = (size_t)((launch & 1u) ^ 1u) * nunits + unit;
            uint64_t incoming = 0;
            if (launch > 0) {
                bool need = false;
                if (first > 0) incoming = unit_out[out_before - 1];
                for (uint32_t t = 0; t < lanes; t++) {
                    if (first + t == 0) continue;
                    const uint64_t pred = t > 0 ? end[first + t - 1] : incoming;
                    need = need || (pred != kLlInvalidPacked && pred != start[first + t]);
                }
                unit_out[out_now] = unit_out[out_before];
                if (!need) continue;
            } else {
                for (uint32_t t = 0; t < lanes; t++) {
                    const uint32_t i = first + t;
                    LlState st{0u, 0u}, from = st;
                    if (i == 0)
                        count[i] = ll_parse(env, phases, shared, total_bits, ll_limit(i, total_bits), &st, none);
                    else
                        count[i] = ll_pass0(env, phases, shared, total_bits, i, ll_limit(i, total_bits), &from, &st);
                    start[i] = ll_pack(from);
                    end[i] = ll_pack(st);
                }
            }
            for (uint32_t round = 0; round < kLlMaxRounds; round++) {
                // every lane looks at the end states as the round before left them
                std::vector<uint64_t> pred(lanes);
                bool any = false;
                for (uint32_t t = 0; t < lanes; t++) {
                    pred[t] = t > 0 ? end[first + t - 1] : (launch > 0 && first > 0 ? incoming : start[first]);
                    any = any || (pred[t] != kLlInvalidPacked && pred[t] != start[first + t]);
                }
                if (!any) break;
                for (uint32_t t = 0; t < lanes; t++) {
                    const uint32_t i = first + t;
                    if (pred[t] == kLlInvalidPacked || pred[t] == start[i]) continue;
                    LlState st = ll_unpack(pred[t]);
                    start[i] = pred[t];
                    count[i] = ll_parse(env, phases, shared, total_bits, ll_limit(i, total_bits), &st, none);
                    end[i] = ll_pack(st);
                }
            }
            unit_out[out_now] = end[first + lanes - 1];
            uint32_t total = 0;
            for (uint32_t t = 0; t < lanes; t++) total += count[first + t];
            unit_count[unit] = total;
        }

    // ---- the write pass
    uint32_t verdict = 0, k = 0;
    for (uint32_t i = 0; i < nsub; i++) {
        const uint64_t pred = i == 0 ? 0ull : end[i - 1];
        if (pred != start[i]) verdict |= kLlUnconverged;
        if (end[i] == kLlInvalidPacked) verdict |= kLlInvalidCode;
        if (count[i] != 0 && k < samples) {
            HostSink sink{plane, pitch, ncomp, width, height, LlCursor(), k, samples};
            sink.cur.start(ncomp, width, first_row, k);
            LlState st = ll_unpack(start[i]);
            st.phase = sink.cur.comp;
            (void)ll_parse(env, ncomp, shared, total_bits, ll_limit(i, total_bits), &st, sink);
        }
        k += count[i];
    }
    if (k != samples) verdict |= kLlBadCount;
    return verdict;
}

}  // namespace

bool lossless_gpu_algorithm_host(const uint8_t* data, const LosslessFrame& f, uint16_t* const planes[4], size_t pitch, uint32_t* verdict)
{
    *verdict = 0;
    std::vector<LlRawSegment> segments;
    if (!lossless_gpu_segments(data, f, &segments)) return false;
    uint32_t specs[4 * kLlSpecWords];
    const uint32_t ntables = lossless_gpu_tables(f, specs);
    std::vector<uint32_t> tables(4 * kLlTableWords);
    for (uint32_t t = 0; t < ntables; t++) {
        const uint32_t* words = specs + t * kLlSpecWords;
        const auto spec = [words](uint32_t i) -> uint32_t { return (words[i >> 2] >> (8u * (i & 3u))) & 0xFFu; };
        for (uint32_t w = 0; w < kLlTableWords; w++) tables[t * kLlTableWords + w] = ll_table_word(spec, w);  // (the kernels: a word per lane)
    }
    uint16_t* by_position[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < f.ncomp; i++) by_position[i] = planes[f.scan_comp[i]];
    for (size_t k = 0; k < segments.size(); k++)
        *verdict |= segment_schedule(data + segments[k].begin, (uint32_t)(segments[k].end - segments[k].begin), tables.data(), ntables, (uint32_t)f.ncomp,
                                     (uint32_t)f.width, (uint32_t)f.height, lossless_gpu_first_row(f, k), (uint32_t)lossless_gpu_samples(f, k),
                                     by_position, pitch);
    return true;
}

}  // namespace hipjpeg

// ---------------------------------------------------------------------------------------------------------------- C entry points
// (here, not in hipjpeg_api.cpp, so that they link without the HIP runtime: tests, sanitizer programs)
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

// the frame of a file and the caller's planes checked against it
hipjpegStatus_t frame_and_planes(const uint8_t* data, size_t length, uint16_t* const planes[4], size_t pitch, LosslessFrame* f)
{
    if (!data || !planes) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    const hipjpegStatus_t st = lossless_frame(data, length, f);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    for (int c = 0; c < f->ncomp; c++)
        if (!planes[c]) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return pitch < (size_t)f->width ? HIPJPEG_STATUS_INVALID_ARGUMENT : HIPJPEG_STATUS_SUCCESS;
}
}  // namespace

extern "C" hipjpegStatus_t hipjpegLosslessEntropyShape(hipjpegLosslessEntropyShape_t* shape)
{
    if (!shape) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    shape->subsequence_bits = (int32_t)kLlSubseqBits;
    shape->subsequences_per_workgroup = (int32_t)kLlLanes;
    shape->max_rounds = (int32_t)kLlMaxRounds;
    shape->max_ripple_launches = (int32_t)kLlMaxRipple;
    return HIPJPEG_STATUS_SUCCESS;
}

extern "C" hipjpegStatus_t hipjpegLosslessEntropyHost(const uint8_t* data, size_t length, uint16_t* const planes[4], size_t pitch)
{
    return guarded([&]() -> hipjpegStatus_t {
        LosslessFrame f;
        const hipjpegStatus_t st = frame_and_planes(data, length, planes, pitch, &f);
        return st != HIPJPEG_STATUS_SUCCESS ? st : lossless_entropy_decode(data, f, planes, pitch);
    });
}

extern "C" hipjpegStatus_t hipjpegLosslessEntropyAlgorithmHost(const uint8_t* data, size_t length, uint16_t* const planes[4], size_t pitch,
                                                               int32_t* converged)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (converged) *converged = 1;
        LosslessFrame f;
        const hipjpegStatus_t st = frame_and_planes(data, length, planes, pitch, &f);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        uint32_t verdict = 0;
        const bool ran = lossless_gpu_algorithm_host(data, f, planes, pitch, &verdict);
        if (converged) *converged = (verdict & kLlUnconverged) ? 0 : 1;
        if (ran && verdict == 0) return HIPJPEG_STATUS_SUCCESS;
        return lossless_entropy_decode(data, f, planes, pitch);  // as the batch call does: the host stage names the status
    });
}
