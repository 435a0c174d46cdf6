// hipjpeg_api.cpp -- the C-ABI declared in include/hipjpeg.h (decode side).
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/hipjpeg.h"
#include "coefficients_core.h"
#include "decoder_core.h"
#include "diagnostics.h"
#include "encoder_core.h"
#include "entropy_decode.h"
#include "gpu_huffman_encode.h"
#include "gpu_huffman_host.h"
#include "lossless_batch.h"
#include "lossless_encode_batch.h"
#include "progressive_encode.h"
#include "progressive_gpu_host.h"
#include "scratch_fill.h"
#include "thread_pool.h"
#include "transcode_core.h"

#include <chrono>
#include <future>
#include <cstdio>
#include <cstdlib>

using namespace hipjpeg;

namespace {
// No C++ exception may cross the C boundary (the reference wraps every entry point the same way, e.g.
// extensions/libjpeg_turbo/libjpeg_turbo_decoder.cpp:226-236): whatever is thrown below becomes a status code.
template <class F>
hipjpegStatus_t guarded(F&& body) noexcept
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

struct hipjpegHandle {
    int device_id = 0;
    MemoryHooks hooks;
    std::unique_ptr<ForkJoinPool> pool;
    // three batch pages, used in turn: the host stage and H2D copy of batches k+1 and k+2 proceed while the device is still
    // consuming batch k (same idea as the reference's two pinned pages per thread, cuda_decoder.h:50-53; the third page
    // keeps the copy engine a whole batch ahead of the kernels)
    // (hipjpegSetPipelineDepth: up to kMaxPages, for work whose batches leave most of the chip idle -- progressive scans)
    static constexpr int kMaxPages = 8;
    int pages = 3;
    std::unique_ptr<DecodeBatch> batches[kMaxPages];
    int current = 0;
    int settled = -1;  // page whose batch the last Wait settled, until the next batch is planned (hipjpegTestHostFallbacks)
    DecodeBatch& cur() { return *batches[current]; }
    // pipelined submission (hipjpegDecodeBatchSubmit / Wait): pages in flight, oldest first, with the stream each runs on
    std::vector<hipjpegTransform_t> transforms;  // geometry for the next batch (hipjpegDecodeBatchSetTransforms)
    std::vector<int32_t> scales;                 // scale denominators for the next batch (hipjpegDecodeBatchSetScales)
    // the three batch calls that take no scales: pending ones are dropped and the call refused
    bool drop_pending_scales()
    {
        const bool pending = !scales.empty();
        scales.clear();
        return pending;
    }
    int submitted[kMaxPages] = {-1, -1, -1, -1, -1, -1, -1, -1};
    void* submitted_stream[kMaxPages] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int num_submitted = 0;
    hipStream_t copy_stream = nullptr;  // H2D copies of submitted batches: they overlap the kernels of the batch before
    hipStream_t entropy_stream = nullptr;  // GPU entropy stage of submitted batches: beside the pixel kernels of the batch before
    // batches with progressive images: the walk of a progressive scan is one wave per scan and leaves most of the chip idle, so
    // the entropy stages of consecutive batches run beside EACH OTHER, one stream per page
    hipStream_t page_entropy_stream[kMaxPages] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::unique_ptr<EncodeBatch> encode;
    EncodeBatch* encode_view = nullptr;  // the batch hipjpegEncodeGetBitstream / GetCoefficients / Stats talk about
    // pipelined encoding (hipjpegEncodeBatchSubmit / Wait): three pages, each driven by its own host thread on its own
    // stream, so that the PCIe-bound file output and the two short host round trips of one batch overlap the kernels of the
    // others (two pages fall into lock-step: both batches compute, then both wait for PCIe)
    struct EncodePage {
        std::unique_ptr<EncodeBatch> batch;
        hipStream_t stream = nullptr;
        hipEvent_t ready = nullptr;
        std::future<hipjpegStatus_t> result;
        std::vector<hipjpegEncodeInput_t> inputs;
        std::vector<hipjpegEncodeParams_t> params;
    };
    static constexpr int kEncodePages = 3;
    EncodePage encode_pages[kEncodePages];
    int encode_next = 0, encode_oldest = 0, encode_in_flight = 0;
    // the last hipjpegTranscodeBatch: images on the GPU entropy decoder / coder, blocks through the relayout kernel
    int32_t transcode_gpu_decoded = 0, transcode_gpu_coded = 0, transcode_blocks = 0;
    // hipjpegTranscodeBatchSetRegions: for the next hipjpegTranscodeBatch only
    std::vector<hipjpegTranscodeRegion_t> transcode_regions;
    bool transcode_regions_set = false;
    // the last hipjpegDecodeCoefficientsBatch / hipjpegEncodeCoefficientsBatch: images on the GPU entropy decoder / coder; blocks the
    // last of the four coefficient-tensor calls moved
    int32_t coefficients_gpu_decoded = 0, coefficients_gpu_coded = 0;
    int64_t coefficients_blocks = 0;
    std::unique_ptr<LosslessBatch> lossless;  // hipjpegDecodeLosslessBatch: staging pages of its own, made at the first call
    std::unique_ptr<LosslessEncodeBatch> lossless_encode;  // hipjpegEncodeLosslessBatch: likewise
};

extern "C" {

const char* hipjpegStatusString(hipjpegStatus_t s)
{
    switch (s) {
    case HIPJPEG_STATUS_SUCCESS: return "success";
    case HIPJPEG_STATUS_INVALID_ARGUMENT: return "invalid argument";
    case HIPJPEG_STATUS_BAD_JPEG: return "not a JPEG or malformed marker segment";
    case HIPJPEG_STATUS_UNSUPPORTED: return "JPEG feature outside this decoder's scope";
    case HIPJPEG_STATUS_TRUNCATED: return "entropy-coded data ends early";
    case HIPJPEG_STATUS_CORRUPT: return "corrupt entropy-coded data";
    case HIPJPEG_STATUS_ALLOC_FAILED: return "memory allocation failed";
    case HIPJPEG_STATUS_HIP_ERROR: return "HIP runtime error";
    case HIPJPEG_STATUS_NO_DEVICE: return "no usable HIP device";
    case HIPJPEG_STATUS_BUFFER_TOO_SMALL: return "buffer too small";
    case HIPJPEG_STATUS_INTERNAL_ERROR: return "internal error (exception caught at the C boundary)";
    }
    return "unknown status";
}

int hipjpegVersion(void) { return 200; }

// Batches in flight run their entropy stages on streams of their own (decoder pages, plugin jobs); the HIP runtime multiplexes streams
// onto GPU_MAX_HW_QUEUES hardware queues -- four by default -- and kernels of streams that share a queue run one after the other: with
// six progressive batches in flight their 80 ms walks queued up behind each other.  The runtime reads the variable when
// it initialises, i.e. at the process's first HIP call; this library is normally loaded before that (an extension module is opened when
// the instance is created, the Python package on import), so it asks for twelve queues itself unless the environment already says
// otherwise.  A process that has initialised HIP earlier keeps its setting: nothing breaks, deep pipelines of progressive batches are
// slower.  (the figure must not depend on the caller exporting the variable.)
__attribute__((constructor)) static void hipjpeg_runtime_defaults() { (void)setenv("GPU_MAX_HW_QUEUES", "12", /*overwrite=*/0); }

// The hipjpegTest* entry points exist for the test suite (fault injection, counters the tests assert on).  They answer only in a
// process that was started with HIPJPEG_ENABLE_TEST_HOOKS=1 (read once); anywhere else they refuse -- no caller of a production process can
// arm a throw inside the library.  tests/conftest.py sets the variable; bench.py and the tools do not need the hooks.
static bool test_hooks_enabled()
{
    static const bool on = [] {
        const char* e = getenv("HIPJPEG_ENABLE_TEST_HOOKS");
        return e != nullptr && e[0] == '1';
    }();
    return on;
}

hipjpegStatus_t hipjpegTestSetFault(const char* site, int countdown)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!test_hooks_enabled()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        set_fault(site, countdown);
        return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegTestSetScratchFill(int byte)
{
    if (!test_hooks_enabled() || byte < 0 || byte > 255) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    scratch_fill_byte().store(byte);
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t hipjpegGetImageInfo(const uint8_t* data, size_t length, hipjpegImageInfo_t* info)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!data || !info) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    ParseStatus ps = parse_jpeg(data, length, &f, /*headers_only=*/false);
    memset(info, 0, sizeof *info);
    info->sof_marker = f.sof;
    if (ps != kParseOk) return status_from_parse(ps);
    info->width = f.width;
    info->height = f.height;
    info->num_components = f.ncomp;
    info->color_model = (int)f.color;
    info->subsampling = classify_subsampling(f);
    info->restart_interval = f.scans.empty() ? 0 : f.scans[0].restart_interval;
    info->num_scans = (int)f.scans.size();
    for (int c = 0; c < f.ncomp; c++) {
        info->h[c] = f.comp[c].h;
        info->v[c] = f.comp[c].v;
        info->blocks_w[c] = f.comp[c].blocks_w;
        info->blocks_h[c] = f.comp[c].blocks_h;
        info->samp_w[c] = f.comp[c].samp_w;
        info->samp_h[c] = f.comp[c].samp_h;
    }
    info->coef_bytes = f.total_blocks() * 128;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEntropyDecodeHost(const uint8_t* data, size_t length, int16_t* coef, size_t coef_capacity_bytes,
                                         uint64_t comp_offsets[4], uint16_t qtables[256])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!data || !coef) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    ParseStatus ps = parse_jpeg(data, length, &f);
    if (ps != kParseOk) return status_from_parse(ps);
    if (f.total_blocks() * 128 > coef_capacity_bytes) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    int16_t* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t off = 0;
    for (int c = 0; c < f.ncomp; c++) {
        ptr[c] = coef + off;
        if (comp_offsets) comp_offsets[c] = off;
        off += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64;
        if (qtables)
            for (int j = 0; j < 64; j++) qtables[c * 64 + (j & 7) * 8 + (j >> 3)] = f.qtab[c][j];
    }
    switch (decode_coefficients(data, length, f, ptr)) {
    case kEntropyOk: return HIPJPEG_STATUS_SUCCESS;
    case kEntropyTruncated: return HIPJPEG_STATUS_TRUNCATED;
    case kEntropyMissingTable: return HIPJPEG_STATUS_BAD_JPEG;
    default: return HIPJPEG_STATUS_CORRUPT;
    }
    });
}

hipjpegStatus_t hipjpegEntropyDecodeHostSparse(const uint8_t* data, size_t length, uint8_t* stream, size_t capacity_bytes, size_t* stream_bytes,
                                               uint64_t table_offsets[4])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!data || !stream || !stream_bytes) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    ParseStatus ps = parse_jpeg(data, length, &f);
    if (ps != kParseOk) return status_from_parse(ps);
    if (!sparse_staging_applies(f)) return HIPJPEG_STATUS_UNSUPPORTED;
    if (sparse_stream_capacity(f) > capacity_bytes) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    size_t blocks = 0;
    for (int c = 0; c < f.ncomp; c++) {
        if (table_offsets) table_offsets[c] = blocks;
        blocks += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
    }
    switch (decode_coefficients_sparse(data, length, f, stream, stream_bytes)) {
    case kEntropyOk: return HIPJPEG_STATUS_SUCCESS;
    case kEntropyTruncated: return HIPJPEG_STATUS_TRUNCATED;
    case kEntropyMissingTable: return HIPJPEG_STATUS_BAD_JPEG;
    default: return HIPJPEG_STATUS_CORRUPT;
    }
    });
}

hipjpegStatus_t hipjpegEntropyDecodeGpuAlgorithmHost(const uint8_t* data, size_t length, int16_t* coef, size_t coef_capacity_bytes,
                                                     uint64_t comp_offsets[4], int32_t* sync_passes)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!data || !coef) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    ParseStatus ps = parse_jpeg(data, length, &f);
    if (ps != kParseOk) return status_from_parse(ps);
    const bool progressive = gpu_progressive_eligible(f);
    if (!progressive && !gpu_entropy_eligible(f)) return HIPJPEG_STATUS_UNSUPPORTED;
    if (f.total_blocks() * 128 > coef_capacity_bytes) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    int16_t* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t off = 0;
    for (int c = 0; c < f.ncomp; c++) {
        ptr[c] = coef + off;
        if (comp_offsets) comp_offsets[c] = off;
        off += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64;
    }
    int passes = 0;
    int rc = progressive ? emulate_gpu_progressive(data, length, f, ptr) : emulate_gpu_entropy(data, length, f, ptr, &passes);
    if (sync_passes) *sync_passes = passes;
    // rc 5: a block-start record disagrees with the position walk, or the walk forms or table classes disagree (self-checks of the
    // emulation, not properties of the stream)
    if (rc == 5) return HIPJPEG_STATUS_INTERNAL_ERROR;
    return rc == 0 ? HIPJPEG_STATUS_SUCCESS : (rc == 2 ? HIPJPEG_STATUS_TRUNCATED : HIPJPEG_STATUS_CORRUPT);
    });
}

hipjpegStatus_t hipjpegTestSyncScheduleCounts(const uint8_t* data, size_t length, uint64_t counts[10])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!test_hooks_enabled() || !data || !counts) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    ParseStatus ps = parse_jpeg(data, length, &f);
    if (ps != kParseOk) return status_from_parse(ps);
    if (gpu_progressive_eligible(f) || !gpu_entropy_eligible(f)) return HIPJPEG_STATUS_UNSUPPORTED;
    std::vector<int16_t> coef(f.total_blocks() * 64);
    int16_t* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t off = 0;
    for (int c = 0; c < f.ncomp; c++) {
        ptr[c] = coef.data() + off;
        off += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64;
    }
    SyncScheduleCounts schedules[2];
    const int rc = emulate_gpu_entropy(data, length, f, ptr, nullptr, schedules);
    for (int s = 0; s < 2; s++) {
        for (int q = 0; q < 4; q++) counts[5 * s + q] = schedules[s].phase[q];
        counts[5 * s + 4] = schedules[s].tail;
    }
    if (rc == 5) return HIPJPEG_STATUS_INTERNAL_ERROR;
    return rc == 0 ? HIPJPEG_STATUS_SUCCESS : (rc == 2 ? HIPJPEG_STATUS_TRUNCATED : HIPJPEG_STATUS_CORRUPT);
    });
}

hipjpegStatus_t hipjpegEntropyDecodeGpuIntervalAlgorithmHost(const uint8_t* data, size_t length, int16_t* coef, size_t coef_capacity_bytes,
                                                             uint64_t comp_offsets[4])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!data || !coef) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    ParseStatus ps = parse_jpeg(data, length, &f);
    if (ps != kParseOk) return status_from_parse(ps);
    if (!gpu_progressive_interval_eligible(f)) return HIPJPEG_STATUS_UNSUPPORTED;
    if (f.total_blocks() * 128 > coef_capacity_bytes) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    int16_t* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t off = 0;
    for (int c = 0; c < f.ncomp; c++) {
        ptr[c] = coef + off;
        if (comp_offsets) comp_offsets[c] = off;
        off += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64;
    }
    return emulate_gpu_progressive_intervals(data, length, f, ptr) == 0 ? HIPJPEG_STATUS_SUCCESS : HIPJPEG_STATUS_CORRUPT;
    });
}

hipjpegStatus_t hipjpegCreate(hipjpegHandle_t* handle, int device_id, int num_host_threads)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    *handle = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return HIPJPEG_STATUS_NO_DEVICE;
    if (device_id < 0 || device_id >= count) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    hipjpegHandle* h = new (std::nothrow) hipjpegHandle();
    if (!h) return HIPJPEG_STATUS_ALLOC_FAILED;
    h->device_id = device_id;
    h->pool.reset(new ForkJoinPool(num_host_threads));
    for (auto& b : h->batches) b.reset(new DecodeBatch(device_id, &h->hooks));
    h->encode.reset(new EncodeBatch(device_id, &h->hooks));
    h->encode_view = h->encode.get();
    *handle = h;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDestroy(hipjpegHandle_t handle)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    (void)hipSetDevice(handle->device_id);
    if (handle->copy_stream) (void)hipStreamDestroy(handle->copy_stream);
    if (handle->entropy_stream) (void)hipStreamDestroy(handle->entropy_stream);
    for (hipStream_t ps : handle->page_entropy_stream)
        if (ps) (void)hipStreamDestroy(ps);
    for (auto& pg : handle->encode_pages) {
        if (pg.result.valid()) {
            try {
                (void)pg.result.get();
            } catch (...) {
            }
        }
        pg.batch.reset();
        if (pg.ready) (void)hipEventDestroy(pg.ready);
        if (pg.stream) (void)hipStreamDestroy(pg.stream);
    }
    delete handle;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatchHost(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                       const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags,
                                       hipjpegStatus_t* statuses)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->current = (handle->current + 1) % handle->pages;
    handle->settled = -1;
    DecodeBatch& b = handle->cur();
    static const bool timing = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;  // debug aid: host-stage phase times on stderr
    const auto t0 = std::chrono::steady_clock::now();
    const bool geometry = !handle->transforms.empty(), scaled = !handle->scales.empty();
    if ((geometry && (int)handle->transforms.size() != batch_size) || (scaled && (int)handle->scales.size() != batch_size)) {
        handle->transforms.clear();
        handle->scales.clear();
        return HIPJPEG_STATUS_INVALID_ARGUMENT;
    }
    hipjpegStatus_t st = b.plan(data, lengths, batch_size, outputs, format, flags, statuses, nullptr, handle->pool.get(),
                                geometry ? handle->transforms.data() : nullptr, scaled ? handle->scales.data() : nullptr);
    handle->transforms.clear();
    handle->scales.clear();
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    const auto t1 = std::chrono::steady_clock::now();
    handle->pool->parallel_for(batch_size, [&](int i, int) { b.entropy_stage(i); });
    const auto t2 = std::chrono::steady_clock::now();
    b.finalize(statuses);
    if (timing) {
        const auto t3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[hipjpeg] host stage: plan %.2f ms, entropy/staging %.2f ms, finalize %.2f ms (%d threads)\n", ms(t0, t1), ms(t1, t2), ms(t2, t3),
                handle->pool->num_threads());
    }
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatchSetTransforms(hipjpegHandle_t handle, const hipjpegTransform_t* transforms, int batch_size)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (transforms)
        handle->transforms.assign(transforms, transforms + batch_size);
    else
        handle->transforms.clear();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatchSetScales(hipjpegHandle_t handle, const int32_t* scale_denoms, int batch_size)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (scale_denoms)
        handle->scales.assign(scale_denoms, scale_denoms + batch_size);
    else
        handle->scales.clear();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegGetScaledImageSize(int32_t width, int32_t height, int32_t scale_denom, int32_t* scaled_width, int32_t* scaled_height)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (width <= 0 || height <= 0 || !scaled_width || !scaled_height) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (scale_denom != 1 && scale_denom != 2 && scale_denom != 4 && scale_denom != 8) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // jdmaster.c jpeg_calc_output_dimensions: ceil(extent * k / 8) with k = 8 / denominator
    const int64_t k = 8 / scale_denom;
    *scaled_width = (int32_t)(((int64_t)width * k + 7) / 8);
    *scaled_height = (int32_t)(((int64_t)height * k + 7) / 8);
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatchTransfer(hipjpegHandle_t handle, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return handle->cur().transfer(stream);
    });
}

hipjpegStatus_t hipjpegDecodeBatchDevice(hipjpegHandle_t handle, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return handle->cur().launch(stream);
    });
}

hipjpegStatus_t hipjpegDecodeBatchDeviceKernel(hipjpegHandle_t handle, int which, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || which < 0 || which > 6 || which == 5) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return handle->cur().launch(stream, which);
    });
}

hipjpegStatus_t hipjpegDecodeBatchStats(hipjpegHandle_t handle, int32_t num_units[3], uint64_t* coef_bytes, uint64_t* output_bytes)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->cur().stats(num_units, coef_bytes, output_bytes);
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                   const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags, hipjpegStatus_t* statuses,
                                   void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    hipjpegStatus_t st = hipjpegDecodeBatchHost(handle, data, lengths, batch_size, outputs, format, flags, statuses);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = hipjpegDecodeBatchTransfer(handle, stream)) != HIPJPEG_STATUS_SUCCESS) return st;
    st = hipjpegDecodeBatchDevice(handle, stream);
    // the GPU entropy stage may have found problems the host never looked at: wait for its verdicts (batches without
    // GPU-decoded streams return without waiting)
    if (st == HIPJPEG_STATUS_SUCCESS) st = handle->cur().resolve(stream);
    if (statuses)
        for (int i = 0; i < batch_size; i++) statuses[i] = handle->cur().image(i).status;
    return st;
    });
}

hipjpegStatus_t hipjpegDecodeBatchSubmit(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                         const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (handle->num_submitted >= handle->pages) return HIPJPEG_STATUS_INVALID_ARGUMENT;  // every page in flight: Wait first
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    if (!handle->copy_stream && hipStreamCreateWithFlags(&handle->copy_stream, hipStreamNonBlocking) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    if (!handle->entropy_stream && hipStreamCreateWithFlags(&handle->entropy_stream, hipStreamNonBlocking) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    hipjpegStatus_t st = hipjpegDecodeBatchHost(handle, data, lengths, batch_size, outputs, format, flags, nullptr);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    DecodeBatch& b = handle->cur();
    // From here on the page may have device work queued (its H2D copy, entropy kernels, pixel kernels) that reads the page's pinned and
    // device arenas.  If a later step fails or throws, the page is not recorded as submitted and would be reused `pages` Submits later
    // without anybody having waited for that work: drain the streams it may sit on before the error leaves.
    hipStream_t es = handle->entropy_stream;
    auto drain = [&]() {
        if (hipSetDevice(handle->device_id) != hipSuccess) return;
        (void)hipStreamSynchronize(handle->copy_stream);
        if (handle->entropy_stream) (void)hipStreamSynchronize(handle->entropy_stream);
        if (es && es != handle->entropy_stream) (void)hipStreamSynchronize(es);
        (void)hipStreamSynchronize((hipStream_t)stream);
    };
    try {
        if ((st = b.transfer(handle->copy_stream, true)) == HIPJPEG_STATUS_SUCCESS) {
            if (b.has_progressive()) {
                hipStream_t& ps = handle->page_entropy_stream[handle->current];
                if (!ps && hipStreamCreateWithFlags(&ps, hipStreamNonBlocking) != hipSuccess) st = HIPJPEG_STATUS_HIP_ERROR;
                es = ps;
            }
            if (st == HIPJPEG_STATUS_SUCCESS) st = b.launch(stream, -1, es);
        }
    } catch (...) {
        drain();
        throw;
    }
    if (st != HIPJPEG_STATUS_SUCCESS) {
        drain();
        return st;
    }
    handle->submitted[handle->num_submitted] = handle->current;
    handle->submitted_stream[handle->num_submitted] = stream;
    handle->num_submitted++;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegSetHybridHuffmanThreshold(hipjpegHandle_t handle, uint64_t pixels)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    for (auto& b : handle->batches)
        if (b) b->set_gpu_entropy_threshold(pixels);
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegSetAllocators(hipjpegHandle_t handle, const hipjpegAllocators_t* allocators)
{
    return guarded([&]() -> hipjpegStatus_t {
    // every Buffer of the handle (decode pages, encode batch and pages, lossless pages) points at handle->hooks and marks it used at
    // its first allocation: until then no memory exists that another allocator would have to take back
    if (!handle || !allocators || handle->hooks.used.load()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    MemoryHooks& k = handle->hooks;
    const bool device = allocators->device_malloc && allocators->device_free;
    const bool pinned = allocators->pinned_malloc && allocators->pinned_free;
    k.device_malloc = device ? allocators->device_malloc : nullptr;
    k.device_free = device ? allocators->device_free : nullptr;
    k.device_ctx = device ? allocators->device_ctx : nullptr;
    k.pinned_malloc = pinned ? allocators->pinned_malloc : nullptr;
    k.pinned_free = pinned ? allocators->pinned_free : nullptr;
    k.pinned_ctx = pinned ? allocators->pinned_ctx : nullptr;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegSetPipelineDepth(hipjpegHandle_t handle, int depth)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || depth < 1 || depth > hipjpegHandle::kMaxPages || handle->num_submitted != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->pages = depth;
    handle->current = 0;
    handle->settled = -1;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatchWait(hipjpegHandle_t handle, hipjpegStatus_t* statuses, int batch_size)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || handle->num_submitted == 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    DecodeBatch& b = *handle->batches[handle->submitted[0]];
    handle->settled = handle->submitted[0];
    void* stream = handle->submitted_stream[0];
    if (statuses && batch_size != b.size()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    for (int k = 1; k < handle->num_submitted; k++) {
        handle->submitted[k - 1] = handle->submitted[k];
        handle->submitted_stream[k - 1] = handle->submitted_stream[k];
    }
    handle->num_submitted--;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    hipjpegStatus_t st = b.wait_done();
    if (st == HIPJPEG_STATUS_SUCCESS) st = b.resolve(stream);
    if (statuses)
        for (int i = 0; i < batch_size; i++) statuses[i] = b.image(i).status;
    return st;
    });
}

hipjpegStatus_t hipjpegDecodeBatchGetStatuses(hipjpegHandle_t handle, hipjpegStatus_t* statuses, int batch_size)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !statuses || batch_size != handle->cur().size()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    hipjpegStatus_t st = handle->cur().resolve(handle->cur().last_stream());
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    for (int i = 0; i < batch_size; i++) statuses[i] = handle->cur().image(i).status;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeBatchEntropyStats(hipjpegHandle_t handle, int32_t* gpu_images, int32_t* sync_launches, uint64_t* stream_bytes)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (gpu_images) *gpu_images = handle->cur().gpu_entropy_images();
    if (sync_launches) *sync_launches = handle->cur().last_sync_launches();
    if (stream_bytes) *stream_bytes = handle->cur().stream_bytes();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

int32_t hipjpegDecodeBatchZeroCopyImages(hipjpegHandle_t handle) { return handle ? handle->cur().zero_copy_images() : -1; }

int32_t hipjpegDecodeBatchIntervalImages(hipjpegHandle_t handle) { return handle ? handle->cur().interval_images() : -1; }

int32_t hipjpegDecodeBatchIntervalTakeovers(hipjpegHandle_t handle)
{
    // the batch the last Wait settled, if no batch has been planned since; else the current page's
    if (!handle) return -1;
    return handle->batches[handle->settled >= 0 ? handle->settled : handle->current]->interval_takeover_images();
}

hipjpegStatus_t hipjpegDecodeBatchTransferStats(hipjpegHandle_t handle, uint64_t* h2d_bytes, int32_t* sparse_images)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (h2d_bytes) *h2d_bytes = handle->cur().h2d_bytes();
    if (sparse_images) *sparse_images = handle->cur().sparse_images();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

int32_t hipjpegTestScanChunkDrops(const uint8_t* data, size_t length, int scan_index, uint32_t* drops, int32_t capacity)
{
    int32_t result = -1;
    if (!test_hooks_enabled()) return result;
    (void)guarded([&]() -> hipjpegStatus_t {
        hipjpeg::FrameInfo f;
        if (hipjpeg::parse_jpeg(data, length, &f) != hipjpeg::kParseOk || scan_index < 0 || scan_index >= (int)f.scans.size()) return HIPJPEG_STATUS_BAD_JPEG;
        const auto& d = f.scans[scan_index].chunk_drops;
        for (int32_t c = 0; c < (int32_t)d.size() && c < capacity && drops; c++) drops[c] = d[c];
        result = (int32_t)d.size();
        return HIPJPEG_STATUS_SUCCESS;
    });
    return result;
}

int32_t hipjpegTestPairSteps(const uint8_t bits[16], const uint8_t* vals, int32_t nvals, uint32_t* steps)
{
    int32_t result = -1;
    if (!test_hooks_enabled() || !bits || !vals || !steps || nvals < 0 || nvals > 256) return result;
    (void)guarded([&]() -> hipjpegStatus_t {
        hipjpeg::HuffSpec spec;
        for (int l = 1; l <= 16; l++) spec.bits[l] = bits[l - 1];
        for (int32_t i = 0; i < nvals; i++) spec.vals[i] = vals[i];
        spec.present = true;
        if (hipjpeg::pair_table_steps(spec, steps)) result = 0;
        return HIPJPEG_STATUS_SUCCESS;
    });
    return result;
}

int32_t hipjpegTestHostFallbacks(hipjpegHandle_t handle)
{
    // the batch the last Wait settled, if no batch has been planned since; else the current page's
    if (!handle || !test_hooks_enabled()) return -1;
    return handle->batches[handle->settled >= 0 ? handle->settled : handle->current]->host_fallback_images();
}

hipjpegStatus_t hipjpegTestKernelFlavours(hipjpegHandle_t handle, int32_t plane_units[1], int32_t luma_units[3])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !plane_units || !luma_units || !test_hooks_enabled()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->cur().flavour_units(plane_units, luma_units);
    return HIPJPEG_STATUS_SUCCESS;
    });
}

int32_t hipjpegTestFusedUnits(hipjpegHandle_t handle) { return handle && test_hooks_enabled() ? handle->cur().fused_units() : -1; }

// ---------------------------------------------------------------- encode
hipjpegStatus_t hipjpegEncodeBatchDevice(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params,
                                         int batch_size, hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->encode_view = handle->encode.get();
    return handle->encode->device_stage(inputs, params, batch_size, statuses, stream);
    });
}

hipjpegStatus_t hipjpegEncodeBatchRelaunch(hipjpegHandle_t handle, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return handle->encode->relaunch(stream);
    });
}

hipjpegStatus_t hipjpegEncodeBatchEntropy(hipjpegHandle_t handle, unsigned flags, hipjpegStatus_t* statuses)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    EncodeBatch& b = *handle->encode;
    const hipjpegStatus_t st = b.route_entropy((flags & HIPJPEG_FLAG_GPU_HUFFMAN) != 0, (flags & HIPJPEG_FLAG_GPU_RESTART_INTERVALS) != 0,
                                  (flags & HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART) != 0);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    if (b.host_images()) handle->pool->parallel_for(b.size(), [&](int i, int) { b.entropy_stage(i); });
    if (statuses)
        for (int i = 0; i < b.size(); i++) statuses[i] = b.image(i).status;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeBatchHost(hipjpegHandle_t handle, hipjpegStatus_t* statuses) { return hipjpegEncodeBatchEntropy(handle, 0u, statuses); }

hipjpegStatus_t hipjpegEncodeBatch(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params,
                                   int batch_size, hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    hipjpegStatus_t st = hipjpegEncodeBatchDevice(handle, inputs, params, batch_size, statuses, stream);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    return hipjpegEncodeBatchHost(handle, statuses);
    });
}

hipjpegStatus_t hipjpegEncodeBatchSubmit(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params, int batch_size,
                                         unsigned flags, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0 || (batch_size > 0 && (!inputs || !params))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (handle->encode_in_flight >= hipjpegHandle::kEncodePages) return HIPJPEG_STATUS_INVALID_ARGUMENT;  // every page busy: Wait first
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    hipjpegHandle::EncodePage& pg = handle->encode_pages[handle->encode_next];
    if (!pg.batch) {
        pg.batch.reset(new EncodeBatch(handle->device_id, &handle->hooks));
        if (hipStreamCreateWithFlags(&pg.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&pg.ready, hipEventDisableTiming) != hipSuccess)
            return HIPJPEG_STATUS_HIP_ERROR;
    }
    pg.inputs.assign(inputs, inputs + batch_size);
    pg.params.assign(params, params + batch_size);
    // the page's stream must see the producer's pixels
    if (hipEventRecord(pg.ready, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(pg.stream, pg.ready, 0) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    const int device = handle->device_id;
    hipjpegHandle::EncodePage* page = &pg;
    pg.result = std::async(std::launch::async, [page, device, flags]() -> hipjpegStatus_t {
        if (hipSetDevice(device) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
        EncodeBatch& b = *page->batch;
        hipjpegStatus_t st = b.device_stage(page->inputs.data(), page->params.data(), (int)page->inputs.size(), nullptr, page->stream);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        if ((st = b.route_entropy((flags & HIPJPEG_FLAG_GPU_HUFFMAN) != 0, (flags & HIPJPEG_FLAG_GPU_RESTART_INTERVALS) != 0,
                                  (flags & HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART) != 0)) != HIPJPEG_STATUS_SUCCESS) return st;
        for (int i = 0; i < b.size(); i++) b.entropy_stage(i);
        return HIPJPEG_STATUS_SUCCESS;
    });
    handle->encode_next = (handle->encode_next + 1) % hipjpegHandle::kEncodePages;
    handle->encode_in_flight++;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeBatchWait(hipjpegHandle_t handle, hipjpegStatus_t* statuses, int batch_size)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || handle->encode_in_flight == 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    hipjpegHandle::EncodePage& pg = handle->encode_pages[handle->encode_oldest];
    handle->encode_oldest = (handle->encode_oldest + 1) % hipjpegHandle::kEncodePages;
    handle->encode_in_flight--;
    const hipjpegStatus_t st = pg.result.get();
    handle->encode_view = pg.batch.get();
    if (statuses) {
        if (batch_size != pg.batch->size()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        for (int i = 0; i < batch_size; i++) statuses[i] = pg.batch->image(i).status;
    }
    return st;
    });
}

hipjpegStatus_t hipjpegEncodeGetBitstream(hipjpegHandle_t handle, int index, const uint8_t** data, size_t* length)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !data || !length || index < 0 || index >= handle->encode_view->size()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    PlannedEncode& im = handle->encode_view->image(index);
    if (im.status != HIPJPEG_STATUS_SUCCESS) return im.status;
    *data = im.file();
    *length = im.file_size();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeGetCoefficients(hipjpegHandle_t handle, int index, int component, const int16_t** coef, int32_t grid[4])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !coef || !grid || index < 0 || index >= handle->encode_view->size()) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    PlannedEncode& im = handle->encode_view->image(index);
    if (im.status != HIPJPEG_STATUS_SUCCESS) return im.status;
    if (component < 0 || component >= im.geom.ncomp) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    hipjpegStatus_t st = handle->encode_view->fetch_coefficients();
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    *coef = handle->encode_view->host_coef(index, component);
    grid[0] = im.geom.blocks_w[component];
    grid[1] = im.geom.blocks_h[component];
    grid[2] = im.geom.real_w[component];
    grid[3] = im.geom.real_h[component];
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeBatchStats(hipjpegHandle_t handle, int32_t* num_units, uint64_t* pixel_bytes, uint64_t* coef_bytes)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (num_units) *num_units = handle->encode_view->num_units();
    if (pixel_bytes) *pixel_bytes = handle->encode_view->pixel_bytes();
    if (coef_bytes) *coef_bytes = handle->encode_view->coef_bytes();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

int32_t hipjpegEncodeBatchGpuEntropyImages(hipjpegHandle_t handle)
{
    return handle && handle->encode_view ? (int32_t)handle->encode_view->gpu_entropy_images() : -1;
}

hipjpegStatus_t hipjpegEncodeFromCoefficientsHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params, const int16_t* const coef[3],
                                                  uint8_t* out, size_t capacity, size_t* length)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!params || !coef || !length || width < 1 || height < 1 || width > 65535 || height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    EncodeGeometry g;
    uint16_t ql[64], qc[64];
    hipjpegStatus_t st = picture_setup(*params, width, height, &g, ql, qc);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    for (int c = 0; c < g.ncomp; c++)
        if (!coef[c]) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    std::vector<uint8_t> bytes;
    encode_jfif(g, ql, qc, coef, entropy_options(*params), &bytes);
    *length = bytes.size();
    if (!out || capacity < bytes.size()) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    memcpy(out, bytes.data(), bytes.size());
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeFromCoefficientsGpuAlgorithmHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                              const int16_t* const coef[3], uint8_t* out, size_t capacity, size_t* length)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!params || !coef || !length || width < 1 || height < 1 || width > 65535 || height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    EncodeGeometry g;
    uint16_t ql[64], qc[64];
    hipjpegStatus_t st = picture_setup(*params, width, height, &g, ql, qc);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    for (int c = 0; c < g.ncomp; c++)
        if (!coef[c]) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (!params->progressive || params->restart_interval != 0) return HIPJPEG_STATUS_UNSUPPORTED;  // what the GPU coder's progressive path takes
    std::vector<uint8_t> bytes;
    encode_progressive_gpu_algorithm(g, ql, qc, coef, 0, &bytes);
    *length = bytes.size();
    if (!out || capacity < bytes.size()) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    memcpy(out, bytes.data(), bytes.size());
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeProgressiveGpuAlgorithmHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                         const int16_t* const coef[3], uint8_t* out, size_t capacity, size_t* length)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!params || !coef || !length || width < 1 || height < 1 || width > 65535 || height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    EncodeGeometry g;
    uint16_t ql[64], qc[64];
    hipjpegStatus_t st = picture_setup(*params, width, height, &g, ql, qc);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    for (int c = 0; c < g.ncomp; c++)
        if (!coef[c]) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (params->restart_interval < 0 || params->restart_interval > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (!params->progressive) return HIPJPEG_STATUS_UNSUPPORTED;  // the progressive plan of the GPU coder
    std::vector<uint8_t> bytes;
    encode_progressive_gpu_algorithm(g, ql, qc, coef, params->restart_interval, &bytes);
    *length = bytes.size();
    if (!out || capacity < bytes.size()) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    memcpy(out, bytes.data(), bytes.size());
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeBaselineGpuAlgorithmHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params, const int16_t* const coef[3],
                                                      uint8_t* out, size_t capacity, size_t* length)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!params || !coef || !length || width < 1 || height < 1 || width > 65535 || height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    EncodeGeometry g;
    uint16_t ql[64], qc[64];
    hipjpegStatus_t st = picture_setup(*params, width, height, &g, ql, qc);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    for (int c = 0; c < g.ncomp; c++)
        if (!coef[c]) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (params->restart_interval < 0 || params->restart_interval > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (params->progressive) return HIPJPEG_STATUS_UNSUPPORTED;  // the baseline plan of the GPU coder
    std::vector<uint8_t> bytes;
    encode_baseline_gpu_algorithm(g, ql, qc, coef, params->restart_interval, params->optimized_huffman != 0, &bytes);
    *length = bytes.size();
    if (!out || capacity < bytes.size()) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
    memcpy(out, bytes.data(), bytes.size());
    return HIPJPEG_STATUS_SUCCESS;
    });
}

// ---------------------------------------------------------------- lossless transcode
// (hipjpegTranscodeHost / hipjpegTranscodeHostRegion: transcode_core.cpp, with the rest of the host route)
hipjpegStatus_t hipjpegTranscodeBatchSetRegions(hipjpegHandle_t handle, const hipjpegTranscodeRegion_t* regions, int batch_size)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->transcode_regions_set = regions != nullptr;
    if (regions)
        handle->transcode_regions.assign(regions, regions + batch_size);
    else
        handle->transcode_regions.clear();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegTranscodeBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                      const hipjpegTranscodeParams_t* params, unsigned flags, hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (handle && handle->drop_pending_scales()) return HIPJPEG_STATUS_INVALID_ARGUMENT;  // no scaled transcode
    if (!handle || batch_size < 0 || (batch_size > 0 && (!data || !lengths || !params))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // the call takes a decode page and the encode batch for itself: nothing submitted may still be using either
    if (handle->num_submitted != 0 || handle->encode_in_flight != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    handle->transcode_gpu_decoded = handle->transcode_gpu_coded = handle->transcode_blocks = 0;
    handle->settled = -1;  // a batch is planned on the current page
    // the regions belong to this batch alone, whatever becomes of it
    std::vector<hipjpegTranscodeRegion_t> regions;
    regions.swap(handle->transcode_regions);
    const bool have_regions = handle->transcode_regions_set;
    handle->transcode_regions_set = false;
    if (have_regions && (int)regions.size() != batch_size) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // (the call blocks and nothing is submitted: the current decode page is free, and staying on it keeps its arenas warm)
    DecodeBatch& d = handle->cur();
    // decode side: the headers first
    hipjpegStatus_t st = d.plan_coefficients(data, lengths, batch_size, flags, nullptr, handle->pool.get(), params);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    // the pictures by geometry and the source's tables, as transcode_host derives them: drop chroma -> crop -> turn.  What the header
    // settles is settled before anything is decoded: a refused request costs no entropy decoding and reports what the host route reports.
    std::vector<CoefficientPicture> pics((size_t)batch_size);
    for (int i = 0; i < batch_size; i++) {
        CoefficientPicture& p = pics[(size_t)i];
        if (transcode_params_ok(params[i]) != HIPJPEG_STATUS_SUCCESS) d.reject(i, HIPJPEG_STATUS_INVALID_ARGUMENT);
        if ((p.status = d.image(i).status) != HIPJPEG_STATUS_SUCCESS) continue;
        TranscodePicture source, cropped;
        const int32_t field = params[i].orientation;
        const int orientation = transcode_orientation(params[i], data[i], lengths[i]);
        p.status = transcode_picture(d.image(i).frame, (field & HIPJPEG_TRANSCODE_GRAYSCALE) != 0, &source);
        if (p.status == HIPJPEG_STATUS_SUCCESS)
            p.status = transcode_crop(source, have_regions ? &regions[(size_t)i] : nullptr, (field & HIPJPEG_TRANSCODE_CROP_EXPAND) != 0, &cropped, &p.origin);
        if (p.status == HIPJPEG_STATUS_SUCCESS) p.status = transcode_turn(cropped, orientation, (field & HIPJPEG_TRANSCODE_TRIM) != 0, &p.picture, &p.turn);
        if (p.status != HIPJPEG_STATUS_SUCCESS) {
            d.reject(i, p.status);
            continue;
        }
        transcode_markers(params[i], orientation, data[i], lengths[i], &p.markers);
        p.params.restart_interval = params[i].restart_interval;
        p.params.optimized_huffman = params[i].optimized_huffman;
        p.params.progressive = params[i].progressive;
    }
    // decode side: the entropy stage alone, verdicts settled (launch 3 = entropy kernels + resolve) before anything is coded
    handle->pool->parallel_for(batch_size, [&](int i, int) { d.entropy_stage(i); });
    d.finalize(nullptr);
    if ((st = d.transfer(stream)) != HIPJPEG_STATUS_SUCCESS || (st = d.launch(stream, 3)) != HIPJPEG_STATUS_SUCCESS) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // nothing of this batch stays queued behind an error
        return st;
    }
    // encode side: the coefficient area filled by the relayout kernels; what the decoder found wrong with an image stands
    for (int i = 0; i < batch_size; i++)
        if (pics[(size_t)i].status == HIPJPEG_STATUS_SUCCESS) pics[(size_t)i].status = d.image(i).status;
    EncodeBatch& e = *handle->encode;
    handle->encode_view = &e;
    if ((st = e.coefficient_stage(pics.data(), batch_size, d.device_descriptors(), stream)) != HIPJPEG_STATUS_SUCCESS) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        return st;
    }
    if ((st = e.route_entropy((flags & HIPJPEG_FLAG_GPU_HUFFMAN) != 0, (flags & HIPJPEG_FLAG_GPU_RESTART_INTERVALS) != 0,
                                  (flags & HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART) != 0)) != HIPJPEG_STATUS_SUCCESS) return st;
    if (e.host_images()) handle->pool->parallel_for(e.size(), [&](int i, int) { e.entropy_stage(i); });
    if (statuses)
        for (int i = 0; i < batch_size; i++) statuses[i] = e.image(i).status;
    handle->transcode_gpu_decoded = d.gpu_entropy_images();
    handle->transcode_gpu_coded = (int32_t)e.gpu_entropy_images();
    handle->transcode_blocks = (int32_t)e.relayout_blocks();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegTranscodeBatchStats(hipjpegHandle_t handle, int32_t* gpu_decoded_images, int32_t* gpu_coded_images, int32_t* relayout_blocks)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (gpu_decoded_images) *gpu_decoded_images = handle->transcode_gpu_decoded;
    if (gpu_coded_images) *gpu_coded_images = handle->transcode_gpu_coded;
    if (relayout_blocks) *relayout_blocks = handle->transcode_blocks;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

// ---------------------------------------------------------------- coefficient tensors
// (hipjpegGetCoefficientInfo / hipjpegDecodeCoefficientsHost / hipjpegEncodeCoefficientsHost: coefficients_core.cpp, with the rules)
hipjpegStatus_t hipjpegDecodeCoefficientsBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                               const hipjpegCoefficientPlanes_t* planes, unsigned flags, hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (handle && handle->drop_pending_scales()) return HIPJPEG_STATUS_INVALID_ARGUMENT;  // coefficients have no scale
    if (!handle || batch_size < 0 || (batch_size > 0 && (!data || !lengths || !planes))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // the call takes the current decode page for itself: nothing submitted may still be using it
    if (handle->num_submitted != 0 || handle->encode_in_flight != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    handle->coefficients_gpu_decoded = 0;
    handle->coefficients_blocks = 0;
    handle->settled = -1;  // a batch is planned on the current page
    DecodeBatch& d = handle->cur();
    hipjpegStatus_t st = d.plan_coefficients(data, lengths, batch_size, flags, nullptr, handle->pool.get(), nullptr, /*any_frame=*/true);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    // what the header settles about the caller's planes is settled before anything is decoded
    for (int i = 0; i < batch_size; i++) {
        if (d.image(i).status != HIPJPEG_STATUS_SUCCESS) continue;
        hipjpegCoefficientInfo_t info;
        coefficient_info(d.image(i).frame, &info);
        d.reject(i, coefficient_planes_ok(info.num_components, info.blocks_w, planes[i]));
    }
    // the entropy stage alone, verdicts settled (launch 3 = entropy kernels + resolve): a failing image writes nothing into its planes
    handle->pool->parallel_for(batch_size, [&](int i, int) { d.entropy_stage(i); });
    d.finalize(nullptr);
    if ((st = d.transfer(stream)) != HIPJPEG_STATUS_SUCCESS || (st = d.launch(stream, 3)) != HIPJPEG_STATUS_SUCCESS ||
        (st = d.export_coefficients(planes, stream)) != HIPJPEG_STATUS_SUCCESS) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // nothing of this batch stays queued behind an error
        return st;
    }
    if (statuses)
        for (int i = 0; i < batch_size; i++) statuses[i] = d.image(i).status;
    handle->coefficients_gpu_decoded = d.gpu_entropy_images();
    handle->coefficients_blocks = (int64_t)d.exported_blocks();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegEncodeCoefficientsBatch(hipjpegHandle_t handle, const hipjpegCoefficientInfo_t* infos, const hipjpegCoefficientPlanes_t* planes,
                                               const hipjpegTranscodeParams_t* params, int batch_size, unsigned flags, hipjpegStatus_t* statuses,
                                               void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0 || (batch_size > 0 && (!infos || !planes || !params))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // the call takes the encode batch for itself
    if (handle->num_submitted != 0 || handle->encode_in_flight != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    handle->coefficients_gpu_coded = 0;
    handle->coefficients_blocks = 0;
    std::vector<CoefficientPicture> pics((size_t)batch_size);
    for (int i = 0; i < batch_size; i++) {
        CoefficientPicture& p = pics[(size_t)i];
        p.status = coefficient_picture(infos[i], planes[i], params[i], &p.picture);
        p.params.restart_interval = params[i].restart_interval;
        p.params.optimized_huffman = params[i].optimized_huffman;
        p.params.progressive = params[i].progressive;
    }
    EncodeBatch& e = *handle->encode;
    handle->encode_view = &e;
    hipjpegStatus_t st = e.import_stage(pics.data(), planes, batch_size, stream);
    if (st != HIPJPEG_STATUS_SUCCESS) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        return st;
    }
    if ((st = e.route_entropy((flags & HIPJPEG_FLAG_GPU_HUFFMAN) != 0, (flags & HIPJPEG_FLAG_GPU_RESTART_INTERVALS) != 0,
                                  (flags & HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART) != 0)) != HIPJPEG_STATUS_SUCCESS) return st;
    if (e.host_images()) handle->pool->parallel_for(e.size(), [&](int i, int) { e.entropy_stage(i); });
    if (statuses)
        for (int i = 0; i < batch_size; i++) statuses[i] = e.image(i).status;
    handle->coefficients_gpu_coded = (int32_t)e.gpu_entropy_images();
    handle->coefficients_blocks = (int64_t)e.relayout_blocks();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegCoefficientsToPixelsBatch(hipjpegHandle_t handle, const hipjpegCoefficientInfo_t* infos, const hipjpegCoefficientPlanes_t* planes,
                                                 int batch_size, const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags,
                                                 hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // the transforms belong to this batch alone, whatever becomes of it
    std::vector<hipjpegTransform_t> transforms;
    transforms.swap(handle->transforms);
    if (handle->drop_pending_scales()) return HIPJPEG_STATUS_INVALID_ARGUMENT;  // scaling from coefficient tensors: not in this version
    if (batch_size < 0 || (batch_size > 0 && (!infos || !planes || !outputs))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // the call takes the current decode page for itself: nothing submitted may still be using it
    if (handle->num_submitted != 0 || handle->encode_in_flight != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (!transforms.empty() && (int)transforms.size() != batch_size) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    handle->coefficients_blocks = 0;
    DecodeBatch& d = handle->cur();
    hipjpegStatus_t st = d.plan_tensors(infos, planes, batch_size, outputs, format, flags, nullptr, handle->pool.get(),
                                        transforms.empty() ? nullptr : transforms.data());
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    // no entropy stage: the statuses are final here; then descriptors and units, the relayout kernel, the pixel kernels
    d.finalize(statuses);
    if ((st = d.transfer(stream)) != HIPJPEG_STATUS_SUCCESS || (st = d.import_tensors(stream)) != HIPJPEG_STATUS_SUCCESS ||
        (st = d.launch(stream)) != HIPJPEG_STATUS_SUCCESS) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // nothing of this batch stays queued behind an error
        return st;
    }
    handle->coefficients_blocks = (int64_t)d.imported_blocks();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegPixelsToCoefficientsBatch(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params,
                                                 int batch_size, const hipjpegCoefficientPlanes_t* planes, hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0 || (batch_size > 0 && (!inputs || !params || !planes))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // the call takes the encode batch for itself
    if (handle->num_submitted != 0 || handle->encode_in_flight != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    handle->coefficients_blocks = 0;
    EncodeBatch& e = *handle->encode;
    handle->encode_view = &e;
    hipjpegStatus_t st = e.device_stage(inputs, params, batch_size, statuses, stream);
    if (st == HIPJPEG_STATUS_SUCCESS) st = e.planes_stage(planes, statuses, stream);
    if (st != HIPJPEG_STATUS_SUCCESS) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // nothing of this batch stays queued behind an error
        return st;
    }
    handle->coefficients_blocks = (int64_t)e.planes_blocks();
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegCoefficientsBatchStats(hipjpegHandle_t handle, int32_t* gpu_decoded_images, int32_t* gpu_coded_images, int64_t* moved_blocks)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (gpu_decoded_images) *gpu_decoded_images = handle->coefficients_gpu_decoded;
    if (gpu_coded_images) *gpu_coded_images = handle->coefficients_gpu_coded;
    if (moved_blocks) *moved_blocks = handle->coefficients_blocks;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

// ---------------------------------------------------------------- lossless JPEG
// (hipjpegGetLosslessInfo / hipjpegDecodeLosslessHost / hipjpegLosslessReconstructAlgorithmHost: lossless_core.cpp, with the rules)
hipjpegStatus_t hipjpegDecodeLosslessBatchFlags(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                const hipjpegLosslessOutput_t* outputs, hipjpegStatus_t* statuses, unsigned int flags, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0 || (batch_size > 0 && (!data || !lengths || !outputs))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    if (!handle->lossless) handle->lossless.reset(new LosslessBatch(handle->device_id, &handle->hooks));
    return handle->lossless->decode(data, lengths, batch_size, outputs, statuses, flags, handle->pool.get(), (hipStream_t)stream);
    });
}

hipjpegStatus_t hipjpegDecodeLosslessBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                           const hipjpegLosslessOutput_t* outputs, hipjpegStatus_t* statuses, void* stream)
{
    return hipjpegDecodeLosslessBatchFlags(handle, data, lengths, batch_size, outputs, statuses, 0u, stream);
}

hipjpegStatus_t hipjpegDecodeLosslessBatchEntropyStats(hipjpegHandle_t handle, int32_t* gpu_images, int32_t* host_fallback_images, int32_t* ripple_launches)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (gpu_images) *gpu_images = handle->lossless ? handle->lossless->gpu_images() : 0;
    if (host_fallback_images) *host_fallback_images = handle->lossless ? handle->lossless->host_fallback_images() : 0;
    if (ripple_launches) *ripple_launches = handle->lossless ? handle->lossless->ripple_launches() : 0;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

hipjpegStatus_t hipjpegDecodeLosslessBatchDeviceKernel(hipjpegHandle_t handle, int which, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !handle->lossless) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    return handle->lossless->relaunch(which, (hipStream_t)stream);
    });
}

hipjpegStatus_t hipjpegDecodeLosslessBatchStats(hipjpegHandle_t handle, int32_t images_per_kernel[2], uint64_t* h2d_bytes)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (images_per_kernel) {
        images_per_kernel[0] = handle->lossless ? handle->lossless->rows_images() : 0;
        images_per_kernel[1] = handle->lossless ? handle->lossless->wavefront_images() : 0;
    }
    if (h2d_bytes) *h2d_bytes = handle->lossless ? handle->lossless->h2d_bytes() : 0;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

// (hipjpegEncodeLosslessHost / hipjpegEncodeLosslessGpuAlgorithmHost / hipjpegLosslessEncodeShape: lossless_encode_host.cpp, with the rules)
hipjpegStatus_t hipjpegEncodeLosslessBatch(hipjpegHandle_t handle, const hipjpegLosslessEncodeInput_t* inputs, const hipjpegLosslessEncodeParams_t* params,
                                           int batch_size, hipjpegStatus_t* statuses, void* stream)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || batch_size < 0 || (batch_size > 0 && (!inputs || !params))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    if (!handle->lossless_encode) handle->lossless_encode.reset(new LosslessEncodeBatch(handle->device_id, &handle->hooks));
    return handle->lossless_encode->encode(inputs, params, batch_size, statuses, (hipStream_t)stream);
    });
}

hipjpegStatus_t hipjpegEncodeLosslessGetBitstream(hipjpegHandle_t handle, int index, const uint8_t** data, size_t* length)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !handle->lossless_encode || !data || !length) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    return handle->lossless_encode->bitstream(index, data, length);
    });
}

hipjpegStatus_t hipjpegEncodeLosslessBatchStageTimes(hipjpegHandle_t handle, float milliseconds[10])
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle || !handle->lossless_encode || !milliseconds) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(handle->device_id) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    return handle->lossless_encode->stage_times(milliseconds);
    });
}

hipjpegStatus_t hipjpegEncodeLosslessBatchStats(hipjpegHandle_t handle, int32_t* gpu_images, int32_t* waits, uint64_t* bit_buffer_bytes)
{
    return guarded([&]() -> hipjpegStatus_t {
    if (!handle) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (gpu_images) *gpu_images = handle->lossless_encode ? handle->lossless_encode->gpu_images() : 0;
    if (waits) *waits = handle->lossless_encode ? handle->lossless_encode->waits() : 0;
    if (bit_buffer_bytes) *bit_buffer_bytes = handle->lossless_encode ? handle->lossless_encode->bit_buffer_bytes() : 0;
    return HIPJPEG_STATUS_SUCCESS;
    });
}

}  // extern "C"
