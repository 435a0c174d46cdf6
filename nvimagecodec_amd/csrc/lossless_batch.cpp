// lossless_batch.cpp -- see lossless_batch.h
#include "lossless_batch.h"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "lossless_entropy_kernels.h"
#include "lossless_kernels.h"

namespace hipjpeg {

LosslessBatch::LosslessBatch(int device_id, const MemoryHooks* hooks) : device_id_(device_id)
{
    for (auto& p : pages_) p = new Page(hooks);
}

LosslessBatch::~LosslessBatch()
{
    (void)hipSetDevice(device_id_);
    for (auto& p : pages_) {
        if (p->in_flight) (void)hipEventSynchronize(p->done);
        if (p->done) (void)hipEventDestroy(p->done);
        delete p;
    }
}

// The next staging page, free of the call that used it last, with room for `pinned_bytes` and `device_bytes`
hipjpegStatus_t LosslessBatch::take_page(size_t pinned_bytes, size_t device_bytes, int* page_index)
{
    *page_index = next_;
    Page& page = *pages_[next_];
    next_ = (next_ + 1) % kPages;
    if (page.in_flight) {
        if (hipEventSynchronize(page.done) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        page.in_flight = false;
    }
    if (!page.done && hipEventCreateWithFlags(&page.done, hipEventDisableTiming) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    hipjpegStatus_t st = page.pinned.reserve(pinned_bytes);
    if (st == HIPJPEG_STATUS_SUCCESS) st = page.device.reserve(device_bytes);
    return st;
}

hipjpegStatus_t LosslessBatch::decode(const uint8_t* const* data, const size_t* lengths, int batch_size, const hipjpegLosslessOutput_t* outputs,
                                      hipjpegStatus_t* statuses, unsigned flags, ForkJoinPool* pool, hipStream_t stream)
{
    rows_images_ = wavefront_images_ = 0;
    gpu_images_ = host_fallback_images_ = ripple_launches_ = 0;
    h2d_bytes_ = 0;
    last_page_ = -1;
    last_entropy_ = LlArrays();
    std::vector<Image> images((size_t)batch_size);
    pool->parallel_for(batch_size, [&](int i, int) {
        Image& im = images[(size_t)i];
        if (!data[i]) {
            im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
            return;
        }
        im.status = lossless_frame(data[i], lengths[i], &im.frame);
        if (im.status == HIPJPEG_STATUS_SUCCESS) im.status = lossless_output_ok(im.frame, outputs[i]);
    });
    if (flags & HIPJPEG_FLAG_GPU_HUFFMAN) return decode_gpu_entropy(data, batch_size, outputs, statuses, images, pool, stream);
    // the arena: both descriptor tables and the difference planes travel; the scratch behind them exists on the device only
    Carve carve;
    size_t planes_total = 0;
    for (const Image& im : images)
        if (im.status == HIPJPEG_STATUS_SUCCESS) planes_total += (size_t)im.frame.ncomp;
    const size_t table_at = carve.take(planes_total * sizeof(LosslessPlane));
    for (Image& im : images) {
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const size_t bytes = (size_t)lossless_diff_pitch((uint32_t)im.frame.width) * (size_t)im.frame.height * sizeof(uint16_t);
        for (int c = 0; c < im.frame.ncomp; c++) im.diff[c] = carve.take(bytes);
    }
    const size_t upload_bytes = carve.end;
    for (Image& im : images) {
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const bool rows = lossless_takes_rows_kernel((uint32_t)im.frame.ps, (uint32_t)im.frame.width);
        const size_t bytes = (rows ? align_up((size_t)im.frame.height, 8) : (size_t)lossless_diff_pitch((uint32_t)im.frame.width)) * sizeof(uint16_t);
        for (int c = 0; c < im.frame.ncomp; c++) im.scratch[c] = carve.take(bytes);
    }
    if (planes_total == 0) {
        if (statuses)
            for (int i = 0; i < batch_size; i++) statuses[i] = images[(size_t)i].status;
        return HIPJPEG_STATUS_SUCCESS;
    }
    int page_index;
    const hipjpegStatus_t st = take_page(upload_bytes, carve.end, &page_index);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    Page& page = *pages_[page_index];

    // the entropy stage: differences straight into the staging
    pool->parallel_for(batch_size, [&](int i, int) {
        Image& im = images[(size_t)i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) return;
        uint16_t* planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int c = 0; c < im.frame.ncomp; c++) planes[c] = at<uint16_t>(page.pinned, im.diff[c]);
        im.status = lossless_entropy_decode(data[i], im.frame, planes, lossless_diff_pitch((uint32_t)im.frame.width));
    });

    return reconstruct(page, page_index, images, batch_size, outputs, statuses, table_at, 0, upload_bytes, stream);
}

// HIPJPEG_FLAG_GPU_HUFFMAN: the compressed scans travel, the entropy kernels leave the differences where the host stage's would
// have been uploaded, and the call waits ONCE for their verdict words.  Images the device flagged, whose rounds did not converge, or
// that lossless_gpu_segments turned away are then decoded by the host stage, which names their status; what it decodes is uploaded.
hipjpegStatus_t LosslessBatch::decode_gpu_entropy(const uint8_t* const* data, int batch_size, const hipjpegLosslessOutput_t* outputs,
                                                  hipjpegStatus_t* statuses, std::vector<Image>& images, ForkJoinPool* pool, hipStream_t stream)
{
    // the host's share: where the intervals lie
    pool->parallel_for(batch_size, [&](int i, int) {
        Image& im = images[(size_t)i];
        if (im.status == HIPJPEG_STATUS_SUCCESS) im.gpu = lossless_gpu_segments(data[i], im.frame, &im.segments);
    });
    size_t planes_total = 0, num_gpu = 0, num_segments = 0, num_units = 0, num_chunks = 0, num_subseq = 0;
    for (const Image& im : images) {
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        planes_total += (size_t)im.frame.ncomp;
        if (!im.gpu) continue;
        num_gpu++;
        num_segments += im.segments.size();
        for (const LlRawSegment& sg : im.segments) {
            const size_t bytes = sg.end - sg.begin, subseq = (bytes * 8 + kLlSubseqBits - 1) / kLlSubseqBits;
            num_subseq += subseq;
            num_units += (subseq + kLlLanes - 1) / kLlLanes;
            num_chunks += (bytes + kLlDestuffChunk - 1) / kLlDestuffChunk;
        }
    }
    if (planes_total == 0) {
        if (statuses)
            for (int i = 0; i < batch_size; i++) statuses[i] = images[(size_t)i].status;
        return HIPJPEG_STATUS_SUCCESS;
    }
    if (num_subseq > 0xFFFFFFFFull || num_chunks > 0x7FFFFFFFull) return HIPJPEG_STATUS_ALLOC_FAILED;
    // the arena: descriptors, table specifications and raw scans travel; behind them the words that come back, then what only the device has
    Carve carve;
    const size_t table_at = carve.take(planes_total * sizeof(LosslessPlane));
    const size_t table_end = carve.end;
    const size_t images_at = carve.take(num_gpu * sizeof(LlImage));
    const size_t segments_at = carve.take(num_segments * sizeof(LlSegment));
    const size_t units_at = carve.take(num_units * sizeof(LlUnit));
    const size_t chunk_units_at = carve.take(num_chunks * sizeof(LlUnit));
    const size_t specs_at = carve.take(num_gpu * 4 * kLlSpecWords * sizeof(uint32_t));
    for (Image& im : images) {
        if (!im.gpu) continue;
        im.raw.resize(im.segments.size());
        for (size_t k = 0; k < im.segments.size(); k++) im.raw[k] = carve.take(align_up(im.segments[k].end - im.segments[k].begin, 16), 16);
    }
    const size_t upload_bytes = carve.end;
    const size_t back_words = num_gpu + kLlMaxRipple + 1;
    const size_t back_at = carve.take(back_words * sizeof(uint32_t));
    const size_t pinned_bytes = carve.end;
    for (Image& im : images) {
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const size_t bytes = (size_t)lossless_diff_pitch((uint32_t)im.frame.width) * (size_t)im.frame.height * sizeof(uint16_t);
        for (int c = 0; c < im.frame.ncomp; c++) im.diff[c] = carve.take(bytes);
        const bool rows = lossless_takes_rows_kernel((uint32_t)im.frame.ps, (uint32_t)im.frame.width);
        const size_t sbytes = (rows ? align_up((size_t)im.frame.height, 8) : (size_t)lossless_diff_pitch((uint32_t)im.frame.width)) * sizeof(uint16_t);
        for (int c = 0; c < im.frame.ncomp; c++) im.scratch[c] = carve.take(sbytes);
        if (!im.gpu) continue;
        im.stream.resize(im.segments.size());
        for (size_t k = 0; k < im.segments.size(); k++) im.stream[k] = carve.take(align_up(im.segments[k].end - im.segments[k].begin, 4), 16);
    }
    const size_t drops_at = carve.take(num_chunks * sizeof(uint32_t));
    const size_t seg_bits_at = carve.take(num_segments * sizeof(uint32_t));
    const size_t start_at = carve.take(num_subseq * sizeof(uint64_t));
    const size_t end_at = carve.take(num_subseq * sizeof(uint64_t));
    const size_t count_at = carve.take(num_subseq * sizeof(uint32_t));
    const size_t unit_out_at = carve.take(2 * num_units * sizeof(uint64_t));
    const size_t unit_count_at = carve.take(num_units * sizeof(uint32_t));
    int page_index;
    const hipjpegStatus_t st = take_page(pinned_bytes, carve.end, &page_index);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    Page& page = *pages_[page_index];
    uint8_t* const dev = page.device.data();

    // descriptors, in image order; the raw scans are copied by the threads
    {
        LlImage* ims = at<LlImage>(page.pinned, images_at);
        LlSegment* sgs = at<LlSegment>(page.pinned, segments_at);
        LlUnit* units = at<LlUnit>(page.pinned, units_at);
        LlUnit* chunk_units = at<LlUnit>(page.pinned, chunk_units_at);
        uint32_t g = 0, s = 0, u = 0, ch = 0, sub = 0;
        for (Image& im : images) {
            if (!im.gpu) continue;
            im.gpu_index = g;
            uint32_t* specs = at<uint32_t>(page.pinned, specs_at) + (size_t)g * 4 * kLlSpecWords;
            LlImage& d = ims[g];
            d = LlImage();
            d.ntables = lossless_gpu_tables(im.frame, specs);
            d.specs = reinterpret_cast<const uint32_t*>(dev + specs_at) + (size_t)g * 4 * kLlSpecWords;
            for (int c = 0; c < 4; c++) d.plane[c] = c < im.frame.ncomp ? reinterpret_cast<uint16_t*>(dev + im.diff[im.frame.scan_comp[c]]) : nullptr;
            d.ncomp = (uint32_t)im.frame.ncomp;
            d.width = (uint32_t)im.frame.width;
            d.height = (uint32_t)im.frame.height;
            d.pitch = lossless_diff_pitch((uint32_t)im.frame.width);
            for (size_t k = 0; k < im.segments.size(); k++) {
                const uint32_t bytes = (uint32_t)(im.segments[k].end - im.segments[k].begin);
                LlSegment& sg = sgs[s];
                sg.raw = dev + im.raw[k];
                sg.stream = dev + im.stream[k];
                sg.raw_bytes = bytes;
                sg.image = g;
                sg.first_subseq = sub;
                sg.max_subseq = (uint32_t)(((uint64_t)bytes * 8 + kLlSubseqBits - 1) / kLlSubseqBits);
                sg.first_chunk = ch;
                sg.first_unit = u;
                sg.samples = (uint32_t)lossless_gpu_samples(im.frame, k);
                sg.first_row = lossless_gpu_first_row(im.frame, k);
                for (uint32_t first = 0; first < sg.max_subseq; first += kLlLanes) units[u++] = LlUnit{s, first};
                for (uint32_t c = 0; c * kLlDestuffChunk < bytes; c++) chunk_units[ch++] = LlUnit{s, c};
                sub += sg.max_subseq;
                s++;
            }
            g++;
        }
    }
    pool->parallel_for(batch_size, [&](int i, int) {
        const Image& im = images[(size_t)i];
        if (!im.gpu) return;
        for (size_t k = 0; k < im.segments.size(); k++) {
            const size_t bytes = im.segments[k].end - im.segments[k].begin;
            uint8_t* dst = at<uint8_t>(page.pinned, im.raw[k]);
            memcpy(dst, data[i] + im.segments[k].begin, bytes);
            memset(dst + bytes, 0x01, align_up(bytes, 16) - bytes);
        }
    });

    uint32_t* back = at<uint32_t>(page.pinned, back_at);
    if (num_gpu) {
        LlArrays a;
        a.images = at<LlImage>(page.device, images_at);
        a.segments = at<LlSegment>(page.device, segments_at);
        a.chunk_units = at<LlUnit>(page.device, chunk_units_at);
        a.units = at<LlUnit>(page.device, units_at);
        a.num_chunk_units = (int)num_chunks;
        a.num_units = (int)num_units;
        a.drops = at<uint32_t>(page.device, drops_at);
        a.seg_bits = at<uint32_t>(page.device, seg_bits_at);
        a.start = at<uint64_t>(page.device, start_at);
        a.end = at<uint64_t>(page.device, end_at);
        a.count = at<uint32_t>(page.device, count_at);
        a.unit_out = at<uint64_t>(page.device, unit_out_at);
        a.unit_count = at<uint32_t>(page.device, unit_count_at);
        a.verdicts = at<uint32_t>(page.device, back_at);
        a.moved = a.verdicts + num_gpu;
        // the one wait of the call: statuses are final on return and a failing image's output stays untouched, so the verdicts must be
        // here before any reconstruction kernel is queued
        bool ok = hipMemcpyAsync(dev, page.pinned.data(), upload_bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
        page.in_flight = true;
        ok = ok && hipMemsetAsync(a.verdicts, 0, back_words * sizeof(uint32_t), stream) == hipSuccess;
        ok = ok && launch_lossless_entropy_sync(a, stream) == hipSuccess;
        ok = ok && launch_lossless_entropy_write(a, stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(back, a.verdicts, back_words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess;
        ok = hipStreamSynchronize(stream) == hipSuccess && ok;
        page.in_flight = false;
        if (!ok) return HIPJPEG_STATUS_HIP_ERROR;
        h2d_bytes_ += upload_bytes;
        for (uint32_t l = 1; l <= kLlMaxRipple; l++)
            if (back[num_gpu + l]) ripple_launches_++;
        last_entropy_ = a;
    }

    // the host stage for what is left to it, into a staging of its own
    Carve again;
    std::vector<int> fallback;
    for (int i = 0; i < batch_size; i++) {
        Image& im = images[(size_t)i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        if (im.gpu && back[im.gpu_index] == 0) {
            gpu_images_++;
            continue;
        }
        fallback.push_back(i);
        const size_t bytes = (size_t)lossless_diff_pitch((uint32_t)im.frame.width) * (size_t)im.frame.height * sizeof(uint16_t);
        for (int c = 0; c < im.frame.ncomp; c++) im.host_diff[c] = again.take(bytes);
    }
    host_fallback_images_ = (int32_t)fallback.size();
    if (!fallback.empty()) {
        const hipjpegStatus_t fst = page.fallback.reserve(again.end);
        if (fst != HIPJPEG_STATUS_SUCCESS) return fst;
        pool->parallel_for((int)fallback.size(), [&](int j, int) {
            const int i = fallback[(size_t)j];
            Image& im = images[(size_t)i];
            uint16_t* planes[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int c = 0; c < im.frame.ncomp; c++) planes[c] = at<uint16_t>(page.fallback, im.host_diff[c]);
            im.status = lossless_entropy_decode(data[i], im.frame, planes, lossless_diff_pitch((uint32_t)im.frame.width));
        });
        for (int i : fallback) {
            const Image& im = images[(size_t)i];
            if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
            const size_t bytes = (size_t)lossless_diff_pitch((uint32_t)im.frame.width) * (size_t)im.frame.height * sizeof(uint16_t);
            for (int c = 0; c < im.frame.ncomp; c++) {
                if (hipMemcpyAsync(dev + im.diff[c], page.fallback.data() + im.host_diff[c], bytes, hipMemcpyHostToDevice, stream) != hipSuccess) {
                    (void)hipStreamSynchronize(stream);
                    return HIPJPEG_STATUS_HIP_ERROR;
                }
                page.in_flight = true;
                h2d_bytes_ += bytes;
            }
        }
        last_entropy_ = LlArrays();  // (the write pass would store over what the host stage decoded: nothing to queue again)
    }
    last_upload_bytes_ = upload_bytes;
    const hipjpegStatus_t rst = reconstruct(page, page_index, images, batch_size, outputs, statuses, table_at, table_at, table_end, stream);
    if (rst == HIPJPEG_STATUS_SUCCESS && page.in_flight && last_page_ < 0) {
        // fallback copies were queued, yet no image came through: the page is free once they have passed
        (void)hipStreamSynchronize(stream);
        page.in_flight = false;
    }
    return rst;
}

// Descriptors of the images that came through, those for the rows kernel first; bytes [copy_begin, copy_end) of the page's staging
// travel (the descriptors among them), then the reconstruction kernels are queued.
hipjpegStatus_t LosslessBatch::reconstruct(Page& page, int page_index, const std::vector<Image>& images, int batch_size,
                                           const hipjpegLosslessOutput_t* outputs, hipjpegStatus_t* statuses, size_t table_at, size_t copy_begin,
                                           size_t copy_end, hipStream_t stream)
{
    LosslessPlane* table = at<LosslessPlane>(page.pinned, table_at);
    const uint64_t base = (uint64_t)reinterpret_cast<uintptr_t>(page.device.data());
    int num_rows = 0, num_wave = 0, max_height = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < batch_size; i++) {
            const Image& im = images[(size_t)i];
            if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
            const bool rows = lossless_takes_rows_kernel((uint32_t)im.frame.ps, (uint32_t)im.frame.width);
            if (rows != (pass == 0)) continue;
            uint64_t diff[4], scratch[4];
            for (int c = 0; c < 4; c++) {
                diff[c] = base + im.diff[c];
                scratch[c] = base + im.scratch[c];
            }
            lossless_planes(im.frame, outputs[i], diff, scratch, table + num_rows + num_wave);
            if (rows) {
                num_rows += im.frame.ncomp;
                rows_images_++;
                if (im.frame.height > max_height) max_height = im.frame.height;
            } else {
                num_wave += im.frame.ncomp;
                wavefront_images_++;
            }
        }
    if (statuses)
        for (int i = 0; i < batch_size; i++) statuses[i] = images[(size_t)i].status;
    if (num_rows + num_wave == 0) return HIPJPEG_STATUS_SUCCESS;
    if (hipMemcpyAsync(page.device.data() + copy_begin, page.pinned.data() + copy_begin, copy_end - copy_begin, hipMemcpyHostToDevice, stream) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    h2d_bytes_ += copy_end - copy_begin;
    page.in_flight = true;  // from here on the page is the stream's until the event has passed
    const LosslessPlane* device_table = at<LosslessPlane>(page.device, table_at);
    hipError_t err = hipSuccess;
    if (num_rows) err = launch_lossless_rows(device_table, num_rows, max_height, stream);
    if (err == hipSuccess && num_wave) err = launch_lossless_wavefront(device_table + num_rows, num_wave, stream);
    if (hipEventRecord(page.done, stream) != hipSuccess || err != hipSuccess) {
        (void)hipStreamSynchronize(stream);  // nothing of this batch stays queued behind an error
        page.in_flight = false;
        return HIPJPEG_STATUS_HIP_ERROR;
    }
    last_page_ = page_index;
    last_rows_planes_ = num_rows;
    last_wave_planes_ = num_wave;
    last_max_height_ = max_height;
    last_table_at_ = table_at;
    if (copy_begin == 0) last_upload_bytes_ = copy_end;
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t LosslessBatch::relaunch(int which, hipStream_t stream)
{
    if (last_page_ < 0 || which < 0 || which > 4) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (which >= 3 && last_entropy_.num_units == 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    Page& page = *pages_[last_page_];
    const LosslessPlane* table = at<LosslessPlane>(page.device, last_table_at_);
    hipError_t err = hipSuccess;
    if (which == 0)
        err = hipMemcpyAsync(page.device.data(), page.pinned.data(), last_upload_bytes_, hipMemcpyHostToDevice, stream);
    else if (which == 1 && last_rows_planes_)
        err = launch_lossless_rows(table, last_rows_planes_, last_max_height_, stream);
    else if (which == 2 && last_wave_planes_)
        err = launch_lossless_wavefront(table + last_rows_planes_, last_wave_planes_, stream);
    else if (which == 3)
        err = launch_lossless_entropy_sync(last_entropy_, stream);
    else if (which == 4)
        err = launch_lossless_entropy_write(last_entropy_, stream);
    if (err != hipSuccess || hipEventRecord(page.done, stream) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    page.in_flight = true;
    return HIPJPEG_STATUS_SUCCESS;
}

}  // namespace hipjpeg
