// lossless_batch.cpp -- see lossless_batch.h
#include "lossless_batch.h"

#include <hip/hip_runtime_api.h>

#include <vector>

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

hipjpegStatus_t LosslessBatch::decode(const uint8_t* const* data, const size_t* lengths, int batch_size, const hipjpegLosslessOutput_t* outputs,
                                      hipjpegStatus_t* statuses, ForkJoinPool* pool, hipStream_t stream)
{
    rows_images_ = wavefront_images_ = 0;
    h2d_bytes_ = 0;
    last_page_ = -1;
    struct Image {
        LosslessFrame frame;
        hipjpegStatus_t status = HIPJPEG_STATUS_SUCCESS;
        size_t diff[4] = {0, 0, 0, 0}, scratch[4] = {0, 0, 0, 0};  // offsets in the arena
    };
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
    const int page_index = next_;
    Page& page = *pages_[next_];
    next_ = (next_ + 1) % kPages;
    if (page.in_flight) {
        if (hipEventSynchronize(page.done) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        page.in_flight = false;
    }
    if (!page.done && hipEventCreateWithFlags(&page.done, hipEventDisableTiming) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    hipjpegStatus_t st = page.pinned.reserve(upload_bytes);
    if (st == HIPJPEG_STATUS_SUCCESS) st = page.device.reserve(carve.end);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;

    // the entropy stage: differences straight into the staging
    pool->parallel_for(batch_size, [&](int i, int) {
        Image& im = images[(size_t)i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) return;
        uint16_t* planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int c = 0; c < im.frame.ncomp; c++) planes[c] = at<uint16_t>(page.pinned, im.diff[c]);
        im.status = lossless_entropy_decode(data[i], im.frame, planes, lossless_diff_pitch((uint32_t)im.frame.width));
    });

    // descriptors of the images that came through: those for the rows kernel first
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
    if (hipMemcpyAsync(page.device.data(), page.pinned.data(), upload_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    h2d_bytes_ = upload_bytes;
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
    last_upload_bytes_ = upload_bytes;
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t LosslessBatch::relaunch(int which, hipStream_t stream)
{
    if (last_page_ < 0 || which < 0 || which > 2) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    Page& page = *pages_[last_page_];
    const LosslessPlane* table = at<LosslessPlane>(page.device, last_table_at_);
    hipError_t err = hipSuccess;
    if (which == 0)
        err = hipMemcpyAsync(page.device.data(), page.pinned.data(), last_upload_bytes_, hipMemcpyHostToDevice, stream);
    else if (which == 1 && last_rows_planes_)
        err = launch_lossless_rows(table, last_rows_planes_, last_max_height_, stream);
    else if (which == 2 && last_wave_planes_)
        err = launch_lossless_wavefront(table + last_rows_planes_, last_wave_planes_, stream);
    if (err != hipSuccess || hipEventRecord(page.done, stream) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    page.in_flight = true;
    return HIPJPEG_STATUS_SUCCESS;
}

}  // namespace hipjpeg
