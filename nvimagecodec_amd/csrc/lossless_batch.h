// lossless_batch.h -- one hipjpegDecodeLosslessBatch: frames checked and entropy-decoded on the host threads into pinned staging, one
// upload, the reconstruction kernels on the caller's stream.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "lossless_host.h"
#include "staging.h"
#include "thread_pool.h"

namespace hipjpeg {

class LosslessBatch {
public:
    LosslessBatch(int device_id, const MemoryHooks* hooks);
    ~LosslessBatch();
    LosslessBatch(const LosslessBatch&) = delete;
    LosslessBatch& operator=(const LosslessBatch&) = delete;

    // Asynchronous on `stream`; statuses[i] (optional) is final on return.  A failing image launches nothing.
    hipjpegStatus_t decode(const uint8_t* const* data, const size_t* lengths, int batch_size, const hipjpegLosslessOutput_t* outputs,
                           hipjpegStatus_t* statuses, ForkJoinPool* pool, hipStream_t stream);

    // Queues one part of the last decode() again, for measurements: 0 = the upload, 1 = the column sums and lossless_rows_kernel,
    // 2 = lossless_wavefront_kernel.  The parts read the staging and write the outputs and the scratch, so repeating them changes nothing.
    hipjpegStatus_t relaunch(int which, hipStream_t stream);

    int32_t rows_images() const { return rows_images_; }
    int32_t wavefront_images() const { return wavefront_images_; }
    uint64_t h2d_bytes() const { return h2d_bytes_; }

private:
    // Staging pages used in turn: the host stage of a call may fill one while the copy of the call before still reads another.  A
    // page is taken again only once the event recorded behind its kernels has passed.
    struct Page {
        Page(const MemoryHooks* hooks) : pinned(Buffer::kPinned, hooks), device(Buffer::kDevice, hooks) {}
        Buffer pinned, device;
        hipEvent_t done = nullptr;
        bool in_flight = false;
    };
    static constexpr int kPages = 3;
    int device_id_;
    Page* pages_[kPages];
    int next_ = 0;
    // the last decode(), for relaunch()
    int last_page_ = -1, last_rows_planes_ = 0, last_wave_planes_ = 0, last_max_height_ = 0;
    size_t last_table_at_ = 0, last_upload_bytes_ = 0;
    int32_t rows_images_ = 0, wavefront_images_ = 0;
    uint64_t h2d_bytes_ = 0;
};

}  // namespace hipjpeg
