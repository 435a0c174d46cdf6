// lossless_batch.h -- one hipjpegDecodeLosslessBatch: frames checked and entropy-decoded on the host threads into pinned staging, one
// upload, the reconstruction kernels on the caller's stream.  With HIPJPEG_FLAG_GPU_HUFFMAN the compressed scans travel instead and
// the entropy stage runs on the GPU too.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include <vector>

#include "lossless_entropy_kernels.h"
#include "lossless_gpu_host.h"
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
    // flags: 0, or HIPJPEG_FLAG_GPU_HUFFMAN -- the entropy stage on the GPU (lossless_entropy_kernels.hip); the call then waits once,
    // for the kernels' verdict words, and hands what they turned away to the host stage.
    hipjpegStatus_t decode(const uint8_t* const* data, const size_t* lengths, int batch_size, const hipjpegLosslessOutput_t* outputs,
                           hipjpegStatus_t* statuses, unsigned flags, ForkJoinPool* pool, hipStream_t stream);

    // Queues one part of the last decode() again, for measurements: 0 = the upload, 1 = the column sums and lossless_rows_kernel,
    // 2 = lossless_wavefront_kernel, 3 = destuffing and synchronisation of the GPU entropy stage, 4 = its write pass (3 and 4: only behind
    // a decode() with the flag in which no image went to the host stage).  The parts read the staging and write the outputs, the
    // differences and the scratch, so repeating them changes nothing.
    hipjpegStatus_t relaunch(int which, hipStream_t stream);

    int32_t rows_images() const { return rows_images_; }
    int32_t wavefront_images() const { return wavefront_images_; }
    uint64_t h2d_bytes() const { return h2d_bytes_; }
    // of the last decode() with the flag: images whose differences the kernels made, images the host stage decoded, ripple launches
    // that found work
    int32_t gpu_images() const { return gpu_images_; }
    int32_t host_fallback_images() const { return host_fallback_images_; }
    int32_t ripple_launches() const { return ripple_launches_; }

private:
    // Staging pages used in turn: the host stage of a call may fill one while the copy of the call before still reads another.  A
    // page is taken again only once the event recorded behind its kernels has passed.
    struct Page {
        Page(const MemoryHooks* hooks) : pinned(Buffer::kPinned, hooks), device(Buffer::kDevice, hooks), fallback(Buffer::kPinned, hooks) {}
        Buffer pinned, device;
        Buffer fallback;  // differences of the images the GPU entropy stage left to the host stage
        hipEvent_t done = nullptr;
        bool in_flight = false;
    };
    struct Image {
        LosslessFrame frame;
        hipjpegStatus_t status = HIPJPEG_STATUS_SUCCESS;
        size_t diff[4] = {0, 0, 0, 0}, scratch[4] = {0, 0, 0, 0};  // offsets in the arena
        // GPU entropy stage
        bool gpu = false;
        uint32_t gpu_index = 0;
        std::vector<LlRawSegment> segments;
        std::vector<size_t> raw, stream;       // per segment: offsets in the arena
        size_t host_diff[4] = {0, 0, 0, 0};    // offsets in Page::fallback
    };
    hipjpegStatus_t take_page(size_t pinned_bytes, size_t device_bytes, int* page_index);
    hipjpegStatus_t decode_gpu_entropy(const uint8_t* const* data, int batch_size, const hipjpegLosslessOutput_t* outputs, hipjpegStatus_t* statuses,
                                       std::vector<Image>& images, ForkJoinPool* pool, hipStream_t stream);
    hipjpegStatus_t reconstruct(Page& page, int page_index, const std::vector<Image>& images, int batch_size, const hipjpegLosslessOutput_t* outputs,
                                hipjpegStatus_t* statuses, size_t table_at, size_t copy_begin, size_t copy_end, hipStream_t stream);
    static constexpr int kPages = 3;
    int device_id_;
    Page* pages_[kPages];
    int next_ = 0;
    // the last decode(), for relaunch()
    int last_page_ = -1, last_rows_planes_ = 0, last_wave_planes_ = 0, last_max_height_ = 0;
    size_t last_table_at_ = 0, last_upload_bytes_ = 0;
    int32_t rows_images_ = 0, wavefront_images_ = 0;
    uint64_t h2d_bytes_ = 0;
    int32_t gpu_images_ = 0, host_fallback_images_ = 0, ripple_launches_ = 0;
    LlArrays last_entropy_ = LlArrays();  // num_units = 0: nothing to queue again
};

}  // namespace hipjpeg
