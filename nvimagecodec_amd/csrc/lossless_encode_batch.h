// lossless_encode_batch.h -- one hipjpegEncodeLosslessBatch: pictures in device memory to lossless JPEG files in pinned host memory,
// every stage in kernels (lossless_encode_kernels.h), on the caller's stream.  The call waits twice: for the category counts (the
// tables and headers are built on the host) and for the total bits (the bit buffers are laid out on the host).  What follows -- bits,
// stuffing, file assembly, the copy of lengths and offsets -- stays queued; bitstream() waits for it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "lossless_encode_host.h"
#include "lossless_encode_kernels.h"
#include "staging.h"

namespace hipjpeg {

class LosslessEncodeBatch {
public:
    LosslessEncodeBatch(int device_id, const MemoryHooks* hooks);
    ~LosslessEncodeBatch();
    LosslessEncodeBatch(const LosslessEncodeBatch&) = delete;
    LosslessEncodeBatch& operator=(const LosslessEncodeBatch&) = delete;

    // statuses[i] (optional) is final on return.  A failing image launches nothing.
    hipjpegStatus_t encode(const hipjpegLosslessEncodeInput_t* inputs, const hipjpegLosslessEncodeParams_t* params, int batch_size,
                           hipjpegStatus_t* statuses, hipStream_t stream);
    // file `index` of the last encode(); waits for the batch's last copy first
    hipjpegStatus_t bitstream(int index, const uint8_t** data, size_t* length);

    // Of the last encode(), by HIP events on its stream, in ms: 0 descriptors up + statistics, 1 counts down, the first wait and the host's
    // tables, 2 codes up + lengths, 3 scan, 4 totals down, the second wait and the host's layout, 5 descriptors up + clearing the bit
    // buffers, 6 write, 7 count + layout, 8 expand (the files into pinned memory when it is the library's), 9 the copies behind it.
    static constexpr int kStages = 10;
    hipjpegStatus_t stage_times(float ms[kStages]);

    int32_t gpu_images() const { return gpu_images_; }
    int32_t waits() const { return waits_; }
    uint64_t bit_buffer_bytes() const { return bit_buffer_bytes_; }

private:
    // Pages used in turn: the files of a batch stay readable while the next two batches are coded.  A page is taken again only once the
    // event recorded behind its last copy has passed.
    struct Page {
        Page(const MemoryHooks* hooks)
            : pinned1(Buffer::kPinned, hooks), pinned2(Buffer::kPinned, hooks), out(Buffer::kPinned, hooks), dev1(Buffer::kDevice, hooks),
              dev2(Buffer::kDevice, hooks)
        {
        }
        Buffer pinned1;  // phase 1: descriptors and units up, counts and totals back, codes up
        Buffer pinned2;  // phase 2: descriptors, chunk units and headers up, lengths and offsets back
        Buffer out;      // the files
        Buffer dev1, dev2;
        hipEvent_t done = nullptr;
        hipEvent_t mark[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool in_flight = false;
        std::vector<int> slot;  // per image of the batch: its place among the coded ones, -1 for one that failed
        size_t len_at = 0, foff_at = 0;
    };
    hipjpegStatus_t take_page(int* page_index);
    static constexpr int kPages = 3;
    int device_id_;
    Page* pages_[kPages];
    int next_ = 0, last_page_ = -1;
    int32_t gpu_images_ = 0, waits_ = 0;
    uint64_t bit_buffer_bytes_ = 0;
};

}  // namespace hipjpeg
