// lossless_encode_batch.cpp -- see lossless_encode_batch.h
#include "lossless_encode_batch.h"

#include <cstring>

namespace hipjpeg {

LosslessEncodeBatch::LosslessEncodeBatch(int device_id, const MemoryHooks* hooks) : device_id_(device_id)
{
    for (auto& p : pages_) p = new Page(hooks);
}

LosslessEncodeBatch::~LosslessEncodeBatch()
{
    (void)hipSetDevice(device_id_);
    for (auto& p : pages_) {
        if (p->in_flight) (void)hipEventSynchronize(p->done);
        if (p->done) (void)hipEventDestroy(p->done);
        for (hipEvent_t e : p->mark)
            if (e) (void)hipEventDestroy(e);
        delete p;
    }
}

hipjpegStatus_t LosslessEncodeBatch::take_page(int* page_index)
{
    *page_index = next_;
    Page& page = *pages_[next_];
    next_ = (next_ + 1) % kPages;
    if (page.in_flight) {
        if (hipEventSynchronize(page.done) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        page.in_flight = false;
    }
    if (!page.done && hipEventCreateWithFlags(&page.done, hipEventDisableTiming) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    for (hipEvent_t& e : page.mark)
        if (!e && hipEventCreate(&e) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t LosslessEncodeBatch::encode(const hipjpegLosslessEncodeInput_t* inputs, const hipjpegLosslessEncodeParams_t* params, int batch_size,
                                            hipjpegStatus_t* statuses, hipStream_t stream)
{
    gpu_images_ = waits_ = 0;
    bit_buffer_bytes_ = 0;
    last_page_ = -1;
    // ---- the argument rules and the uint32 predicate, before anything is launched
    std::vector<LencImage> images;
    std::vector<int> source;  // image of the batch behind each descriptor
    std::vector<int> slot((size_t)batch_size, -1);
    std::vector<LencUnit> units;
    size_t ngroups = 0;
    for (int i = 0; i < batch_size; i++) {
        LencImage im;
        hipjpegStatus_t st = lossless_encode_describe(inputs[i], params[i], &im);
        if (st == HIPJPEG_STATUS_SUCCESS && !lenc_offsets_fit((uint64_t)im.row_samples * im.height, lenc_intervals(im))) st = HIPJPEG_STATUS_UNSUPPORTED;
        if (st == HIPJPEG_STATUS_SUCCESS && ngroups + im.num_groups > 0xFFFFFFFFull) st = HIPJPEG_STATUS_UNSUPPORTED;  // batch-wide group arrays
        if (statuses) statuses[i] = st;
        if (st != HIPJPEG_STATUS_SUCCESS) continue;
        im.index = (uint32_t)images.size();
        im.first_group = (uint32_t)ngroups;
        for (uint32_t g = 0; g < im.num_groups; g += kLencThreads) units.push_back(LencUnit{im.index, g});
        ngroups += im.num_groups;
        slot[(size_t)i] = (int)im.index;
        images.push_back(im);
        source.push_back(i);
    }
    const size_t n = images.size();
    if (n == 0) return HIPJPEG_STATUS_SUCCESS;
    if (units.size() > 0x7FFFFFFFull || n > 0x7FFFFFFFull / 128) return HIPJPEG_STATUS_ALLOC_FAILED;
    int page_index;
    hipjpegStatus_t st = take_page(&page_index);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    Page& page = *pages_[page_index];
    page.slot = slot;

    // ---- phase 1: statistics, table, lengths, offsets
    Carve c1;
    const size_t images_at = c1.take(n * sizeof(LencImage));
    const size_t units_at = c1.take(units.size() * sizeof(LencUnit));
    const size_t upload1 = c1.end;
    const size_t counts_at = c1.take(n * kLencCountStride * sizeof(uint32_t));
    const size_t totals_at = c1.take(n * sizeof(uint32_t));
    const size_t codes_at = c1.take(n * kLencCountStride * sizeof(uint32_t));
    const size_t pinned1_end = c1.end;
    const size_t spans_at = c1.take(ngroups * sizeof(uint32_t));
    const size_t offsets_at = c1.take(ngroups * sizeof(uint32_t));
    if ((st = page.pinned1.reserve(pinned1_end + 256)) != HIPJPEG_STATUS_SUCCESS || (st = page.dev1.reserve(c1.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    uint8_t* const d1 = page.dev1.data();
    for (LencImage& im : images) {
        im.counts = (uint64_t)reinterpret_cast<uintptr_t>(d1 + counts_at) + (uint64_t)im.index * kLencCountStride * sizeof(uint32_t);
        im.codes = (uint64_t)reinterpret_cast<uintptr_t>(d1 + codes_at) + (uint64_t)im.index * kLencCountStride * sizeof(uint32_t);
    }
    copy_table(page.pinned1, images_at, images);
    copy_table(page.pinned1, units_at, units);
    const LencImage* dimages = at<const LencImage>(page.dev1, images_at);
    const LencUnit* dunits = at<const LencUnit>(page.dev1, units_at);
    auto fail = [&]() {
        (void)hipStreamSynchronize(stream);  // nothing of this batch stays queued behind an error
        page.in_flight = false;
        return HIPJPEG_STATUS_HIP_ERROR;
    };
    auto mark = [&](int k) { return hipEventRecord(page.mark[k], stream); };  // stage borders, for stage_times()
    page.in_flight = true;
    if (mark(0) != hipSuccess || hipMemcpyAsync(d1, page.pinned1.data(), upload1, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemsetAsync(d1 + counts_at, 0, n * kLencCountStride * sizeof(uint32_t), stream) != hipSuccess ||
        launch_lenc_stats(dimages, (int)n, stream) != hipSuccess || mark(1) != hipSuccess ||
        hipMemcpyAsync(page.pinned1.data() + counts_at, d1 + counts_at, n * kLencCountStride * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail();
    waits_++;
    std::vector<std::vector<uint8_t>> headers(n);
    for (size_t k = 0; k < n; k++) {
        uint32_t* codes = at<uint32_t>(page.pinned1, codes_at) + k * kLencCountStride;
        memset(codes, 0, kLencCountStride * sizeof(uint32_t));
        lossless_encode_headers(images[k], params[source[k]], at<const uint32_t>(page.pinned1, counts_at) + k * kLencCountStride, codes, &headers[k]);
    }
    if (mark(2) != hipSuccess || hipMemcpyAsync(d1 + codes_at, page.pinned1.data() + codes_at, n * kLencCountStride * sizeof(uint32_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
        launch_lenc_length(dimages, dunits, (int)units.size(), at<uint32_t>(page.dev1, spans_at), stream) != hipSuccess || mark(3) != hipSuccess ||
        launch_lenc_scan(dimages, (int)n, at<const uint32_t>(page.dev1, spans_at), at<uint32_t>(page.dev1, offsets_at), at<uint32_t>(page.dev1, totals_at),
                         stream) != hipSuccess ||
        mark(4) != hipSuccess || hipMemcpyAsync(page.pinned1.data() + totals_at, d1 + totals_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail();
    waits_++;

    // ---- phase 2: bit buffers, stuffing, files (gpu_huffman_encode.hip's count / layout / expand over descriptors filled here)
    const uint32_t* totals = at<const uint32_t>(page.pinned1, totals_at);
    std::vector<HencImage> segs(n);
    std::vector<HencUnit> chunk_units;
    std::vector<size_t> raw_off(n), hdr_off(n);
    Carve raw, hdr;
    size_t arena_cap = 0;
    bool restart = false;
    for (size_t k = 0; k < n; k++) {
        HencImage& h = segs[k];
        memset(&h, 0, sizeof h);
        h.raw_bytes = (totals[k] + 7) / 8;
        h.first_chunk = (uint32_t)chunk_units.size();
        h.num_chunks = (h.raw_bytes + kHencChunk - 1) / kHencChunk;
        for (uint32_t c = 0; c < h.num_chunks; c++) chunk_units.push_back(HencUnit{(uint32_t)k, c});
        h.header_bytes = (uint32_t)headers[k].size();
        h.nseg = h.last_seg = 1;
        h.rst_blocks = lenc_intervals(images[k]) > 1 ? 1u : 0u;  // to count / expand: the marker bitmap lies behind the bit buffer
        restart = restart || h.rst_blocks;
        raw_off[k] = raw.take(h.rst_blocks ? (size_t)henc_map_offset(h.raw_bytes) + henc_map_bytes(h.raw_bytes) : (size_t)h.raw_bytes + 16);
        hdr_off[k] = hdr.take(headers[k].size(), 16);
        arena_cap += align_up(2 + (size_t)h.header_bytes + 2 * (size_t)h.raw_bytes, 16);  // every byte could be 0xFF
    }
    const size_t raw_total = raw.take(0), hdr_total = hdr.take(0, 16), nchunks = chunk_units.size();
    if (nchunks > 0x7FFFFFFFull) return HIPJPEG_STATUS_ALLOC_FAILED;
    Carve c2;
    const size_t desc_at = c2.take(sizeof(HencImage) * n);
    const size_t chunks_at = c2.take(sizeof(HencUnit) * nchunks);
    const size_t headers_at = c2.take(hdr_total);
    const size_t upload2 = c2.end;
    const size_t len_at = c2.take(n * 4);
    const size_t foff_at = c2.take(n * 8);
    const size_t pinned2_end = c2.end;
    const size_t ff_at = c2.take(nchunks * 4);
    const size_t cout_at = c2.take(nchunks * 4);
    const size_t raw_at = c2.take(raw_total);
    const size_t arena_at = c2.take(arena_cap);
    if ((st = page.pinned2.reserve(pinned2_end + 256)) != HIPJPEG_STATUS_SUCCESS || (st = page.dev2.reserve(c2.end + 256)) != HIPJPEG_STATUS_SUCCESS ||
        (st = page.out.reserve(arena_cap + 256)) != HIPJPEG_STATUS_SUCCESS)
        return st;
    uint8_t* const d2 = page.dev2.data();
    for (size_t k = 0; k < n; k++) {
        segs[k].raw = d2 + raw_at + raw_off[k];
        segs[k].header = d2 + headers_at + hdr_off[k];
        copy_table(page.pinned2, headers_at + hdr_off[k], headers[k]);
    }
    copy_table(page.pinned2, desc_at, segs);
    copy_table(page.pinned2, chunks_at, chunk_units);
    // The files go straight into pinned host memory when it is ours (mapped into the device's address space); with a caller's pinned
    // allocator the mapping is unknown: they are assembled in HBM and copied, over the whole capacity (the lengths are not here yet).
    const bool direct = !page.out.custom();
    const HencImage* dsegs = at<const HencImage>(page.dev2, desc_at);
    const HencUnit* dchunks = at<const HencUnit>(page.dev2, chunks_at);
    uint32_t *chunk_ff = at<uint32_t>(page.dev2, ff_at), *chunk_out = at<uint32_t>(page.dev2, cout_at), *len = at<uint32_t>(page.dev2, len_at);
    unsigned long long* foff = at<unsigned long long>(page.dev2, foff_at);
    page.in_flight = true;
    if (mark(5) != hipSuccess || hipMemcpyAsync(d2, page.pinned2.data(), upload2, hipMemcpyHostToDevice, stream) != hipSuccess ||
        launch_henc_zero(d2 + raw_at, raw_total, stream) != 0 || mark(6) != hipSuccess ||
        launch_lenc_write(dimages, dunits, (int)units.size(), dsegs, at<const uint32_t>(page.dev1, offsets_at), stream) != hipSuccess ||
        mark(7) != hipSuccess || launch_henc_count(dsegs, dchunks, (int)nchunks, chunk_ff, stream, restart) != 0 ||
        launch_henc_layout(dsegs, (int)n, chunk_ff, chunk_out, len, foff, stream) != 0 || mark(8) != hipSuccess ||
        launch_henc_expand(dsegs, dchunks, (int)nchunks, chunk_out, len, foff, direct ? page.out.data() : d2 + arena_at, stream, restart) != 0 ||
        mark(9) != hipSuccess || hipMemcpyAsync(page.pinned2.data() + len_at, len, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(page.pinned2.data() + foff_at, foff, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        (!direct && hipMemcpyAsync(page.out.data(), d2 + arena_at, arena_cap, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
        mark(10) != hipSuccess || hipEventRecord(page.done, stream) != hipSuccess)
        return fail();
    page.len_at = len_at;
    page.foff_at = foff_at;
    last_page_ = page_index;
    gpu_images_ = (int32_t)n;
    bit_buffer_bytes_ = raw_total;
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t LosslessEncodeBatch::bitstream(int index, const uint8_t** data, size_t* length)
{
    if (last_page_ < 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    Page& page = *pages_[last_page_];
    if (index < 0 || (size_t)index >= page.slot.size() || page.slot[(size_t)index] < 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (page.in_flight) {
        if (hipEventSynchronize(page.done) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        page.in_flight = false;
    }
    const int k = page.slot[(size_t)index];
    *data = page.out.data() + at<const unsigned long long>(page.pinned2, page.foff_at)[k];
    *length = at<const uint32_t>(page.pinned2, page.len_at)[k];
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t LosslessEncodeBatch::stage_times(float ms[kStages])
{
    if (last_page_ < 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    Page& page = *pages_[last_page_];
    if (hipEventSynchronize(page.mark[kStages]) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    for (int k = 0; k < kStages; k++)
        if (hipEventElapsedTime(&ms[k], page.mark[k], page.mark[k + 1]) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

}  // namespace hipjpeg
