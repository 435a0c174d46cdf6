// decoder_core.h -- host-side planning, staging and launch of one decode batch.
//
// A DecodeBatch owns: a pinned staging area [DecodeImage[] | WorkUnit tables | coefficient blocks], its device
// mirror (same offsets, one hipMemcpyAsync), and a device-only arena for intermediate chroma planes.  It is the
// MI355X counterpart of the reference's per-thread {pinned buffer, device buffer, stream} resources
// (extensions/nvjpeg/cuda_decoder.h:54-75), but sized for a whole batch so the device stage is one launch per kernel.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/hipjpeg.h"
#include "coefficient_kernels.h"
#include "device_layout.h"
#include "decode_kernels.h"
#include "gpu_huffman.h"
#include "progressive_gpu.h"
#include "jpeg_syntax.h"
#include "staging.h"
#include "thread_pool.h"

namespace hipjpeg {

enum KernelVariant { kVarGray = 0, kVar11 = 1, kVar21 = 2, kVar22 = 3, kVar12 = 4, kNumLumaVariants = 5 };

// A work-unit table and the byte offset it was staged at (the kernels read it from the device mirror there).
struct UnitList {
    std::vector<WorkUnit> units;
    size_t offset = 0;
};

struct PlannedImage {
    FrameInfo frame;
    hipjpegStatus_t status = HIPJPEG_STATUS_SUCCESS;
    const uint8_t* data = nullptr;
    size_t size = 0;
    size_t coef_offset[4] = {0, 0, 0, 0};  // byte offset of component c inside the staging area
    int variant = -1;                      // KernelVariant, or -1 = generic colour path, -2 = planes-to-output only, -3 = CMYK / YCCK, -5 = scaled
    // Scaled decode (hipjpegDecodeBatchSetScales): scale_k = libjpeg's min_DCT_scaled_size = 8 / denominator, 8 = full size; scaled_size[c] =
    // component c's DCT_scaled_size.  pic_w x pic_h is the picture the pixel kernels write (the frame's size, or the scaled one): outputs,
    // pitches and transforms are judged against it.  The entropy stage and the coefficient layout know nothing of the scale.
    int scale_k = 8, scaled_size[4] = {8, 8, 8, 8};
    int pic_w = 0, pic_h = 0;
    uint32_t coef_or[4] = {0, 0, 0, 0};    // OR of |coefficient| per component (from the entropy stage)
    uint32_t ac_bound[4] = {32768, 32768, 32768, 32768};  // upper bound of |AC coefficient| per component (packed IDCT pass 1 decision); default: any int16, -32768 included
    // GPU entropy decoding (flag HIPJPEG_FLAG_GPU_HUFFMAN and an eligible stream): the host only stages the scans
    bool gpu_entropy = false;
    // sequential: every scan is a HuffImage of its own, huff_index .. huff_index + huff_count - 1 (scan order)
    int huff_index = -1, huff_count = 0;
    size_t tables_offset = 0;    // staging offset of the expanded tables (progressive: all scans' tables)
    bool has_transform = false;  // region of interest and/or EXIF orientation (geometry pass)
    hipjpegTransform_t transform = {0, 0, 0, 0, 1};
    int xform_index = -1;
    size_t pool_words = 0;      // lookup-table entries of the picture (GPU entropy path; sequential: the largest scan's)
    struct SeqScan {             // one scan of a sequential picture on the GPU entropy stage
        size_t raw_offset = 0;       // staged copy of the scan's entropy-coded bytes
        size_t stream_offset = 0;    // destuffed stream (device-only scratch)
        size_t tables_offset = 0;    // the scan's expanded tables (staging area)
        size_t pool_words = 0;
        uint32_t first_chunk = 0;    // first destuff chunk (batch-wide numbering)
        size_t boundary_offset = 0;  // restart boundaries + per-subsequence boundary index (staging area)
        uint32_t num_boundaries = 0;
        size_t block_pos_offset = 0;  // bytes into the block-position scratch
        size_t dc_diff_offset = 0;    // bytes into the DC-difference scratch
        uint32_t stream_bytes = 0;
    } seq[4];
    size_t dc_plane_offset[4] = {0, 0, 0, 0};  // bytes into the DC-difference scratch: compact DC planes per component
    uint32_t stream_bytes = 0;   // entropy-coded bytes of all scans
    // the FUSED kernel builds decode a picture from one HuffImage whose slots are the frame's components (one scan, frame order)
    bool fused_layout = true;
    // progressive scans on the GPU entropy stage (progressive_gpu_core.h): gpu_entropy is set as well (device-only coefficient
    // arena, compact DC planes); every scan has a HuffImage of its own for the destuff kernels
    bool gpu_prog = false;
    bool sparse = false;        // host entropy stage wrote the picture's zero-run-compressed stream (entropy_decode.h) instead of dense blocks
    size_t host_coef_offset = 0, host_coef_bytes = 0;  // where this picture's host-decoded coefficients (sparse stream or dense blocks) landed
    bool input_pinned = false;  // the caller's bitstream memory is page-locked: the scan's bytes are fetched from there, no staging copy
    const uint8_t* input_device_view = nullptr;  // ... `data` as the device addresses it (hipPointerGetAttributes)
    int prog_index = -1;               // index into the ProgImage array
    uint32_t prog_huff_first = 0;      // HuffImage index of scan 0, relative to the first progressive one
    size_t prog_raw_offset[kProgMaxScans] = {0};     // staged copy of each scan's entropy-coded bytes (staging area)
    size_t prog_stream_offset[kProgMaxScans] = {0};  // destuffed streams (device-only scratch)
    uint32_t prog_first_chunk[kProgMaxScans] = {0};
    size_t prog_pos_offset[kProgMaxScans] = {0};     // block positions of the AC scans (device-only scratch)
    // ... every scan of which has a restart interval (HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS, progressive_interval_core.h): gpu_prog is
    // set as well; the interval kernels stand in for the walk
    bool gpu_prog_intervals = false;
    size_t prog_start_offset[kProgMaxScans] = {0};   // interval starts of each scan (staging area, the sequential path's boundaries region)
    size_t prog_hist_offset[4] = {0, 0, 0, 0};       // non-zero bitmaps of a component with several AC scans (device-only scratch)
};

class DecodeBatch {
public:
    DecodeBatch(int device_id, const MemoryHooks* hooks);
    ~DecodeBatch();

    // Phase 0: parse headers, choose kernels, lay out staging memory.  Per-image problems land in statuses[i].
    // `formats` (optional) gives one output format per image; otherwise `format` applies to all.
    // `scale_denoms` (optional) gives one denominator per image: 1 (full size), 2, 4 or 8; see hipjpegDecodeBatchSetScales.
    hipjpegStatus_t plan(const uint8_t* const* data, const size_t* lengths, int n, const hipjpegOutput_t* outputs,
                         hipjpegOutputFormat_t format, unsigned flags, hipjpegStatus_t* statuses,
                         const hipjpegOutputFormat_t* formats = nullptr, ForkJoinPool* pool = nullptr,
                         const hipjpegTransform_t* transforms = nullptr, const int32_t* scale_denoms = nullptr);
    // Lossless transcode (hipjpegTranscodeBatch): plans the entropy stage alone -- no outputs, no pixel kernels, no geometry; the
    // coefficients stay in HBM in the decoder's layout, host-decoded pictures as dense blocks.  Of `flags` only
    // HIPJPEG_FLAG_GPU_HUFFMAN counts.  Sources the coder cannot take (transcode_core.h transcode_picture) are UNSUPPORTED.
    // Then entropy_stage() per image, finalize(), transfer() and launch(stream, 3) as for any batch.
    // `params` (per image, or nullptr): HIPJPEG_TRANSCODE_GRAYSCALE waives the chroma rules for that image.
    // `any_frame` (hipjpegDecodeCoefficientsBatch): every frame the entropy stage decodes is taken, whatever the coder thinks of it.
    hipjpegStatus_t plan_coefficients(const uint8_t* const* data, const size_t* lengths, int n, unsigned flags, hipjpegStatus_t* statuses,
                                      ForkJoinPool* pool, const hipjpegTranscodeParams_t* params = nullptr, bool any_frame = false);
    // Coefficient tensors to pixels (hipjpegCoefficientsToPixelsBatch): plan() for pictures given by infos[i] + planes[i] instead of files.
    // The frame is coefficients_core.h's coefficient_frame(); kernel variants, quantizers, outputs, transforms and unit tables are
    // plan()'s own.  There is no entropy stage: every image's coefficients live in the device-only part of the arena, where
    // import_tensors() puts them.  Of `flags` HIPJPEG_FLAG_GPU_HUFFMAN is ignored.  Then finalize(), transfer(), import_tensors(),
    // launch(); entropy_stage() does nothing for such a batch.
    hipjpegStatus_t plan_tensors(const hipjpegCoefficientInfo_t* infos, const hipjpegCoefficientPlanes_t* planes, int n, const hipjpegOutput_t* outputs,
                                 hipjpegOutputFormat_t format, unsigned flags, hipjpegStatus_t* statuses, ForkJoinPool* pool,
                                 const hipjpegTransform_t* transforms = nullptr);
    // Behind plan_tensors() ... transfer(), which took the CoefPlane table and the relayout units up with the descriptors: queues
    // coef_to_decoder_kernel (coefficient_kernels.hip) on `stream`: the caller's planes into the arena in the decoder's layout, zeros in
    // the blocks of the MCU-padded grid outside the real area.  Images with a status other than SUCCESS are left out.  Nothing blocks.
    hipjpegStatus_t import_tensors(void* stream);
    uint64_t imported_blocks() const { return imported_blocks_; }  // real blocks the last import_tensors() moved
    // Coefficient tensors (hipjpegDecodeCoefficientsBatch), behind plan_coefficients() ... launch(stream, 3): coef_export_kernel
    // (coefficient_kernels.hip) copies the real blocks of every image that decoded into planes[i] (checked by the caller: pointers,
    // alignment, pitch), natural order, queued on `stream`.  Images with a status other than SUCCESS are left out.
    hipjpegStatus_t export_coefficients(const hipjpegCoefficientPlanes_t* planes, void* stream);
    uint64_t exported_blocks() const { return exported_blocks_; }  // blocks the last export_coefficients() moved
    // The batch's DecodeImage table as the kernels see it (valid after transfer()).
    const DecodeImage* device_descriptors() const { return at<const DecodeImage>(device_, staging_.desc); }
    // GPU entropy stage only for images of MORE than this many pixels (width x height); smaller ones keep the host Huffman decoder.
    // The reference's nvJPEG plugin has the same switch between its HYBRID and GPU_HYBRID backends (`hybrid_huffman_threshold`,
    // extensions/nvjpeg/cuda_decoder.cpp:188-209, 512-521; default 1000 x 1000 there).  Default here 0: every eligible stream goes to
    // the GPU -- measured faster from 224 x 224 upwards.
    void set_gpu_entropy_threshold(uint64_t pixels) { gpu_entropy_min_pixels_ = pixels; }
    // Between plan() and entropy_stage(): give up image i (e.g. the caller's image descriptor is too small for it).
    void reject(int i, hipjpegStatus_t st)
    {
        if (i >= 0 && i < (int)images_.size() && images_[i].status == HIPJPEG_STATUS_SUCCESS) images_[i].status = st;
    }
    // Size of what image i writes into the caller's buffer: width x height after region of interest and orientation.
    void output_size(int i, int* w, int* h) const;
    // Phase 1: entropy-decode image i into the pinned staging area.  Thread-safe for distinct i.
    void entropy_stage(int i);
    // Phase 1b: after every entropy_stage returned: final per-image flags, drop failed images from the unit tables.
    void finalize(hipjpegStatus_t* statuses);
    // Phase 2: one async H2D copy of descriptors + coefficients.
    // kernels_on_other_stream: the copy is issued on a stream of its own; launch() then makes the kernels' stream wait for
    // it on the device (copy of batch n+1 overlaps the kernels of batch n)
    hipjpegStatus_t transfer(void* stream, bool kernels_on_other_stream = false);
    // Phase 3: kernel launches.  which = -1: all; 0 idct_plane, 1 luma_color (every variant), 2 generic_color,
    // 3 GPU entropy stage (blocks until its result status has been read back).
    // entropy_stream (optional): a second stream for the GPU entropy stage, see launch() in decoder_core.cpp
    hipjpegStatus_t launch(void* stream, int which = -1, void* entropy_stream = nullptr);
    // After launch(): waits for `stream` and settles the GPU entropy stage's verdicts (see decoder_core.cpp); image(i).status
    // is final afterwards.  A no-op for batches without GPU-decoded streams.
    hipjpegStatus_t resolve(void* stream);
    // Blocks until the kernels of the last launch() have finished (the event recorded behind them).
    hipjpegStatus_t wait_done();
    void* last_stream() const { return last_stream_; }
    int gpu_entropy_images() const { return seq_gpu_images_ + (int)prog_to_image_.size(); }
    int last_sync_launches() const { return last_sync_launches_; }
    int host_fallback_images() const { return host_fallback_images_; }  // GPU-entropy images the host decoder took over in resolve()
    bool has_progressive() const { return !prog_to_image_.empty(); }
    int interval_images() const { return (int)(prog_to_image_.size() - prog_walk_images_); }  // progressive images on the interval kernels
    // ... of which the kernels flagged (a stream they could not vouch for) and the host decoder took over in resolve()
    int interval_takeover_images() const { return interval_takeover_images_; }
    uint64_t stream_bytes() const { return stream_bytes_total_; }
    // images of the current batch whose bitstream went to the device from the caller's own (pinned) memory
    int zero_copy_images() const { return zero_copy_images_; }
    uint64_t h2d_bytes() const { return h2d_used_; }  // bytes the current batch's transfer() copies to the device
    int sparse_images() const { return (int)std::count_if(images_.begin(), images_.end(), [](const PlannedImage& im) { return im.sparse; }); }
    void flavour_units(int32_t* plane_units, int32_t luma_units[kNumLumaLayouts]) const { unit_counts(true, plane_units, luma_units); }
    int fused_units() const;  // work units of the FUSED kernel builds (blocks decoded inside the pixel kernels) in the current batch

    int size() const { return (int)images_.size(); }
    const PlannedImage& image(int i) const { return images_[i]; }
    void stats(int32_t num_units[3], uint64_t* coef_bytes, uint64_t* output_bytes) const;

private:
    int device_id_;
    ForkJoinPool* pool_ = nullptr;  // the pool plan() was given (resolve() decodes handed-over images on it)
    uint64_t gpu_entropy_min_pixels_ = 0;

    // ---- plan(): per-image checks and descriptors, sizes, layout of the arenas, device pointers
    struct PlanArgs;  // plan()'s arguments as prepare() reads them
    struct Sizing;    // what the per-image sizing adds up
    hipjpegStatus_t plan_attempts(const PlanArgs& a, int n, hipjpegStatus_t* statuses);
    bool coef_only_ = false;  // the batch was planned by plan_coefficients()
    bool tensor_source_ = false;  // the batch was planned by plan_tensors()
    const hipjpegCoefficientPlanes_t* tensor_planes_ = nullptr;  // plan_tensors(): the caller's planes, read until finalize() returns
    std::vector<CoefPlane> tensor_table_;      // plan_tensors(): four records per image and the units of coef_to_decoder_kernel,
    std::vector<RelayoutUnit> tensor_units_;   // built by finalize(), staged with the other tables
    void build_tensor_units();
    uint64_t imported_blocks_ = 0;
    hipjpegStatus_t plan_once(const PlanArgs& a, int n, hipjpegStatus_t* statuses);
    void prepare(int i, const PlanArgs& a);
    bool pitch_ok(int i, const hipjpegOutput_t& out, OutFormat fmt) const;
    void demote_progressive_lds();
    void size_image(int i, Sizing& s);
    void layout(const Sizing& s);
    hipjpegStatus_t reserve(const Sizing& s);
    void bind_pointers(const Sizing& s);
    Buffer pinned_, device_, planes_;
    Buffer export_pinned_, export_device_;  // export_coefficients(): CoefPlane[4 n] | RelayoutUnit[]
    uint64_t exported_blocks_ = 0;
    // Staging area, pinned and mirrored on the device at the same offsets:  descriptors | work units | entropy descriptors, units,
    // tables | staged bitstreams [streams, coef) | coefficients of host-decoded images  ||  (device only from h2d_bytes) coefficients of
    // GPU-decoded images.  The pinned side keeps 256 spare bytes and verdict_bytes() behind h2d_bytes (entropy_launch_args).
    struct StagingLayout {
        size_t desc, units, huff_desc, huff_units, huff_pairs, huff_wunits, huff_dc_units, huff_chunk_units, huff_drops, xform_desc, xform_units,
            prog_desc, prog_units, prog_iv_desc, prog_iv_units, tensor_planes, tensor_units, tables, boundaries, streams, coef, h2d_bytes, gpu_coef_begin, total;
    } staging_{};
    // Device-only scratch of the entropy kernels (work_): subsequence states (at 0) | first block indices | change counters | ...
    struct WorkLayout {
        size_t first_block, changed, incoming, tail, dc_diff, block_pos, records, walkers, verdicts, drops, prog_pos, group_sums, streams, total;
    } scratch_{};
    // what resolve() reads of the GPU entropy stage: the convergence counters and one verdict word per sequential HuffImage
    size_t verdict_bytes() const { return (kHuffVerdictCounters + huff_to_image_.size()) * sizeof(unsigned int); }
    Buffer work_;
    std::vector<PlannedImage> images_;
    std::vector<DecodeImage> desc_;  // host copy (device pointers inside)
    // HIPJPEG_FLAG_FAST_IDCT of the batch being planned: the descriptors' qpk hold IFAST multiplier tables and K1 / K2 launch their
    // fast-IDCT flavour; such a batch never takes the FUSED builds (they have no IFAST flavour).  Set by every plan().
    bool fast_idct_ = false;
    uint64_t coef_bytes_ = 0, output_bytes_ = 0;
    // Host-decoded coefficients are handed out of their region [staging_.coef, staging_.h2d_bytes) first come first served while the
    // pool threads decode (a sparse stream's size is known only then): h2d_used_ = what transfer() actually has to copy.
    bool sparse_mode_ = false;
    std::atomic<size_t> host_coef_used_{0};
    size_t h2d_used_ = 0;
    // ---- entropy_stage(), finalize(): unit tables, entropy descriptors, staging of the tables
    void stage_chunk_drops(const ScanHeader& sc, uint32_t first_chunk);
    void build_pixel_units();
    void build_entropy_units();
    void stage_tables();
    void merge_zero_fills();
    void unit_counts(bool plain, int32_t* plane, int32_t luma[kNumLumaLayouts]) const;
    UnitList plane_units_, luma_units_[kNumLumaLayouts][kNumLumaVariants], generic_units_, cmyk_units_, xform_units_;  // luma: [layout of K2][sampling]
    // scaled images: components of DCT_scaled_size 8 have their units in plane_units_ (K1, kToPlane), the others here; then a unit per row
    UnitList reduced_units_, scaled_color_units_;
    // Images of the GPU entropy stage (baseline): their K1 / K2 units go to the FUSED kernel builds, which Huffman-decode the blocks
    // themselves (decode_kernels.hip) -- same unit geometry.  host_taken_: such images the host entropy decoder took over in resolve()
    // (damaged / periodic streams): their coefficients then lie in HBM and the plain builds run for them (launch_taken_pixels).
    UnitList fused_plane_units_, fused_luma_units_[kNumLumaLayouts][kNumLumaVariants];
    bool fused_ = false;
    bool finalized_ = false;
    std::vector<TransformImage> xform_desc_;
    // GPU entropy stage: one HuffImage per scan of the sequential images first, then one per scan of the progressive images
    std::vector<HuffImage> huff_images_;
    std::vector<HuffUnit> huff_units_, huff_dc_units_;
    std::vector<uint32_t> huff_pairs_;  // the first sync launch's workgroups: huff_pair_entry()
    std::vector<int> huff_to_image_;  // sequential HuffImage -> image
    int seq_gpu_images_ = 0;          // sequential images among them
    // blocks of GPU-decoded sequential pictures that no scan codes (padding of a one-component scan's grid): zeroed before the
    // entropy kernels run, as the host decoder leaves them -- {device address, bytes, count, pitch} (count > 1: a 2D fill)
    struct ZeroFill {
        uint8_t* ptr;
        size_t bytes, count, pitch;
    };
    std::vector<ZeroFill> huff_zero_;
    std::vector<HuffUnit> huff_wunits_;       // block kernel: kHuffMcusPerWg MCUs per workgroup
    std::vector<HuffUnit> huff_chunk_units_;  // destuff kernels: one per kDestuffChunk bytes of a scan
    size_t total_subseq_ = 0, max_huff_units_ = 0, max_huff_pairs_ = 0, max_pool_words_ = 0;
    std::atomic<bool> host_drops_missing_{false};  // set by a host task that found a scan without counts: the device counts instead
    // progressive images of the batch
    std::vector<ProgImage> prog_images_;
    std::vector<int> prog_to_image_;
    std::vector<HuffUnit> prog_units_;  // replay kernel: {ProgImage index, component << 28 | first block}
    unsigned prog_slot_words_ = 0;
    // prog_images_ / prog_to_image_ hold the images of the walk first, [0, prog_walk_images_), then those of the interval kernels; the
    // replay kernel takes them all
    size_t prog_walk_images_ = 0;
    std::vector<ProgIntervalImage> prog_iv_images_;  // beside prog_images_[prog_walk_images_ ...]
    std::vector<HuffUnit> prog_iv_units_;            // AC units, then the DC units of DC-scan index 0, 1, ... (image relative to the tail)
    std::vector<size_t> prog_iv_dc_first_;           // prog_iv_units_ index of the first DC unit of index d; one entry more than indices
    uint64_t stream_bytes_total_ = 0;
    // ---- transfer(), launch(), resolve()
    struct EntropyLaunch {
        HuffImage* dimg;
        const HuffUnit *dunits, *dwunits, *ddc;
        unsigned long long *states, *incoming;
        uint32_t* first_block;
        uint16_t* records;       // block-start records of the synchronisation decodes
        const uint16_t* use_records;  // what the position pass copies (nullptr: it walks every subsequence, HIPJPEG_POSITION_PASS=1)
        uint32_t* walkers;            // per sync unit: subsequences the position pass walks
        int32_t* group_sums;
        unsigned int *changed, *host_changed;
        unsigned int* verdicts;      // pinned, behind host_changed's counters: huff_verdict() per HuffImage
        unsigned int* verdicts_out;  // where the stage's last kernel stores counters and verdicts: host_changed itself, or the scratch
        HuffImage* himg;
        unsigned pool_bytes;
        int nunits;
    };
    EntropyLaunch entropy_launch_args();
    bool entropy_write_passes(const EntropyLaunch& L, void* stream);
    hipjpegStatus_t enqueue_gpu_entropy(void* stream);
    hipjpegStatus_t enqueue_progressive(void* stream);
    int launch_pixel_kernels(void* stream, int which);
    int launch_taken_pixels(void* stream, int which);
    void print_progressive_timing(const ProgImage* hprog) const;
    hipjpegStatus_t take_over_on_host(const std::vector<int>& takeover, bool* redo_pixels);
    int zero_copy_images_ = 0;
    std::vector<int> host_taken_;
    void* taken_units_dev_ = nullptr;
    size_t taken_units_cap_ = 0;
    bool entropy_pending_ = false, pixels_launched_ = false, copy_pending_ = false, entropy_done_ = false;
    void* last_stream_ = nullptr;    // stream of the last launch()
    void* copied_event_ = nullptr;   // hipEvent_t: H2D copy issued on a stream other than the kernels'
    void* entropy_event_ = nullptr;  // hipEvent_t: entropy stage finished on its own stream
    void* done_event_ = nullptr;     // hipEvent_t recorded after the last launch that reads this batch's buffers
    bool in_flight_ = false;
    int last_sync_launches_ = 0, host_fallback_images_ = 0, interval_takeover_images_ = 0;
};

// status helpers
hipjpegStatus_t status_from_parse(ParseStatus s);

}  // namespace hipjpeg
