// encoder_core.h -- host-side planning, launch and entropy stage of one encode batch
// (counterpart of decoder_core.h; reference flow extensions/nvjpeg/cuda_encoder.cpp:284-396).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/hipjpeg.h"
#include "coefficient_kernels.h"
#include "encode_layout.h"
#include "entropy_encode.h"
#include "gpu_huffman_encode.h"
#include "staging.h"
#include "transcode_core.h"
#include "transcode_kernels.h"

namespace hipjpeg {

struct PlannedEncode {
    hipjpegStatus_t status = HIPJPEG_STATUS_SUCCESS;
    EncodeGeometry geom;
    hipjpegEncodeParams_t params{};
    uint16_t qlum[64], qchr[64];
    size_t coef_offset[3] = {0, 0, 0};  // byte offsets inside the coefficient area
    std::vector<uint8_t> bitstream;          // host entropy coder's output
    const uint8_t* gpu_bitstream = nullptr;  // GPU entropy coder's output (inside the batch's pinned arena), or null
    size_t gpu_bitstream_len = 0;
    const uint8_t* file() const { return gpu_bitstream ? gpu_bitstream : bitstream.data(); }
    size_t file_size() const { return gpu_bitstream ? gpu_bitstream_len : bitstream.size(); }
};

// Lossless transcode: a picture given by its geometry, quantization tables and coding parameters instead of pixels; its coefficients
// lie in HBM in the decoder's layout.  status != SUCCESS: the image has no source (it keeps that status and gets no file).
struct CoefficientPicture {
    hipjpegStatus_t status = HIPJPEG_STATUS_SUCCESS;
    TranscodePicture picture;        // the OUTPUT picture (transcode_turn)
    unsigned turn = 0;               // kTurn* bits: where its blocks come from; 0 = the source's own places
    TranscodeOrigin origin;          // block origin per component in the source's grid (transcode_crop)
    std::vector<uint8_t> markers;    // marker segments to go behind APP0 (transcode_markers), usually none
    hipjpegEncodeParams_t params{};  // restart_interval, optimized_huffman, progressive; the rest is not read
};

// Flavours of the forward kernel, in the order their unit lists lie in the units table.
enum EncodeFlavour {
    kFwdOneLane,                                              // one lane per block, any input (forward_kernel)
    kFwdPair420, kFwdPair422, kFwdPair444,                    // forward_pair_kernel on interleaved RGB / BGR
    kFwdPlanes,                                               // planar YCbCr: one lane per real block of each component
    kFwdPlanarPair420, kFwdPlanarPair422, kFwdPlanarPair444,  // forward_pair_kernel on planar RGB / BGR
    kNumFwdFlavours
};

class EncodeBatch {
public:
    EncodeBatch(int device_id, const MemoryHooks* hooks);
    ~EncodeBatch();
    // Parse params, lay out device memory, upload descriptors and launch the forward kernel (asynchronous on `stream`).
    hipjpegStatus_t device_stage(const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params, int n, hipjpegStatus_t* statuses,
                                 void* stream);
    hipjpegStatus_t relaunch(void* stream);
    // Lossless transcode, in place of device_stage(): plans picture i from pics[i], reserves the coefficient area and lets
    // coef_relayout_kernel (pictures with neither turn nor origin) and coef_transform_kernel (the turned ones and those cropped at an origin), one launch each, fill it from `src`
    // (the DecodeImage table of the batch that decoded the same pictures, same indices) on `stream`.  Blocks until the kernel's range flags are back: an image with a coefficient outside jchuff.c's limits becomes
    // UNSUPPORTED before any coder sees it.  route_entropy() / entropy_stage() follow as after device_stage().
    hipjpegStatus_t coefficient_stage(const CoefficientPicture* pics, int n, const DecodeImage* src, void* stream);
    // Coefficient tensors (hipjpegEncodeCoefficientsBatch), the sibling of coefficient_stage() whose source is the caller's memory:
    // planes[i] (checked by the caller: pointers, alignment, pitch against pics[i]'s real area; turn and origin of pics[i] are not read)
    // in the public layout of include/hipjpeg.h; coef_import_kernel (coefficient_kernels.hip) fills the coefficient area, queued on
    // `stream` behind whatever produced the planes there.  Blocks for the range flags as coefficient_stage() does.
    hipjpegStatus_t import_stage(const CoefficientPicture* pics, const hipjpegCoefficientPlanes_t* planes, int n, void* stream);
    uint64_t relayout_blocks() const { return relayout_blocks_; }  // blocks the last coefficient_stage() moved
    // Pixels to coefficient tensors (hipjpegPixelsToCoefficientsBatch), behind device_stage() on the same stream: checks planes[i] against
    // image i's real block area (coefficients_core.h coefficient_planes_ok; a failing image gets that status and is left out), uploads
    // the CoefPlane table and the relayout units and queues coef_from_coder_kernel (coefficient_kernels.hip): the coder's layout to the
    // caller's planes, real blocks only, for every image whose status is SUCCESS.  Nothing blocks.
    hipjpegStatus_t planes_stage(const hipjpegCoefficientPlanes_t* planes, hipjpegStatus_t* statuses, void* stream);
    uint64_t planes_blocks() const { return planes_blocks_; }  // blocks the last planes_stage() moved
    // Coefficients D2H (on the stream used by device_stage), wait.
    hipjpegStatus_t fetch_coefficients();
    // Decides who entropy-codes each planned image: with gpu_huffman the GPU coder (blocking) takes every image it can -- Annex-K
    // or optimized tables or progressive output; with a restart interval baseline images under gpu_restart and progressive ones under
    // gpu_progressive_restart -- and the rest is flagged for the host coder (every planned image without gpu_huffman).  Fetches the coefficients when the host coder has anything to do.
    hipjpegStatus_t route_entropy(bool gpu_huffman, bool gpu_restart = false, bool gpu_progressive_restart = false);
    // Host coder: Huffman + markers for image i when route_entropy() left it to the host; otherwise nothing.  Thread-safe for distinct i.
    void entropy_stage(int i);
    int host_images() const { return host_images_; }  // images route_entropy() left to the host coder
    uint64_t gpu_entropy_images() const { return gpu_entropy_images_; }
    int size() const { return (int)images_.size(); }
    PlannedEncode& image(int i) { return images_[i]; }
    const int16_t* host_coef(int i, int c) const;
    int num_units() const { return (int)units_.size(); }
    uint64_t pixel_bytes() const { return pixel_bytes_; }
    uint64_t coef_bytes() const { return coef_bytes_; }

private:
    int device_id_;
    // ---- device_stage(): per-image checks and descriptors, unit lists, layout of the descriptor arena, device pointers
    void prepare(int i, const hipjpegEncodeInput_t& in, const hipjpegEncodeParams_t& p);
    void add_units(int i, int fmt);
    void layout();
    hipjpegStatus_t reserve();
    void bind_pointers();
    Buffer pinned_desc_, device_, pinned_coef_;
    Buffer planes_pinned_, planes_device_;  // planes_stage(): CoefPlane[4 n] | RelayoutUnit[]
    uint64_t planes_blocks_ = 0;
    std::vector<PlannedEncode> images_;
    std::vector<EncodeImage> desc_;
    std::vector<EncodeUnit> units_;  // every tile of the batch, grouped by flavour
    std::vector<EncodeUnit> unit_lists_[kNumFwdFlavours];
    size_t unit_first_[kNumFwdFlavours] = {};
    // Descriptor arena, pinned and mirrored on the device at the same offsets: EncodeImage[] | EncodeUnit[] (the upload, [0, coef))
    // || (device only) the coefficients, which pinned_coef_ receives at offset 0.
    // (coefficient_stage(): relayout units and one range-flag word per image ride in the upload, the flags as zeros)
    struct EncodeStaging {
        size_t desc, units, relayout, flags, planes, coef, total;
    } staging_{};
    // coefficient_stage() and import_stage() are one plan: `planes` says where the blocks come from
    hipjpegStatus_t coefficient_fill(const CoefficientPicture* pics, int n, const DecodeImage* src, const hipjpegCoefficientPlanes_t* planes, void* stream);
    std::vector<CoefPlane> coef_planes_;  // import_stage(): four records per image (rides in the upload); empty otherwise
    std::vector<RelayoutUnit> relayout_units_;  // the units of the pictures that stay as they are, then those of the turned / cropped ones
    // per image: marker segments for the header writers of every coding route (coefficient_stage(); empty otherwise).  Not a PlannedEncode
    // field, for the reason given at host_coder_.
    std::vector<std::vector<uint8_t>> markers_;
    const std::vector<uint8_t>* markers_of(int i) const { return markers_[(size_t)i].empty() ? nullptr : &markers_[(size_t)i]; }
    size_t identity_units_ = 0;
    uint64_t relayout_blocks_ = 0;
    size_t coef_total_ = 0;
    uint64_t pixel_bytes_ = 0, coef_bytes_ = 0;
    void* stream_ = nullptr;
    void* event_ = nullptr;
    bool launched_ = false, fetched_ = false;
    // route_entropy(): per image, the host coder still has to code it.  Not a PlannedEncode field: the host coder's threads append
    // to their own record's bitstream next to the neighbouring record's geometry, and a record that grows slows them down.
    std::vector<char> host_coder_;
    int host_images_ = 0;

    // ---- gpu_entropy_stage(): a file is a run of segments (header bytes, then entropy-coded data): a baseline file is one
    // segment, a progressive file one per scan.  Phase 1 is the flavour's own and ends with every segment's total bits on the
    // host; phase 2 (henc_chunks, henc_assemble, henc_collect) is shared, runs once per flavour that has images and ends with the
    // file sizes on the host.  Everything else is queued on the stream the forward kernel ran on.
    struct SegmentPlan;  // what phase 1 hands to phase 2
    struct HencPlan;     // SegmentPlan and what phase 1 of baseline output hands on
    struct PencPlan;     // the same for progressive output
    // One flavour's memory: phase-1 and phase-2 device arenas, pinned staging, and the finished files.  The files of one flavour
    // stay in `out` while the other flavour's images of the same batch are coded.
    struct HencArenas {
        explicit HencArenas(const MemoryHooks* hooks)
            : dev(Buffer::kDevice, hooks), dev2(Buffer::kDevice, hooks), pinned(Buffer::kPinned, hooks), out(Buffer::kPinned, hooks) {}
        Buffer dev, dev2, pinned, out;
    };
    hipjpegStatus_t gpu_entropy_stage(bool gpu_restart, bool gpu_progressive_restart);
    void henc_choose(HencPlan& p, PencPlan& q, bool gpu_restart, bool gpu_progressive_restart);
    // baseline output, Annex-K or optimized tables: one host round trip more when any image wants tables of its own
    void henc_describe(HencPlan& p);
    hipjpegStatus_t henc_stage_phase1(HencPlan& p);
    hipjpegStatus_t henc_histograms(HencPlan& p);
    hipjpegStatus_t henc_lengths(HencPlan& p);
    // progressive output (progressive_encode.h): always that round trip -- the symbol counts of every scan, for the per-scan
    // optimal tables -- and a segment's header is the scan's tables and SOS
    void penc_describe(PencPlan& q);
    hipjpegStatus_t penc_statistics(PencPlan& q);
    hipjpegStatus_t penc_lengths(PencPlan& q);
    // phase 2; `write` queues the flavour's kernel that fills the segments' bit buffers
    void henc_chunks(SegmentPlan& p, const HencArenas& a);
    template <class Write>
    hipjpegStatus_t henc_assemble(SegmentPlan& p, HencArenas& a, Write write, bool* direct, bool restart = false);
    hipjpegStatus_t henc_collect(SegmentPlan& p, HencArenas& a, bool direct);
    HencArenas henc_, penc_;
    uint64_t gpu_entropy_images_ = 0;
};

// (subsampling_factors() and picture_setup(): entropy_encode.h, with the geometry and the tables they fill)
EntropyEncodeOptions entropy_options(const hipjpegEncodeParams_t& p);

}  // namespace hipjpeg
