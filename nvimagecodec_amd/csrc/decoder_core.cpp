// decoder_core.cpp -- see decoder_core.h
#include "decoder_core.h"
#include "host_copy.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "coefficients_core.h"
#include "decode_kernels.h"
#include "diagnostics.h"
#include "entropy_decode.h"
#include "gpu_huffman_host.h"
#include "progressive_gpu_host.h"
#include "transcode_core.h"

namespace hipjpeg {

namespace {
// Planes of the caller's buffer and bytes per pixel in each (full-resolution formats; kOutPlanarYUV writes one plane per component).
int out_planes(OutFormat fmt) { return (fmt == kOutInterleavedRGB || fmt == kOutInterleavedBGR || fmt == kOutY) ? 1 : 3; }
int out_bpp(OutFormat fmt) { return (fmt == kOutInterleavedRGB || fmt == kOutInterleavedBGR) ? 3 : 1; }

// Chroma subsampling of each KernelVariant, as launch_luma_color takes it.
constexpr int kLumaHs[kNumLumaVariants] = {0, 1, 2, 2, 1}, kLumaVs[kNumLumaVariants] = {0, 1, 1, 2, 2};

// Where K1 (idct_plane) writes component c: an intermediate plane, the caller's buffer, or nowhere (K2 decodes the luma itself).
enum Route { kRouteNone, kRoutePlane, kRouteOutput };
Route component_route(int variant, OutFormat fmt, int c)
{
    if (variant == -1 || variant == -3 || (variant >= kVar11 && c > 0)) return kRoutePlane;
    if (variant == -2 && (fmt == kOutPlanarYUV || c == 0)) return kRouteOutput;
    return kRouteNone;
}

// HIPJPEG_DEBUG_SYNC=1: synchronise after every launch and report which kernel failed (debug aid only)
bool debug_sync() { static const bool v = getenv("HIPJPEG_DEBUG_SYNC") != nullptr; return v; }

void debug_check(void* stream, const char* what, int n)
{
    if (!debug_sync()) return;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    fprintf(stderr, "[hipjpeg] %s units=%d -> %s\n", what, n, hipGetErrorString(e));
}

bool ensure_event(void** ev)  // a timing-free event, created on first use
{
    hipEvent_t e = nullptr;
    if (!*ev && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) *ev = e;
    return *ev != nullptr;
}
}  // namespace

// Same classification the framework's parser applies (reference src/parsers/jpeg.cpp:70-114).
hipjpegStatus_t status_from_parse(ParseStatus s)
{
    switch (s) {
    case kParseOk: return HIPJPEG_STATUS_SUCCESS;
    case kParseUnsupported: return HIPJPEG_STATUS_UNSUPPORTED;
    case kParseTruncated: return HIPJPEG_STATUS_TRUNCATED;
    default: return HIPJPEG_STATUS_BAD_JPEG;
    }
}

// ---------------------------------------------------------------- DecodeBatch
DecodeBatch::DecodeBatch(int device_id, const MemoryHooks* hooks)
    : device_id_(device_id), pinned_(Buffer::kPinned, hooks), device_(Buffer::kDevice, hooks), planes_(Buffer::kDevice, hooks),
      export_pinned_(Buffer::kPinned, hooks), export_device_(Buffer::kDevice, hooks), work_(Buffer::kDevice, hooks)
{
}

DecodeBatch::~DecodeBatch()
{
    if (taken_units_dev_) (void)hipFree(taken_units_dev_);
    if (copied_event_) (void)hipEventDestroy((hipEvent_t)copied_event_);
    if (entropy_event_) (void)hipEventDestroy((hipEvent_t)entropy_event_);
    if (done_event_) {
        if (in_flight_) (void)hipEventSynchronize((hipEvent_t)done_event_);
        (void)hipEventDestroy((hipEvent_t)done_event_);
    }
}

namespace {

// jddctmgr.c, JDCT_IFAST: the multiplier of quantiser q at natural-order position k, (q * aanscales[k] + 2048) >> 12, as the
// library stores it (IFAST_MULT_TYPE = short for 8-bit samples: a 16-bit table's large products wrap)
uint32_t ifast_multiplier(uint16_t q, int k)
{
    static const int32_t aanscales[64] = {
        16384, 22725, 21407, 19266, 16384, 12873, 8867,  4520,  22725, 31521, 29692, 26722, 22725, 17855, 12299, 6270,
        21407, 29692, 27969, 25172, 21407, 16819, 11585, 5906,  19266, 26722, 25172, 22654, 19266, 15137, 10426, 5315,
        16384, 22725, 21407, 19266, 16384, 12873, 8867,  4520,  12873, 17855, 16819, 15137, 12873, 10114, 6967,  3552,
        8867,  12299, 11585, 10426, 8867,  6967,  4799,  2446,  4520,  6270,  5906,  5315,  4520,  3552,  2446,  1247};
    return (uint32_t)(((int64_t)q * aanscales[k] + 2048) >> 12);
}

// qpk[p][j*4 + i]: the quantisers of rows 2i and 2i+1 at column 4p+j, one per 16-bit half (device_layout.h); IFAST multipliers
// for a fast-IDCT batch
void pack_qpk(const uint16_t* qtab, bool fast_idct, uint32_t qpk[2][16])
{
    for (int pp = 0; pp < 2; pp++)
        for (int j = 0; j < 4; j++)
            for (int r = 0; r < 8; r++) {
                const int k = r * 8 + 4 * pp + j;
                const uint32_t q16 = (fast_idct ? ifast_multiplier(qtab[k], k) : (uint32_t)qtab[k]) & 0xFFFFu;
                uint32_t& pk = qpk[pp][j * 4 + (r >> 1)];
                pk = (r & 1) ? (pk | (q16 << 16)) : q16;
            }
}

// Decide which kernels handle this frame.  Returns false when the layout is outside the decoder's scope.
bool choose_variant(const FrameInfo& f, OutFormat fmt, bool fancy, int* variant)
{
    const bool four = f.color == ColorModel::CMYK || f.color == ColorModel::YCCK;
    if (four ? f.ncomp != 4 : (f.ncomp != 1 && f.ncomp != 3)) return false;
    for (int c = 0; c < f.ncomp; c++)
        if (f.hmax % f.comp[c].h || f.vmax % f.comp[c].v) return false;  // fractional upsampling: libjpeg refuses too
    if (four) {
        // CMYK / YCCK: all four components through planes, then cmyk_color_kernel -- the formats the reference's CPU path
        // produces from such files (extensions/libjpeg_turbo/jpeg_mem.cpp:318-337: I_RGB, I_BGR, P_Y) and their planar twins
        if (fmt == kOutPlanarYUV) return false;
        *variant = -3;
        return true;
    }
    if (fmt == kOutPlanarYUV) {
        *variant = -2;
        return true;
    }
    if (fmt == kOutY) {
        // libjpeg JCS_GRAYSCALE from YCbCr/gray = the luma plane; from an RGB-model JPEG it is a weighted sum (not done here)
        if (f.color == ColorModel::RGB) return false;
        if (f.comp[0].h != f.hmax || f.comp[0].v != f.vmax) return false;
        *variant = -2;
        return true;
    }
    if (f.ncomp == 1) {
        *variant = kVarGray;
        return true;
    }
    const int fx1 = f.hmax / f.comp[1].h, fy1 = f.vmax / f.comp[1].v, fx2 = f.hmax / f.comp[2].h, fy2 = f.vmax / f.comp[2].v;
    const bool luma_full = f.comp[0].h == f.hmax && f.comp[0].v == f.vmax;
    if (luma_full && fx1 == fx2 && fy1 == fy2 && fx1 <= 2 && fy1 <= 2) {
        *variant = fx1 == 1 ? (fy1 == 1 ? kVar11 : kVar12) : (fy1 == 1 ? kVar21 : kVar22);
        return true;
    }
    // Generic path = replication only.  Make sure libjpeg would replicate as well (jdsample.c jinit_upsampler).
    for (int c = 0; c < f.ncomp; c++) {
        int fx = f.hmax / f.comp[c].h, fy = f.vmax / f.comp[c].v;
        bool triangle = fancy && ((fx == 2 && fy == 1 && f.comp[c].samp_w > 2) || (fx == 2 && fy == 2 && f.comp[c].samp_w > 2) ||
                                  (fx == 1 && fy == 2));
        if (triangle) return false;
    }
    *variant = -1;
    return true;
}


// libjpeg's jpeg_calc_output_dimensions (jdmaster.c) for scale 1 / denom: k = min_DCT_scaled_size
int scaled_extent(int extent, int k) { return (int)(((int64_t)extent * k + 7) / 8); }

// A scaled image: every component's DCT_scaled_size (jdmaster.c: doubled from k while the component's group still divides the
// largest one), and whether scaled_color_kernel covers the frame -- one or three components, integral upsampling ratios on the scaled
// groups (jdsample.c refuses the others), no raw planes; `y` as at full size.
bool choose_scaled(const FrameInfo& f, OutFormat fmt, int k, int scaled_size[4])
{
    if (f.color == ColorModel::CMYK || f.color == ColorModel::YCCK || (f.ncomp != 1 && f.ncomp != 3) || fmt == kOutPlanarYUV) return false;
    for (int c = 0; c < f.ncomp; c++) {
        int s = k;
        while (s < 8 && (f.hmax * k) % (f.comp[c].h * s * 2) == 0 && (f.vmax * k) % (f.comp[c].v * s * 2) == 0) s *= 2;
        scaled_size[c] = s;
        const int h_in = f.comp[c].h * s / k, v_in = f.comp[c].v * s / k;
        if (f.hmax % h_in || f.vmax % v_in) return false;
        if (fmt == kOutY && c == 0 && (f.color == ColorModel::RGB || h_in != f.hmax || v_in != f.vmax)) return false;
    }
    return true;
}

}  // namespace

// Largest frame the decoder takes: the reference's CPU path refuses width x height x components >= 2^29 before it allocates
// anything (extensions/libjpeg_turbo/jpeg_mem.cpp:183-196), and a forged SOF of a few hundred bytes must not be able to
// reserve tens of GB of pinned memory for the whole batch.  HIPJPEG_MAX_IMAGE_SAMPLES overrides the bound (tests).
static uint64_t max_image_samples()
{
    static const uint64_t v = [] {
        const char* e = getenv("HIPJPEG_MAX_IMAGE_SAMPLES");
        const unsigned long long x = e ? strtoull(e, nullptr, 10) : 0ull;
        return x ? (uint64_t)x : (uint64_t)1 << 29;
    }();
    return v;
}

// Region of interest / EXIF orientation: normalise, validate (crop semantics of the reference's CPU path,
// extensions/libjpeg_turbo/libjpeg_turbo_decoder.cpp:355-370: the region must lie inside the image)
static hipjpegStatus_t normalise_transform(PlannedImage& im, const hipjpegTransform_t& requested, OutFormat fmt)
{
    const int width = im.pic_w, height = im.pic_h;  // (a scaled image: the region is in scaled-picture coordinates)
    hipjpegTransform_t t = requested;
    if (t.x0 == 0 && t.y0 == 0 && t.x1 == 0 && t.y1 == 0) {
        t.x1 = width;
        t.y1 = height;
    }
    if (t.orientation == 0) t.orientation = 1;
    const bool whole = t.x0 == 0 && t.y0 == 0 && t.x1 == width && t.y1 == height;
    if (t.orientation < 1 || t.orientation > 8 || t.x0 < 0 || t.y0 < 0 || t.x1 > width || t.y1 > height || t.x1 <= t.x0 || t.y1 <= t.y0)
        return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (whole && t.orientation == 1) return HIPJPEG_STATUS_SUCCESS;
    if (fmt == kOutPlanarYUV) return HIPJPEG_STATUS_UNSUPPORTED;  // geometry on subsampled planes is not defined
    im.has_transform = true;
    im.transform = t;
    return HIPJPEG_STATUS_SUCCESS;
}

struct DecodeBatch::PlanArgs {  // plan()'s arguments; give_up: per image, given up after a failed allocation
    const uint8_t* const* data; const size_t* lengths; const hipjpegOutput_t* outputs; hipjpegOutputFormat_t format; unsigned flags;
    const hipjpegOutputFormat_t* formats; const hipjpegTransform_t* transforms; const char* give_up;
    const hipjpegTranscodeParams_t* transcode = nullptr;  // plan_coefficients(): per image, or nullptr
    bool any_frame = false;                               // plan_coefficients(): the coder's rules are not asked
    const hipjpegCoefficientInfo_t* infos = nullptr;      // plan_tensors(): the pictures, in place of data / lengths
    const hipjpegCoefficientPlanes_t* tensors = nullptr;
    const int32_t* scales = nullptr;                      // plan(): one denominator per image, or nullptr
};

// What the per-image sizing adds up, in bytes unless noted; every region is carved in image order.
struct DecodeBatch::Sizing {
    explicit Sizing(int n) : plane_off((size_t)n * 4, (size_t)-1) {}
    size_t units = 0, xform_units = 0;  // WorkUnit slots of the pixel kernels and of the geometry pass
    Carve planes;                       // planes_: intermediate component planes and pictures of the geometry pass
    std::vector<size_t> plane_off, xform_plane_off;  // per image x component ((size_t)-1: no plane); per TransformImage plane, in order
    // GPU entropy stage: staging area (scans, tables, boundaries), device-only scratch (streams, DC values, positions), chunks (a count)
    Carve raw, pools, boundaries, streams, blocks, block_pos, prog_pos, chunks;
    size_t subseq = 0, huff_wunits = 0, prog_units = 0, prog_scans = 0, prog_iv_units = 0;
    size_t tensor_units = 0;  // plan_tensors(): RelayoutUnit slots of coef_to_decoder_kernel

    // One scan: its staged bytes (padded, see entropy_stage), its destuffed stream, its destuff chunks.  Returns the stream's capacity.
    size_t scan(const ScanHeader& sc, size_t* raw_offset, size_t* stream_offset, uint32_t* first_chunk)
    {
        const size_t raw_len = sc.data_end - sc.data_begin, cap = align_up(destuffed_capacity(sc), 64);
        *raw_offset = raw.take(align_up(raw_len, 16) + 16, 1);
        *stream_offset = streams.take(cap, 1);
        *first_chunk = (uint32_t)chunks.take((raw_len + kDestuffChunk - 1) / kDestuffChunk, 1);
        return cap;
    }
};

hipjpegStatus_t DecodeBatch::plan(const uint8_t* const* data, const size_t* lengths, int n, const hipjpegOutput_t* outputs,
                                  hipjpegOutputFormat_t format, unsigned flags, hipjpegStatus_t* statuses,
                                  const hipjpegOutputFormat_t* formats, ForkJoinPool* pool, const hipjpegTransform_t* transforms,
                                  const int32_t* scale_denoms)
{
    pool_ = pool;
    coef_only_ = false;
    tensor_source_ = false;
    PlanArgs a{data, lengths, outputs, format, flags, formats, transforms, nullptr};
    a.scales = scale_denoms;
    return plan_attempts(a, n, statuses);
}

hipjpegStatus_t DecodeBatch::plan_tensors(const hipjpegCoefficientInfo_t* infos, const hipjpegCoefficientPlanes_t* planes, int n,
                                          const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags, hipjpegStatus_t* statuses,
                                          ForkJoinPool* pool, const hipjpegTransform_t* transforms)
{
    if (n > 0 && (!infos || !planes)) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    pool_ = pool;
    coef_only_ = false;
    tensor_source_ = true;
    tensor_planes_ = planes;
    PlanArgs a{nullptr, nullptr, outputs, format, flags & ~HIPJPEG_FLAG_GPU_HUFFMAN, nullptr, transforms, nullptr};
    a.infos = infos;
    a.tensors = planes;
    return plan_attempts(a, n, statuses);
}

hipjpegStatus_t DecodeBatch::plan_coefficients(const uint8_t* const* data, const size_t* lengths, int n, unsigned flags, hipjpegStatus_t* statuses,
                                               ForkJoinPool* pool, const hipjpegTranscodeParams_t* params, bool any_frame)
{
    pool_ = pool;
    coef_only_ = true;
    tensor_source_ = false;
    return plan_attempts(PlanArgs{data, lengths, nullptr, HIPJPEG_OUTPUT_RGBI, flags & (HIPJPEG_FLAG_GPU_HUFFMAN | HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS), nullptr, nullptr, nullptr, params, any_frame}, n,
                         statuses);
}

hipjpegStatus_t DecodeBatch::plan_attempts(const PlanArgs& a, int n, hipjpegStatus_t* statuses)
{
    // An allocation that fails costs only the images that made the arenas grow: the biggest remaining image is given up
    // (ALLOC_FAILED) and the layout is computed again without it.
    std::vector<char> give_up((size_t)std::max(n, 0), 0);
    PlanArgs args = a;
    args.give_up = give_up.data();
    for (int attempt = 0;; attempt++) {
        const hipjpegStatus_t st = plan_once(args, n, statuses);
        if (st != HIPJPEG_STATUS_ALLOC_FAILED || attempt >= 16) return st;
        int worst = -1;
        size_t worst_bytes = 0;
        for (int i = 0; i < n; i++) {
            if (images_[i].status != HIPJPEG_STATUS_SUCCESS) continue;
            const size_t b = images_[i].frame.total_blocks() * 128 + (size_t)images_[i].frame.width * images_[i].frame.height;
            if (b >= worst_bytes) {
                worst_bytes = b;
                worst = i;
            }
        }
        if (worst < 0) return st;
        give_up[worst] = 1;
    }
}

hipjpegStatus_t DecodeBatch::plan_once(const PlanArgs& a, int n, hipjpegStatus_t* statuses)
{
    if (n < 0 || (n > 0 && (((!a.data || !a.lengths) && !a.infos) || (!a.outputs && !coef_only_)))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if ((int)a.format < 0 || (int)a.format > (int)HIPJPEG_OUTPUT_YUV_PLANAR) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    ScopedRange range("hipjpeg plan (parse headers, lay out staging)");
    fault_point("plan");
    finalized_ = false;
    host_drops_missing_.store(false, std::memory_order_relaxed);
    // (every element is reset by its own prepare() below -- on the pool: a batch of a thousand small pictures spent a third of its
    // plan() clearing these two arrays on the caller's thread)
    images_.resize((size_t)n);
    desc_.resize((size_t)n);
    fast_idct_ = (a.flags & HIPJPEG_FLAG_FAST_IDCT) != 0;
    entropy_done_ = false;
    entropy_pending_ = false;  // a caller that re-plans without resolve() gives up the statuses of the previous batch
    huff_images_.clear();
    huff_to_image_.clear();
    seq_gpu_images_ = 0;
    prog_images_.clear();
    prog_to_image_.clear();
    prog_walk_images_ = 0;
    interval_takeover_images_ = 0;
    host_fallback_images_ = 0;  // (resolve() counts only for a batch with GPU-decoded streams: any other must not report its page's last one)
    xform_desc_.clear();
    prog_slot_words_ = 0;
    max_huff_units_ = max_huff_pairs_ = max_pool_words_ = 0;
    coef_bytes_ = output_bytes_ = 0;
    if (pool_ && n > 1)
        pool_->parallel_for(n, [&](int i, int) { prepare(i, a); });
    else
        for (int i = 0; i < n; i++) prepare(i, a);
    demote_progressive_lds();
    // progressive images in descriptor order: those of the walk, then those of the interval kernels (a tail prog_walk_kernel is not
    // launched over)
    for (int tail = 0; tail < 2; tail++) {
        for (int i = 0; i < n; i++) {
            PlannedImage& im = images_[i];
            if (im.status != HIPJPEG_STATUS_SUCCESS || !im.gpu_prog || (int)im.gpu_prog_intervals != tail) continue;
            im.prog_index = (int)prog_to_image_.size();
            prog_to_image_.push_back(i);
        }
        if (tail == 0) prog_walk_images_ = prog_to_image_.size();
    }
    Sizing s(n);
    for (int i = 0; i < n; i++) size_image(i, s);
    layout(s);
    const hipjpegStatus_t st = reserve(s);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    bind_pointers(s);
    h2d_used_ = staging_.h2d_bytes;
    if (statuses)
        for (int i = 0; i < n; i++) statuses[i] = images_[i].status;
    return HIPJPEG_STATUS_SUCCESS;
}

// Per-image header work (marker walk through the whole file, eligibility, table sizing); independent of the other images, so it runs
// on all cores.
void DecodeBatch::prepare(int i, const PlanArgs& a)
{
    PlannedImage& im = images_[i];
    im = PlannedImage();
    desc_[i] = DecodeImage();
    im.data = a.infos ? nullptr : a.data[i];
    im.size = a.infos ? 0 : a.lengths[i];
    if (a.formats && ((int)a.formats[i] < 0 || (int)a.formats[i] > (int)HIPJPEG_OUTPUT_YUV_PLANAR)) {
        im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
        return;
    }
    const OutFormat fmt = (OutFormat)(a.formats ? a.formats[i] : a.format);
    bool fancy = (a.flags & HIPJPEG_FLAG_FANCY_UPSAMPLING) != 0;
    const FrameInfo& f = im.frame;
    const int denom = a.scales ? a.scales[i] : 1;
    if (denom != 1 && denom != 2 && denom != 4 && denom != 8) {
        im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
        return;
    }
    im.scale_k = 8 / denom;
    if (a.infos)  // the picture is described, not parsed
        im.status = coefficient_frame(a.infos[i], a.tensors[i], &im.frame);
    else
        im.status = a.data[i] ? status_from_parse(parse_jpeg(a.data[i], a.lengths[i], &im.frame)) : HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (im.status == HIPJPEG_STATUS_SUCCESS && ((uint64_t)f.width * (uint64_t)f.height * (uint64_t)f.ncomp >= max_image_samples() || a.give_up[i]))
        im.status = HIPJPEG_STATUS_ALLOC_FAILED;  // this image only; its neighbours decode
    if (coef_only_) {
        // coefficients only: no kernel variant (-4: no pixel work at all), no output to check; what counts is whether the coder takes it
        TranscodePicture pic;
        im.variant = -4;
        const bool grayscale = a.transcode && (a.transcode[i].orientation & HIPJPEG_TRANSCODE_GRAYSCALE) != 0;
        if (im.status == HIPJPEG_STATUS_SUCCESS && !a.any_frame) im.status = transcode_picture(f, grayscale, &pic);
    } else {
        im.pic_w = f.width;
        im.pic_h = f.height;
        if (im.status == HIPJPEG_STATUS_SUCCESS && im.scale_k != 8) {
            // kernels of their own (decode_kernels.hip, plane_color_kernels.hip: scaled decode); libjpeg does no fancy upsampling at 1/8 (jdsample.c)
            im.variant = -5;
            im.pic_w = scaled_extent(f.width, im.scale_k);
            im.pic_h = scaled_extent(f.height, im.scale_k);
            fancy = fancy && im.scale_k > 1;
            if (!choose_scaled(f, fmt, im.scale_k, im.scaled_size)) im.status = HIPJPEG_STATUS_UNSUPPORTED;
        } else if (im.status == HIPJPEG_STATUS_SUCCESS && !choose_variant(f, fmt, fancy, &im.variant))
            im.status = HIPJPEG_STATUS_UNSUPPORTED;
        for (int p = 0; im.status == HIPJPEG_STATUS_SUCCESS && p < (fmt == kOutPlanarYUV ? f.ncomp : out_planes(fmt)); p++)
            if (!a.outputs[i].plane[p]) im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
        if (im.status == HIPJPEG_STATUS_SUCCESS && a.transforms) im.status = normalise_transform(im, a.transforms[i], fmt);
        if (im.status == HIPJPEG_STATUS_SUCCESS && !pitch_ok(i, a.outputs[i], fmt)) im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
    }
    const bool want_gpu_entropy = (a.flags & HIPJPEG_FLAG_GPU_HUFFMAN) != 0;
    const bool big_enough = (uint64_t)f.width * (uint64_t)f.height > gpu_entropy_min_pixels_ || gpu_entropy_min_pixels_ == 0;
    if (im.status == HIPJPEG_STATUS_SUCCESS && want_gpu_entropy && big_enough && gpu_entropy_eligible(f)) {
        im.gpu_entropy = true;
        for (const ScanHeader& sc : f.scans) im.pool_words = std::max(im.pool_words, gpu_pool_words(sc));
        im.fused_layout = f.scans.size() == 1;
        for (int c = 0; c < f.scans[0].ncomp; c++) im.fused_layout = im.fused_layout && f.scans[0].comp_index[c] == c;
        // Zero-copy input: page-locked caller memory (hipHostMalloc / hipHostRegister, a pinned torch tensor) can
        // be read by the copy engine directly, so the scan's bytes skip the staging copy -- per rank one pass over host DRAM instead
        // of three (read, non-temporal store into the staging area, the engine's read).  HIPJPEG_NO_ZERO_COPY=1 switches it off.
        static const bool zero_copy = getenv("HIPJPEG_NO_ZERO_COPY") == nullptr;
        if (zero_copy) {
            hipPointerAttribute_t attr;
            if (hipPointerGetAttributes(&attr, im.data) == hipSuccess) {
                im.input_pinned = attr.type == hipMemoryTypeHost && attr.devicePointer != nullptr;
                im.input_device_view = static_cast<const uint8_t*>(attr.devicePointer);  // the same bytes as the device addresses them
            } else
                (void)hipGetLastError();  // ordinary pageable memory: the query fails and leaves an error behind
        }
    } else if (im.status == HIPJPEG_STATUS_SUCCESS && want_gpu_entropy && big_enough && gpu_progressive_eligible(f)) {
        im.gpu_entropy = im.gpu_prog = true;
        im.pool_words = prog_pool_words(f);
    } else if (im.status == HIPJPEG_STATUS_SUCCESS && want_gpu_entropy && big_enough && (a.flags & HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS) != 0 &&
               gpu_progressive_interval_eligible(f)) {
        // every scan has a restart interval: staged like any progressive image, a lane per interval in place of the walk
        im.gpu_entropy = im.gpu_prog = im.gpu_prog_intervals = true;
        im.pool_words = prog_pool_words(f);
    }
    if (im.status != HIPJPEG_STATUS_SUCCESS) return;
    // the part of the device descriptor that does not depend on where things will lie in the arenas
    DecodeImage& d = desc_[i];
    const bool scaled = im.variant == -5;
    d.width = (uint32_t)(scaled ? im.pic_w : f.width);
    d.height = (uint32_t)(scaled ? im.pic_h : f.height);
    d.scale_k = scaled ? (uint32_t)im.scale_k : 0u;
    d.ncomp = (uint32_t)f.ncomp;
    d.hmax = (uint32_t)f.hmax;
    d.vmax = (uint32_t)f.vmax;
    d.color_model = (uint32_t)f.color;
    d.out_format = (uint32_t)fmt;
    d.flags = (fancy ? kFlagFancyUpsampling : 0) | (f.saw_adobe ? kFlagAdobeMarker : 0);
    for (int p = 0; p < 3 && a.outputs; p++) {
        d.out[p] = static_cast<uint8_t*>(a.outputs[i].plane[p]);
        d.out_pitch[p] = a.outputs[i].pitch[p];
    }
    for (int c = 0; c < f.ncomp; c++) {
        const Component& k = f.comp[c];
        DecodeComponent& dc = d.comp[c];
        dc.blocks_w = (uint16_t)k.blocks_w;
        dc.blocks_h = (uint16_t)k.blocks_h;
        dc.samp_w = (uint16_t)k.samp_w;
        dc.samp_h = (uint16_t)k.samp_h;
        dc.h = (uint16_t)k.h;
        dc.v = (uint16_t)k.v;
        if (scaled) {
            // the component at the scale (jdmaster.c downsampled_width / height); the reduced IDCTs take ISLOW tables whatever dct_method says
            const int s = im.scaled_size[c];
            dc.scaled = (uint32_t)s;
            dc.samp_w = (uint16_t)(((int64_t)f.width * k.h * s + (int64_t)f.hmax * 8 - 1) / ((int64_t)f.hmax * 8));
            dc.samp_h = (uint16_t)(((int64_t)f.height * k.v * s + (int64_t)f.vmax * 8 - 1) / ((int64_t)f.vmax * 8));
        }
        pack_qpk(f.qtab[c], fast_idct_ && (!scaled || im.scaled_size[c] == 8), dc.qpk);
    }
}

// Rows of the caller's buffer must hold a row of what is written there (nvJPEG checks the pitch for the reference; here a short
// pitch would make the kernels write overlapping rows or leave the buffer).
bool DecodeBatch::pitch_ok(int i, const hipjpegOutput_t& out, OutFormat fmt) const
{
    const FrameInfo& f = images_[i].frame;
    if (fmt == kOutPlanarYUV) {
        for (int c = 0; c < f.ncomp; c++)
            if (out.pitch[c] < (uint32_t)f.comp[c].samp_w) return false;
        return true;
    }
    int ow = 0, oh = 0;
    output_size(i, &ow, &oh);
    for (int p = 0; p < out_planes(fmt); p++)
        if ((uint64_t)out.pitch[p] < (uint64_t)ow * (uint64_t)out_bpp(fmt)) return false;
    return true;
}

// The progressive walk / replay launches are sized for the batch's maxima (largest table x most scans, enqueue_progressive): keep
// their dynamic LDS inside the device's workgroup limit by handing the most demanding images to the host entropy stage -- a refused
// launch would fail the whole batch.  No golden and no libjpeg-written file comes near the limit.
void DecodeBatch::demote_progressive_lds()
{
    static const size_t lds_limit = [] {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, 0) != hipSuccess || v <= 0) v = 64 * 1024;
        if (const char* e = getenv("HIPJPEG_PROG_LDS_LIMIT")) v = atoi(e);  // test aid
        return (size_t)v;
    }();
    for (;;) {
        // `all`: every progressive image (the table slots of all launches are sized for the batch's largest table); `walk`: the images
        // of the walk alone -- the interval kernels stand in for it and take table slots only, like the replay
        ProgLdsShape all, walk;
        int worst = -1;
        size_t worst_need = 0;
        for (int i = 0; i < (int)images_.size(); i++) {
            if (!images_[i].gpu_prog) continue;
            const ProgLdsShape sh = prog_lds_shape(images_[i].frame);
            all.merge(sh);
            if (!images_[i].gpu_prog_intervals) walk.merge(sh);
            const size_t need = std::max(images_[i].gpu_prog_intervals ? prog_interval_lds_bytes(sh) : prog_walk_lds_bytes(sh), prog_replay_lds_bytes(sh));
            if (need > worst_need) {
                worst_need = need;
                worst = i;
            }
        }
        walk.slot_words = all.slot_words;
        if (worst < 0 || std::max({prog_walk_lds_bytes(walk), prog_interval_lds_bytes(all), prog_replay_lds_bytes(all)}) <= lds_limit) return;
        images_[worst].gpu_entropy = images_[worst].gpu_prog = images_[worst].gpu_prog_intervals = false;
        images_[worst].pool_words = 0;
    }
}

// Image i's share of the pixel kernels' units, the intermediate planes and the geometry pass; then of the entropy stage.
void DecodeBatch::size_image(int i, Sizing& s)
{
    PlannedImage& im = images_[i];
    if (im.status != HIPJPEG_STATUS_SUCCESS) return;
    const FrameInfo& f = im.frame;
    DecodeImage& d = desc_[i];  // (prepare() filled in what does not depend on the layout)
    const OutFormat fmt = (OutFormat)d.out_format;
    if (im.has_transform) {
        // the pixel kernels write a full-frame intermediate picture (same format, 16-byte aligned rows); the geometry
        // pass copies the region, turned upright, into the caller's buffer
        TransformImage t;
        memset(&t, 0, sizeof t);
        t.nplanes = out_planes(fmt);
        t.bpp = out_bpp(fmt);
        const uint32_t ipitch = (uint32_t)align_up((size_t)im.pic_w * t.bpp, 16);
        for (int p = 0; p < t.nplanes; p++) {
            t.dst[p] = d.out[p];
            t.dst_pitch[p] = d.out_pitch[p];
            t.src_pitch[p] = ipitch;
            d.out_pitch[p] = ipitch;
            s.xform_plane_off.push_back(s.planes.take(align_up((size_t)ipitch * im.pic_h + 16, 256)));
        }
        t.x0 = im.transform.x0;
        t.y0 = im.transform.y0;
        t.rw = im.transform.x1 - im.transform.x0;
        t.rh = im.transform.y1 - im.transform.y0;
        const bool swap = im.transform.orientation >= 5;
        t.out_w = swap ? t.rh : t.rw;
        t.out_h = swap ? t.rw : t.rh;
        t.orientation = im.transform.orientation;
        im.xform_index = (int)xform_desc_.size();
        xform_desc_.push_back(t);
        s.xform_units += (size_t)(t.out_h + kTransformRowsPerUnit - 1) / kTransformRowsPerUnit;
    }
    for (int c = 0; c < f.ncomp && im.variant == -5; c++) {
        // a scaled image: every component through a plane of blocks_w s x blocks_h s samples (K1 for s = 8, the reduced kernel else)
        const Component& k = f.comp[c];
        DecodeComponent& dc = d.comp[c];
        const size_t sz = (size_t)im.scaled_size[c];
        dc.plane_pitch = (uint32_t)align_up((size_t)k.blocks_w * sz + 16, 16);
        s.plane_off[(size_t)i * 4 + c] = s.planes.take(align_up((size_t)dc.plane_pitch * k.blocks_h * sz + 16, 256));
        s.units += ((size_t)k.blocks_w * k.blocks_h + kBlocksPerUnit - 1) / kBlocksPerUnit;
    }
    if (im.variant == -5) s.units += ((size_t)im.pic_h + kScaledRowsPerUnit - 1) / kScaledRowsPerUnit;
    for (int c = 0; c < f.ncomp && im.variant != -5; c++) {
        const Component& k = f.comp[c];
        const Route route = component_route(im.variant, fmt, c);
        if (route == kRoutePlane) {
            DecodeComponent& dc = d.comp[c];
            dc.plane_pitch = (uint32_t)align_up((size_t)k.blocks_w * 8 + 16, 16);
            s.plane_off[(size_t)i * 4 + c] = s.planes.take(align_up((size_t)dc.plane_pitch * k.blocks_h * 8 + 16, 256));
        }
        if (route != kRouteNone) s.units += ((size_t)k.blocks_w * k.blocks_h + kBlocksPerUnit - 1) / kBlocksPerUnit;
        if (c == 0 && im.variant >= 0) s.units += (size_t)((k.blocks_w + kLumaTileW - 1) / kLumaTileW) * (size_t)((k.blocks_h + kLumaTileH - 1) / kLumaTileH);
    }
    if (im.variant == -1 || im.variant == -3) s.units += (size_t)f.height;
    coef_bytes_ += f.total_blocks() * 128;
    if (tensor_source_)
        for (int c = 0; c < f.ncomp; c++) s.tensor_units += ((size_t)f.comp[c].blocks_w * f.comp[c].blocks_h + kRelayoutBlocksPerUnit - 1) / kRelayoutBlocksPerUnit;
    if (fmt == kOutPlanarYUV)
        for (int c = 0; c < f.ncomp; c++) output_bytes_ += (uint64_t)f.comp[c].samp_w * f.comp[c].samp_h;
    else
        output_bytes_ += (uint64_t)im.pic_w * im.pic_h * (fmt == kOutY ? 1 : 3);
    if (!im.gpu_entropy) return;
    // the GPU entropy stage's share; offsets into the staging area are relative to their region here, layout() rebases them
    if (im.gpu_prog) im.tables_offset = s.pools.take(align_up(im.pool_words * 2, 64), 1);
    if (!im.gpu_prog)
        for (size_t sidx = 0; sidx < f.scans.size(); sidx++) {
            const ScanHeader& sc = f.scans[sidx];
            const size_t blocks = (size_t)scan_mcus_x(f, sc) * scan_mcus_y(f, sc) * scan_blocks_per_mcu(f, sc);
            im.seq[sidx].dc_diff_offset = s.blocks.take(((blocks + 31) & ~(size_t)31) * 2, 1);
        }
    for (int c = 0; c < f.ncomp; c++) {  // compact DC planes, in the same scratch (behind the differences of a baseline image)
        const size_t nblk = (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
        im.dc_plane_offset[c] = s.blocks.take(((nblk + 31) & ~(size_t)31) * 2, 1);
        if (im.gpu_prog) s.prog_units += (nblk + 255) / 256;
    }
    if (im.gpu_prog) {
        // progressive: every scan is staged and destuffed like a baseline scan; the walk and replay kernels take it from there
        im.prog_huff_first = (uint32_t)s.prog_scans;  // (prog_index: plan_once)
        s.prog_scans += f.scans.size();
        for (size_t sidx = 0; sidx < f.scans.size(); sidx++) {
            const ScanHeader& sc = f.scans[sidx];
            s.scan(sc, &im.prog_raw_offset[sidx], &im.prog_stream_offset[sidx], &im.prog_first_chunk[sidx]);
            if (sc.ss != 0) {
                const int cc = sc.comp_index[0];
                const size_t nb = (size_t)((f.comp[cc].samp_w + 7) / 8) * (size_t)((f.comp[cc].samp_h + 7) / 8);
                im.prog_pos_offset[sidx] = s.prog_pos.take(((nb + 63) & ~(size_t)63) * 4, 1);
                prog_slot_words_ = std::max<unsigned>(prog_slot_words_, (unsigned)prog_table_words(sc.ac[sc.ta[0]]));
            } else if (sc.ah == 0) {
                for (int k = 0; k < sc.ncomp; k++)
                    prog_slot_words_ = std::max<unsigned>(prog_slot_words_, (unsigned)prog_table_words(sc.dc[sc.td[k]]));
            }
        }
        if (im.gpu_prog_intervals) {
            // interval kernels: every scan's interval starts, a workgroup per kProgIntervalLanes intervals of a component's AC chain and
            // of every DC scan, a bitmap per block of the components that have more than one AC scan
            int ac_scans[4] = {0, 0, 0, 0};
            for (size_t sidx = 0; sidx < f.scans.size(); sidx++) {
                const ScanHeader& sc = f.scans[sidx];
                const size_t count = sc.rst_after.size() + 1;
                im.prog_start_offset[sidx] = s.boundaries.take(align_up(sc.rst_after.size() * 4, 64), 1);
                if (sc.ss == 0 || ac_scans[sc.comp_index[0]]++ == 0) s.prog_iv_units += (count + kProgIntervalLanes - 1) / kProgIntervalLanes;
            }
            for (int c = 0; c < f.ncomp; c++)
                if (ac_scans[c] > 1)
                    im.prog_hist_offset[c] = s.prog_pos.take((size_t)((f.comp[c].samp_w + 7) / 8) * (size_t)((f.comp[c].samp_h + 7) / 8) * 8, 8);
        }
        return;
    }
    // sequential: every scan is a stream of its own (one HuffImage each)
    static_assert(sizeof(im.seq) / sizeof(im.seq[0]) == (size_t)kMaxSeqScans, "one SeqScan per scan gpu_entropy_eligible() admits");
    im.huff_index = (int)huff_to_image_.size();
    im.huff_count = (int)f.scans.size();
    seq_gpu_images_++;
    for (size_t sidx = 0; sidx < f.scans.size(); sidx++) {
        const ScanHeader& sc = f.scans[sidx];
        PlannedImage::SeqScan& q = im.seq[sidx];
        huff_to_image_.push_back(i);
        const size_t nsub = (s.scan(sc, &q.raw_offset, &q.stream_offset, &q.first_chunk) * 8 + kSubseqBits - 1) / kSubseqBits;
        const size_t mcus = (size_t)scan_mcus_x(f, sc) * scan_mcus_y(f, sc);
        s.subseq += nsub;
        const size_t sync_units = std::max<size_t>((nsub + kHuffOwn - 1) / kHuffOwn, 1);  // (an empty stream keeps the unit at 0: it reports the image)
        max_huff_units_ += sync_units;
        max_huff_pairs_ += (sync_units + 1) / 2;
        q.pool_words = gpu_pool_words(sc);
        q.tables_offset = s.pools.take(align_up(q.pool_words * 2, 64), 1);
        max_pool_words_ = std::max(max_pool_words_, q.pool_words);
        s.huff_wunits += (mcus + kHuffMcusPerWg - 1) / kHuffMcusPerWg + 1;
        q.num_boundaries = (uint32_t)sc.rst_after.size();  // restart boundaries + per-subsequence index
        q.boundary_offset = s.boundaries.take(sc.restart_interval ? align_up(((size_t)q.num_boundaries + nsub + 1) * 4, 64) : 0, 1);
        q.block_pos_offset = s.block_pos.take(((mcus * scan_blocks_per_mcu(f, sc) + 63) & ~(size_t)63) * 4, 1);
    }
}

// Offsets of every region of the staging area and of the entropy scratch, and the coefficient placement.
void DecodeBatch::layout(const Sizing& s)
{
    const size_t ng = huff_to_image_.size(), chunks = s.chunks.end;
    StagingLayout& L = staging_;
    Carve c;
    L.desc = c.take(sizeof(DecodeImage) * images_.size());
    L.units = c.take(sizeof(WorkUnit) * s.units);
    L.huff_desc = c.take(sizeof(HuffImage) * (ng + s.prog_scans));
    L.huff_units = c.take(sizeof(HuffUnit) * max_huff_units_);
    L.huff_pairs = c.take(sizeof(uint32_t) * max_huff_pairs_);
    L.huff_wunits = c.take(sizeof(HuffUnit) * s.huff_wunits);
    L.huff_dc_units = c.take(sizeof(HuffUnit) * ng * 4);
    L.huff_chunk_units = c.take(sizeof(HuffUnit) * chunks);
    L.huff_drops = c.take(sizeof(uint32_t) * chunks);
    L.xform_desc = c.take(sizeof(TransformImage) * xform_desc_.size());
    L.xform_units = c.take(sizeof(WorkUnit) * s.xform_units);
    L.prog_desc = c.take(sizeof(ProgImage) * prog_to_image_.size());
    L.prog_units = c.take(sizeof(HuffUnit) * s.prog_units);
    L.prog_iv_desc = c.take(sizeof(ProgIntervalImage) * (prog_to_image_.size() - prog_walk_images_));
    L.prog_iv_units = c.take(sizeof(HuffUnit) * s.prog_iv_units);
    L.tensor_planes = c.take(tensor_source_ ? sizeof(CoefPlane) * 4 * images_.size() : 0);
    L.tensor_units = c.take(sizeof(RelayoutUnit) * s.tensor_units);
    L.tables = c.take(s.pools.end);
    L.boundaries = c.take(s.boundaries.end);
    L.streams = c.take(s.raw.end);
    L.coef = c.take(0);
    // HIPJPEG_DENSE_STAGING=1: dense int16 blocks for every host-decoded picture as in rounds 1-2 (A/B and cross-check aid)
    static const bool sparse_enabled = getenv("HIPJPEG_DENSE_STAGING") == nullptr;
    sparse_mode_ = sparse_enabled && !coef_only_ && !tensor_source_;  // (the relayout kernels read and write dense blocks)
    host_coef_used_.store(0);
    for (int pass = 0; pass < 2; pass++) {  // host-decoded images first, GPU-decoded ones (and tensors: import_tensors()) behind the H2D boundary
        if (pass == 1) {
            L.h2d_bytes = c.end;
            L.gpu_coef_begin = c.take(0);
        }
        for (PlannedImage& im : images_) {
            if (im.status != HIPJPEG_STATUS_SUCCESS || (int)(im.gpu_entropy || tensor_source_) != pass) continue;
            if (pass == 0 && sparse_mode_) c.end += 256;  // (host-decoded pictures are placed while they are decoded: room for alignment)
            for (int k = 0; k < im.frame.ncomp; k++) im.coef_offset[k] = c.take((size_t)im.frame.comp[k].blocks_w * im.frame.comp[k].blocks_h * 128, 1);
            if (!im.gpu_entropy) continue;
            if (im.gpu_prog) {
                im.tables_offset += L.tables;
                for (size_t sidx = 0; sidx < im.frame.scans.size(); sidx++) im.prog_raw_offset[sidx] += L.streams;
                for (size_t sidx = 0; sidx < im.frame.scans.size() && im.gpu_prog_intervals; sidx++) im.prog_start_offset[sidx] += L.boundaries;
            } else {
                for (int sidx = 0; sidx < im.huff_count; sidx++) {
                    im.seq[sidx].raw_offset += L.streams;
                    im.seq[sidx].boundary_offset += L.boundaries;
                    im.seq[sidx].tables_offset += L.tables;
                }
            }
        }
    }
    L.total = c.end;
    // device-only scratch of the entropy kernels: subsequence states | first block indices | change counters | ...
    total_subseq_ = s.subseq;
    Carve w;
    w.take(total_subseq_ * 8);  // subsequence states, at 0
    scratch_.first_block = w.take(total_subseq_ * 4);
    scratch_.changed = w.take(256);
    scratch_.incoming = w.take(max_huff_units_ * 8);
    scratch_.tail = w.take(max_huff_units_ * (kTailTaskBytes + 4));  // tail tasks (256 B per unit) + counts
    scratch_.dc_diff = w.take(s.blocks.end);
    scratch_.block_pos = w.take(s.block_pos.end);
    scratch_.records = w.take(total_subseq_ * kRecShorts * 2);  // block-start records: 64 bytes per subsequence
    scratch_.walkers = w.take(max_huff_units_ * 4);            // per sync unit: walks left to the position pass
    scratch_.verdicts = w.take(verdict_bytes());               // what resolve() reads, where the kernels cannot store to the pinned side
    scratch_.drops = w.take(chunks * 4);
    scratch_.prog_pos = w.take(s.prog_pos.end);
    scratch_.group_sums = w.take(s.huff_wunits * 16);  // per block-pass workgroup: DC difference sums of its MCUs
    scratch_.streams = w.take(s.streams.end);
    scratch_.total = w.end;
}

hipjpegStatus_t DecodeBatch::reserve(const Sizing& s)
{
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    // the previous use of these buffers (H2D copy + kernels) must have drained before they are rewritten
    if (in_flight_) {
        if (hipEventSynchronize((hipEvent_t)done_event_) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        in_flight_ = false;
    }
    hipjpegStatus_t st;
    if ((st = pinned_.reserve(staging_.h2d_bytes + 256 + verdict_bytes())) != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = device_.reserve(staging_.total + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = planes_.reserve(s.planes.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    if (!huff_to_image_.empty() || s.prog_scans) return work_.reserve(scratch_.total + 256);
    return HIPJPEG_STATUS_SUCCESS;
}

// Device addresses in the descriptors, now that the arenas have their final size.
void DecodeBatch::bind_pointers(const Sizing& s)
{
    huff_images_.assign(huff_to_image_.size() + s.prog_scans, HuffImage());
    prog_images_.assign(prog_to_image_.size(), ProgImage());
    prog_iv_images_.assign(prog_to_image_.size() - prog_walk_images_, ProgIntervalImage());
    size_t k = 0;  // next TransformImage plane
    for (size_t i = 0; i < images_.size(); i++) {
        const PlannedImage& im = images_[i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        DecodeImage& d = desc_[i];
        for (int c = 0; c < im.frame.ncomp; c++) {
            DecodeComponent& dc = d.comp[c];
            dc.coef = at<const int16_t>(device_, im.coef_offset[c]);
            dc.dc = im.gpu_entropy ? at<const int16_t>(work_, scratch_.dc_diff + im.dc_plane_offset[c]) : dc.coef;
            dc.dc_stride = im.gpu_entropy ? 1 : 64;
            if (s.plane_off[i * 4 + c] != (size_t)-1) dc.plane = planes_.data() + s.plane_off[i * 4 + c];
        }
        if (!im.has_transform) continue;
        TransformImage& t = xform_desc_[im.xform_index];
        for (int p = 0; p < t.nplanes; p++, k++) t.src[p] = d.out[p] = planes_.data() + s.xform_plane_off[k];
    }
}

// The parser counted, per kDestuffChunk-byte chunk of the scan, the bytes that byte-stuffing removal drops; they ride to the device with
// the bitstream (the compact kernel reads them where round 1's count kernel left its results).
void DecodeBatch::stage_chunk_drops(const ScanHeader& sc, uint32_t first_chunk)
{
    static_assert(kScanChunkBytes == (size_t)kDestuffChunk, "the parser counts in the destuff kernels' chunks");
    uint32_t* dst = at<uint32_t>(pinned_, staging_.huff_drops) + first_chunk;
    const size_t chunks = (sc.data_end - sc.data_begin + kScanChunkBytes - 1) / kScanChunkBytes;
    if (sc.chunk_drops.size() != chunks) {  // a frame that was parsed without the walk's counts: the device counts for this batch
        host_drops_missing_.store(true, std::memory_order_relaxed);
        return;
    }
    memcpy(dst, sc.chunk_drops.data(), chunks * sizeof(uint32_t));
}

void DecodeBatch::entropy_stage(int i)
{
    PlannedImage& im = images_[i];
    if (im.status != HIPJPEG_STATUS_SUCCESS || tensor_source_) return;  // (tensors: nothing to decode)
    ScopedRange range(im.gpu_entropy ? "hipjpeg host stage (stage bitstream, is_gpu_huffman=1)" : "hipjpeg host stage (Huffman decode, is_gpu_huffman=0)");
    fault_point("entropy_stage");
    if (im.gpu_prog) {
        // progressive: stage every scan's bytes as they are, expand the scans' Huffman tables, describe scans and chains
        const FrameInfo& f = im.frame;
        for (size_t sidx = 0; sidx < f.scans.size(); sidx++) {
            const ScanHeader& sc = f.scans[sidx];
            const size_t len = sc.data_end - sc.data_begin;
            uint8_t* raw = pinned_.data() + im.prog_raw_offset[sidx];
            copy_to_staging(raw, im.data + sc.data_begin, len);
            memset(raw + len, 0x01, align_up(len, 16) + 16 - len);  // neither FF nor 00
            HuffImage& h = huff_images_[huff_to_image_.size() + im.prog_huff_first + sidx];
            memset(&h, 0, sizeof h);
            h.raw_bytes = (uint32_t)len;
            h.first_chunk = im.prog_first_chunk[sidx];
            im.stream_bytes += (uint32_t)len;
            stage_chunk_drops(sc, h.first_chunk);
            if (im.gpu_prog_intervals) {
                // the destuff kernels drop the restart markers too (their rule: a restart interval other than 0); where the intervals
                // start in what is left, in bits
                h.restart_interval = (uint32_t)sc.restart_interval;
                uint32_t* starts = at<uint32_t>(pinned_, im.prog_start_offset[sidx]);
                for (size_t b = 0; b < sc.rst_after.size(); b++) starts[b] = sc.rst_after[b] * 8u;
            }
        }
        if (im.gpu_prog_intervals) fill_prog_interval_image(f, &prog_iv_images_[(size_t)im.prog_index - prog_walk_images_]);
        fill_prog_image(f, &prog_images_[im.prog_index], at<uint16_t>(pinned_, im.tables_offset));
        for (int c = 0; c < f.ncomp; c++) im.coef_or[c] = 32767u;  // successive approximation: any int16 may come out
        return;
    }
    if (im.gpu_entropy) {
        // host part of the GPU entropy path, scan by scan: stage the scan's bytes as they are (the device removes the byte stuffing),
        // expand its Huffman tables, describe it
        const FrameInfo& f = im.frame;
        im.stream_bytes = 0;
        for (int sidx = 0; sidx < im.huff_count; sidx++) {
            const ScanHeader& sc = f.scans[sidx];
            PlannedImage::SeqScan& q = im.seq[sidx];
            q.stream_bytes = (uint32_t)(sc.data_end - sc.data_begin);
            im.stream_bytes += q.stream_bytes;
            uint8_t* raw = pinned_.data() + q.raw_offset;
            if (!im.input_pinned) {  // (else: transfer() sends the bytes from where they are)
                copy_to_staging(raw, im.data + sc.data_begin, q.stream_bytes);
                memset(raw + q.stream_bytes, 0x01, align_up((size_t)q.stream_bytes, 16) + 16 - q.stream_bytes);  // neither FF nor 00
            }
            stage_chunk_drops(sc, q.first_chunk);
            HuffImage& h = huff_images_[(size_t)im.huff_index + sidx];
            fill_huff_image(f, sc, q.stream_bytes, &h);
            build_gpu_pool(sc, &h, at<uint16_t>(pinned_, q.tables_offset));
            if (sc.restart_interval) {
                // restart boundaries in bits, and for every subsequence the first boundary at or behind its first bit
                uint32_t* bnd = at<uint32_t>(pinned_, q.boundary_offset);
                uint32_t* sub = bnd + q.num_boundaries;
                for (uint32_t b = 0; b < q.num_boundaries; b++) bnd[b] = sc.rst_after[b] * 8u;
                uint32_t idx = 0;
                for (uint32_t j = 0; j <= h.num_subseq; j++) {
                    while (idx < q.num_boundaries && bnd[idx] < j * (uint32_t)kSubseqBits) idx++;
                    sub[j] = idx;
                }
                h.restart_interval = (uint32_t)sc.restart_interval;
                h.num_boundaries = q.num_boundaries;
            }
            // magnitude bound for the 24-bit multiplier decision without seeing the coefficients: DC values live in int16,
            // AC magnitudes are below 2^(largest size category any AC table of the scan can code)
            for (int i = 0; i < sc.ncomp; i++) {
                int maxcat = 0;
                const HuffSpec& t = sc.ac[sc.ta[i]];
                int nv = 0;
                for (int l = 1; l <= 16; l++) nv += t.bits[l];
                for (int v = 0; v < nv; v++) maxcat = std::max(maxcat, t.vals[v] & 15);
                const int c = sc.comp_index[i];
                im.coef_or[c] = 32767u | ((1u << maxcat) - 1);
                im.ac_bound[c] = (1u << maxcat) - 1;
            }
        }
        return;
    }
    EntropyStatus es = kEntropyOk;
    bool dense = true;  // dense blocks at im.coef_offset
    if (sparse_mode_) {
        // Zero-run-compressed staging: the picture is decoded into this thread's scratch as a sparse stream (a record of the non-zero
        // coefficients per block), then given the next free bytes of the host-decoded region -- what crosses PCIe is the stream, a third
        // of the dense blocks for a q90 photograph.  Frames the format does not cover (progressive, several scans), and the odd picture
        // whose stream would be larger than its dense blocks, are placed the same way as dense blocks.
        static thread_local std::vector<uint8_t> scratch;
        size_t bytes = 0, dense_bytes = 0;
        for (int c = 0; c < im.frame.ncomp; c++) dense_bytes += (size_t)im.frame.comp[c].blocks_w * im.frame.comp[c].blocks_h * 128;
        bool sparse = sparse_staging_applies(im.frame);
        if (sparse) {
            scratch.resize(sparse_stream_capacity(im.frame));
            es = decode_coefficients_sparse(im.data, im.size, im.frame, scratch.data(), &bytes);
            if (es == kEntropyOk && bytes > dense_bytes) sparse = false;
        }
        if (es == kEntropyOk) {
            const size_t need = align_up(sparse ? bytes : dense_bytes, 256);
            size_t where = staging_.coef + host_coef_used_.fetch_add(need);
            im.host_coef_offset = where;
            im.host_coef_bytes = need;
            im.sparse = sparse;
            if (sparse) copy_to_staging(pinned_.data() + where, scratch.data(), bytes);
            for (int c = 0; c < im.frame.ncomp && !sparse; c++) {
                im.coef_offset[c] = where;
                where += (size_t)im.frame.comp[c].blocks_w * im.frame.comp[c].blocks_h * 128;
            }
        }
        dense = es == kEntropyOk && !sparse;
    }
    if (dense) {
        int16_t* coef[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int c = 0; c < im.frame.ncomp; c++) coef[c] = at<int16_t>(pinned_, im.coef_offset[c]);
        es = decode_coefficients(im.data, im.size, im.frame, coef, im.coef_or);
    }
    for (int c = 0; c < 4; c++) im.ac_bound[c] = im.coef_or[c];  // the OR covers the DC values too: an upper bound all the same
    switch (es) {
    case kEntropyOk: break;
    case kEntropyTruncated: im.status = HIPJPEG_STATUS_TRUNCATED; break;
    case kEntropyMissingTable: im.status = HIPJPEG_STATUS_BAD_JPEG; break;
    default: im.status = HIPJPEG_STATUS_CORRUPT; break;
    }
}

void DecodeBatch::finalize(hipjpegStatus_t* statuses)
{
    fault_point("finalize");
    // HIPJPEG_FUSED_DECODE=1: the pixel kernels Huffman-decode the blocks themselves (decode_kernels.hip FUSED builds) instead of reading
    // coefficient blocks the block pass wrote to HBM.  Measured: HBM traffic of the step falls by more than half,
    // its TIME rises (2.72 -> 3.20 ms per 256 x 1080p): both halves are bound by instruction issue, and inside the pixel kernels only 32
    // of a wave's 64 lanes have a block to decode.  Off by default; kept as a switch and covered by the parity tests.
    static const bool fused_enabled = getenv("HIPJPEG_FUSED_DECODE") != nullptr && atoi(getenv("HIPJPEG_FUSED_DECODE")) != 0;
    fused_ = fused_enabled && !fast_idct_ && !coef_only_;  // the FUSED builds compute ISLOW only: a fast-IDCT batch takes the plain ones; they write no blocks
    // all or nothing per batch: with fused_ set the block pass is not launched at all, so every GPU-decoded baseline picture must be one the
    // FUSED builds cover completely -- a region of interest launches only the tiles that touch it, the other blocks would go undecoded and
    // unchecked
    for (const PlannedImage& im : images_)
        if (im.status == HIPJPEG_STATUS_SUCCESS && im.gpu_entropy && !im.gpu_prog && im.has_transform) fused_ = false;
    // likewise a scaled image: its kernels read coefficient blocks from HBM, which only the block pass writes
    for (const PlannedImage& im : images_)
        if (im.status == HIPJPEG_STATUS_SUCCESS && im.variant == -5) fused_ = false;
    // likewise a picture the FUSED builds cannot decode from one HuffImage: several scans, or one scan in another component order
    for (const PlannedImage& im : images_)
        if (im.status == HIPJPEG_STATUS_SUCCESS && im.gpu_entropy && !im.gpu_prog && !im.fused_layout) fused_ = false;
    if (statuses)
        for (size_t i = 0; i < images_.size(); i++) statuses[i] = images_[i].status;
    host_taken_.clear();
    build_pixel_units();
    build_entropy_units();
    build_tensor_units();
    // what transfer() has to copy: in sparse mode the host-decoded region ends where the last picture was placed
    h2d_used_ = sparse_mode_ ? std::min(staging_.h2d_bytes, align_up(staging_.coef + host_coef_used_.load(), 256)) : staging_.h2d_bytes;
    stage_tables();
    finalized_ = true;
}

// Units of the pixel kernels (K1 idct_plane, K2 luma_color, K3 generic / CMYK colour) and of the geometry pass, image by image.
void DecodeBatch::build_pixel_units()
{
    for (UnitList* l : {&plane_units_, &fused_plane_units_, &generic_units_, &cmyk_units_, &xform_units_, &reduced_units_, &scaled_color_units_}) l->units.clear();
    for (auto* lists : {&luma_units_, &fused_luma_units_})
        for (auto& row : *lists)
            for (UnitList& l : row) l.units.clear();
    for (size_t i = 0; i < images_.size(); i++) {
        const PlannedImage& im = images_[i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const FrameInfo& f = im.frame;
        DecodeImage& d = desc_[i];
        if (sparse_mode_ && !im.gpu_entropy) {
            // placed while it was decoded (entropy_stage): point the descriptor at where the picture landed
            size_t blocks_before = 0;
            for (int c = 0; c < f.ncomp; c++) {
                DecodeComponent& dc = d.comp[c];
                if (im.sparse) {
                    dc.coef = at<const int16_t>(device_, im.host_coef_offset);
                    dc.block_off = at<const uint32_t>(device_, im.host_coef_offset) + blocks_before;
                    blocks_before += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
                } else {
                    dc.coef = at<const int16_t>(device_, im.coef_offset[c]);
                    dc.block_off = nullptr;
                }
                dc.dc = dc.coef;
                dc.dc_stride = 64;
            }
        }
        const OutFormat fmt = (OutFormat)d.out_format;
        const bool fused = fused_ && im.gpu_entropy && !im.gpu_prog;
        d.huff_index = fused ? (uint32_t)im.huff_index : 0u;
        for (int c = 0; c < f.ncomp && im.variant == -5; c++) {
            const uint32_t nblk = (uint32_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
            std::vector<WorkUnit>& list = (im.scaled_size[c] == 8 ? plane_units_ : reduced_units_).units;
            for (uint32_t b = 0; b < nblk; b += kBlocksPerUnit) list.push_back(WorkUnit{(uint32_t)i, b, (uint32_t)c, (uint32_t)kToPlane});
        }
        for (int y = 0; y < im.pic_h && im.variant == -5; y += kScaledRowsPerUnit) scaled_color_units_.units.push_back(WorkUnit{(uint32_t)i, (uint32_t)y, 0u, 0u});
        for (int c = 0; c < f.ncomp && im.variant != -5; c++) {
            const Route route = component_route(im.variant, fmt, c);
            if (route == kRouteNone) continue;
            const uint32_t nblk = (uint32_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
            const uint32_t mode = route == kRouteOutput ? (uint32_t)(kToOutput | (c << 8)) : (uint32_t)kToPlane;
            for (uint32_t b = 0; b < nblk; b += kBlocksPerUnit) (fused ? fused_plane_units_ : plane_units_).units.push_back(WorkUnit{(uint32_t)i, b, (uint32_t)c, mode});
        }
        if (im.variant >= 0) {
            // luma tiles: 32 blocks wide x 4 block rows (one block row per wave); rows that are pure MCU padding are skipped
            uint32_t real_rows = (uint32_t)(f.height + 7) / 8, first_row = 0, first_col = 0, end_col = (uint32_t)f.comp[0].blocks_w;
            if (im.has_transform) {  // tiles that do not touch the region of interest are not decoded
                first_row = (uint32_t)im.transform.y0 / 8 / kLumaTileH * kLumaTileH;
                real_rows = std::min(real_rows, (uint32_t)(im.transform.y1 + 7) / 8);
                first_col = (uint32_t)im.transform.x0 / 8 / kLumaTileW * kLumaTileW;
                end_col = std::min(end_col, (uint32_t)(im.transform.x1 + 7) / 8);
            }
            // the everyday configuration has a kernel of its own (decode_kernels.hip, COMMON)
            const bool everyday = im.variant != kVarGray && d.color_model == 1 && (d.flags & kFlagFancyUpsampling) &&
                                  (im.variant == kVar11 || im.variant == kVar12 || d.comp[1].samp_w > 2);
            const int layout = !everyday ? 0 : (fmt == kOutInterleavedRGB || fmt == kOutInterleavedBGR) ? 1 : (fmt == kOutPlanarRGB || fmt == kOutPlanarBGR) ? 2 : 0;
            std::vector<WorkUnit>& tiles = (fused ? fused_luma_units_ : luma_units_)[layout][im.variant].units;
            // a ragged right edge of at most half a tile (1920 pixels = 7.5 tiles) is covered by narrow tiles, 16 x 8 blocks,
            // so that no wave runs half empty
            const uint32_t span = end_col - first_col, ragged = span % kLumaTileW;
            const uint32_t wide_end = (ragged != 0 && ragged <= kLumaTileW / 2) ? end_col - ragged : end_col;
            for (uint32_t by = first_row; by < real_rows; by += kLumaTileH)
                for (uint32_t bx = first_col; bx < wide_end; bx += kLumaTileW) tiles.push_back(WorkUnit{(uint32_t)i, bx, by, 0u});
            if (wide_end < end_col)
                for (uint32_t by = first_row; by < real_rows; by += 2 * kLumaTileH) tiles.push_back(WorkUnit{(uint32_t)i, wide_end, by, 1u});
        } else if (im.variant == -1) {
            for (int y = 0; y < f.height; y++) generic_units_.units.push_back(WorkUnit{(uint32_t)i, (uint32_t)y, 0u, 0u});
        } else if (im.variant == -3) {
            for (int y = 0; y < f.height; y++) cmyk_units_.units.push_back(WorkUnit{(uint32_t)i, (uint32_t)y, 0u, 0u});
        }
        if (im.has_transform) {  // geometry pass
            const TransformImage& t = xform_desc_[im.xform_index];
            for (int oy = 0; oy < t.out_h; oy += kTransformRowsPerUnit) xform_units_.units.push_back(WorkUnit{(uint32_t)im.xform_index, (uint32_t)oy, 0u, 0u});
        }
    }
}

// GPU entropy descriptors (batch-wide subsequence numbering, one workgroup per 256 subsequences of an image) and, for the progressive
// images, the scan descriptors' pointers, chunk units for the destuff kernels and units of the replay kernel.
void DecodeBatch::build_entropy_units()
{
    for (std::vector<HuffUnit>* v : {&huff_units_, &huff_wunits_, &huff_chunk_units_, &huff_dc_units_, &prog_units_}) v->clear();
    huff_pairs_.clear();
    uint32_t first_subseq = 0;
    stream_bytes_total_ = 0;
    huff_zero_.clear();
    for (size_t g = 0; g < huff_to_image_.size(); g++) {
        const PlannedImage& im = images_[huff_to_image_[g]];
        HuffImage& h = huff_images_[g];
        if (im.status != HIPJPEG_STATUS_SUCCESS) {
            h.num_subseq = 0;
            continue;
        }
        const int sidx = (int)g - im.huff_index;
        const ScanHeader& sc = im.frame.scans[sidx];
        const PlannedImage::SeqScan& q = im.seq[sidx];
        h.stream = work_.data() + scratch_.streams + q.stream_offset;
        h.raw = device_.data() + q.raw_offset;
        h.raw_src = im.input_pinned ? im.input_device_view + sc.data_begin : nullptr;
        if (h.restart_interval) {
            h.boundaries = at<const uint32_t>(device_, q.boundary_offset);
            h.sub_boundary = h.boundaries + h.num_boundaries;
        }
        h.raw_bytes = q.stream_bytes;
        h.first_chunk = q.first_chunk;
        for (uint32_t c = 0; c * (uint32_t)kDestuffChunk < q.stream_bytes; c++) huff_chunk_units_.push_back(HuffUnit{(uint32_t)g, c});
        h.pool = at<const uint16_t>(device_, q.tables_offset);
        h.dc_diff = at<int16_t>(work_, scratch_.dc_diff + q.dc_diff_offset);
        h.block_pos = at<uint32_t>(work_, scratch_.block_pos + q.block_pos_offset);
        for (uint32_t m = 0; m < h.mcus_x * h.mcus_y; m += kHuffMcusPerWg) huff_wunits_.push_back(HuffUnit{(uint32_t)g, m});
        for (int i = 0; i < sc.ncomp; i++) {  // slot i: frame component sc.comp_index[i]
            const int c = sc.comp_index[i];
            const Component& fc = im.frame.comp[c];
            h.coef[i] = at<int16_t>(device_, im.coef_offset[c]);
            h.dc_plane[i] = at<int16_t>(work_, scratch_.dc_diff + im.dc_plane_offset[c]);
            // a one-component scan codes the real blocks only: the padding of the grid is zeroed (the bottom rows alone when the
            // real blocks fill whole rows, else the whole component)
            const size_t bw = (size_t)fc.blocks_w, bh = (size_t)fc.blocks_h;
            if (sc.ncomp == 1 && (h.mcus_x < bw || h.mcus_y < bh)) {
                const size_t first = h.mcus_x < bw ? 0 : (size_t)h.mcus_y * bw, n = bw * bh - first;
                huff_zero_.push_back(ZeroFill{reinterpret_cast<uint8_t*>(h.coef[i] + first * 64), n * 128, 1, 0});
                huff_zero_.push_back(ZeroFill{reinterpret_cast<uint8_t*>(h.dc_plane[i] + first), n * 2, 1, 0});
            }
        }
        h.first_subseq = first_subseq;
        first_subseq += h.num_subseq;
        // (the unit at 0 also for an empty stream: its workgroup of the position kernel flags the image)
        const size_t first_unit = huff_units_.size();
        for (uint32_t j = 0; j == 0 || j < h.num_subseq; j += kHuffOwn) huff_units_.push_back(HuffUnit{(uint32_t)g, j});
        // the first sync launch takes the image's units two at a time (an odd count: the last one alone)
        for (size_t i = first_unit; i < huff_units_.size(); i += 2) huff_pairs_.push_back(huff_pair_entry((uint32_t)i, i + 1 < huff_units_.size()));
        if (h.restart_interval)  // the predictor starts over inside the scan: the per-component scan (everything else: per MCU group)
            for (uint32_t i = 0; i < h.ncomp; i++) huff_dc_units_.push_back(HuffUnit{(uint32_t)g, i});
        stream_bytes_total_ += q.stream_bytes;
    }
    merge_zero_fills();
    total_subseq_ = first_subseq;
    for (size_t q = 0; q < prog_images_.size(); q++) {
        const PlannedImage& im = images_[prog_to_image_[q]];
        ProgImage& pi = prog_images_[q];
        if (im.status != HIPJPEG_STATUS_SUCCESS) {
            pi.num_scans = 0;
            pi.ncomp = 0;
            pi.dc_len = 0;
            memset(pi.chain_len, 0, sizeof pi.chain_len);
            continue;
        }
        const FrameInfo& f = im.frame;
        for (size_t sidx = 0; sidx < f.scans.size(); sidx++) {
            const size_t hidx = huff_to_image_.size() + im.prog_huff_first + sidx;
            HuffImage& h = huff_images_[hidx];
            h.stream = work_.data() + scratch_.streams + im.prog_stream_offset[sidx];
            h.raw = device_.data() + im.prog_raw_offset[sidx];
            ProgScan& ps = pi.scan[sidx];
            ps.stream = h.stream;
            ps.huff_image = (uint32_t)hidx;
            ps.block_pos = f.scans[sidx].ss != 0 ? at<uint32_t>(work_, scratch_.prog_pos + im.prog_pos_offset[sidx]) : nullptr;
            for (uint32_t c = 0; c * (uint32_t)kDestuffChunk < h.raw_bytes; c++) huff_chunk_units_.push_back(HuffUnit{(uint32_t)hidx, c});
        }
        pi.pool = at<const uint16_t>(device_, im.tables_offset);
        for (int c = 0; c < f.ncomp; c++) {
            pi.coef[c] = at<int16_t>(device_, im.coef_offset[c]);
            pi.dc_plane[c] = at<int16_t>(work_, scratch_.dc_diff + im.dc_plane_offset[c]);
            const uint32_t nblk = (uint32_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
            for (uint32_t b = 0; b < nblk; b += 256) prog_units_.push_back(HuffUnit{(uint32_t)q, ((uint32_t)c << 28) | b});
        }
        stream_bytes_total_ += im.stream_bytes;
    }
    // the interval kernels' share: where each scan's interval starts lie in the batch-wide array, the bitmaps, the units -- AC units
    // first, then the DC units by DC-scan index (one launch per index: enqueue_progressive)
    prog_iv_units_.clear();
    prog_iv_dc_first_.clear();
    uint32_t dc_scans = 0;
    for (size_t q = prog_walk_images_; q < prog_images_.size(); q++) {
        const PlannedImage& im = images_[prog_to_image_[q]];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const uint32_t rel = (uint32_t)(q - prog_walk_images_);
        ProgIntervalImage& iv = prog_iv_images_[rel];
        for (size_t sidx = 0; sidx < im.frame.scans.size(); sidx++) iv.scan[sidx].first_start = (uint32_t)((im.prog_start_offset[sidx] - staging_.boundaries) / 4);
        for (int c = 0; c < im.frame.ncomp; c++) {
            iv.hist[c] = prog_images_[q].chain_len[c] > 1 ? at<unsigned long long>(work_, scratch_.prog_pos + im.prog_hist_offset[c]) : nullptr;
            for (uint32_t first = 0; prog_images_[q].chain_len[c] > 0 && first < iv.ac_count[c]; first += kProgIntervalLanes)
                prog_iv_units_.push_back(HuffUnit{rel, ((uint32_t)c << 28) | first});
        }
        dc_scans = std::max(dc_scans, prog_images_[q].dc_len);
    }
    for (uint32_t d = 0; d < dc_scans; d++) {
        prog_iv_dc_first_.push_back(prog_iv_units_.size());
        for (size_t q = prog_walk_images_; q < prog_images_.size(); q++) {
            const ProgImage& pi = prog_images_[q];
            if (pi.dc_len <= d) continue;  // (an image that failed on the host has none)
            const uint32_t count = prog_iv_images_[q - prog_walk_images_].scan[pi.dc_chain[d]].count;
            for (uint32_t first = 0; first < count; first += kProgIntervalLanes) prog_iv_units_.push_back(HuffUnit{(uint32_t)(q - prog_walk_images_), first});
        }
    }
    prog_iv_dc_first_.push_back(prog_iv_units_.size());
}

// The padding fills of a batch of pictures alike are evenly spaced, in two interleaved series (coefficients, DC planes): each series
// becomes one 2D fill, so that the whole batch costs a handful of launches instead of two per picture.
void DecodeBatch::merge_zero_fills()
{
    std::vector<ZeroFill> in, out;
    in.swap(huff_zero_);
    for (int series = 0; series < 2; series++) {
        for (size_t a = (size_t)series; a < in.size();) {
            ZeroFill z = in[a];
            size_t b = a + 2;
            if (b < in.size() && in[b].bytes == z.bytes && in[b].ptr > z.ptr && (size_t)(in[b].ptr - z.ptr) >= z.bytes) {
                z.pitch = (size_t)(in[b].ptr - z.ptr);
                while (b < in.size() && in[b].bytes == z.bytes && in[b].ptr == z.ptr + z.count * z.pitch) {
                    z.count++;
                    b += 2;
                }
            }
            out.push_back(z);
            a += 2 * z.count;
        }
    }
    huff_zero_.swap(out);
}

// The luma tiles of a tile row share chroma lines at their seams (fancy upsampling reads a sample to the left and to the right of a
// tile: one more 128-byte line on either side), and the hardware deals workgroups to the eight XCDs -- eight L2 caches -- in turn.  So the
// rows are dealt to eight queues and the list takes one tile of every queue in turn: position p goes to XCD p % 8, a row's tiles follow
// each other on ONE XCD and find their neighbour's lines in its L2.
static void deal_rows_to_xcds(std::vector<WorkUnit>& v)
{
    if (v.size() < 64) return;
    constexpr size_t kXcds = 8;
    std::vector<WorkUnit> queue[kXcds], rest, out;
    out.reserve(v.size());
    auto flush = [&]() {  // one picture's tiles: a tile of every queue in turn, then its narrow edge tiles (the list stays sorted by picture)
        size_t taken[kXcds] = {0};
        for (bool any = true; any;) {
            any = false;
            for (size_t q = 0; q < kXcds; q++)
                if (taken[q] < queue[q].size()) {
                    out.push_back(queue[q][taken[q]++]);
                    any = true;
                }
        }
        out.insert(out.end(), rest.begin(), rest.end());
        for (auto& q : queue) q.clear();
        rest.clear();
    };
    size_t row = 0;
    for (size_t a = 0; a < v.size();) {
        size_t b = a + 1;
        while (b < v.size() && v[b].image == v[a].image && v[b].comp == v[a].comp && v[b].mode == v[a].mode) b++;
        if (a > 0 && v[a].image != v[a - 1].image) {
            flush();
            row = 0;
        }
        if (v[a].mode != 0) {
            rest.insert(rest.end(), v.begin() + (long)a, v.begin() + (long)b);
        } else {
            std::vector<WorkUnit>& q = queue[row++ % kXcds];
            q.insert(q.end(), v.begin() + (long)a, v.begin() + (long)b);
        }
        a = b;
    }
    flush();
    v.swap(out);
}

// Descriptors and unit tables into the staging area.  The pixel kernels' lists lie back to back from staging_.units on.
void DecodeBatch::stage_tables()
{
    auto stage = [&](UnitList& list, Carve& where) {
        list.offset = where.take(list.units.size() * sizeof(WorkUnit), 1);
        copy_table(pinned_, list.offset, list.units);
    };
    copy_table(pinned_, staging_.desc, desc_);
    Carve units{staging_.units};
    stage(plane_units_, units);
    for (auto& lists : luma_units_)
        for (UnitList& l : lists) {
            deal_rows_to_xcds(l.units);
            stage(l, units);
        }
    stage(fused_plane_units_, units);
    for (auto& lists : fused_luma_units_)
        for (UnitList& l : lists) stage(l, units);
    stage(generic_units_, units);
    stage(cmyk_units_, units);
    stage(reduced_units_, units);
    stage(scaled_color_units_, units);
    Carve xform{staging_.xform_units};
    stage(xform_units_, xform);
    copy_table(pinned_, staging_.xform_desc, xform_desc_);
    copy_table(pinned_, staging_.tensor_planes, tensor_table_);
    copy_table(pinned_, staging_.tensor_units, tensor_units_);
    copy_table(pinned_, staging_.prog_desc, prog_images_);
    copy_table(pinned_, staging_.prog_units, prog_units_);
    copy_table(pinned_, staging_.prog_iv_desc, prog_iv_images_);
    copy_table(pinned_, staging_.prog_iv_units, prog_iv_units_);
    copy_table(pinned_, staging_.huff_desc, huff_images_);
    copy_table(pinned_, staging_.huff_units, huff_units_);
    copy_table(pinned_, staging_.huff_pairs, huff_pairs_);
    copy_table(pinned_, staging_.huff_wunits, huff_wunits_);
    copy_table(pinned_, staging_.huff_dc_units, huff_dc_units_);
    copy_table(pinned_, staging_.huff_chunk_units, huff_chunk_units_);
}

hipjpegStatus_t DecodeBatch::transfer(void* stream, bool kernels_on_other_stream)
{
    if (!finalized_) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    ScopedRange range("hipjpeg transfer to device");
    fault_point("transfer");
    entropy_done_ = false;
    pixels_launched_ = false;
    if (h2d_used_ == 0) return HIPJPEG_STATUS_SUCCESS;
    // only descriptors, bitstreams of GPU-decoded images and coefficients of host-decoded images cross PCIe
    zero_copy_images_ = 0;
    for (const PlannedImage& im : images_) zero_copy_images_ += (im.status == HIPJPEG_STATUS_SUCCESS && im.gpu_entropy && !im.gpu_prog && im.input_pinned) ? 1 : 0;
    hipError_t e = hipSuccess;
    if (zero_copy_images_ == 0) {
        e = hipMemcpyAsync(device_.data(), pinned_.data(), h2d_used_, hipMemcpyHostToDevice, (hipStream_t)stream);
    } else {
        // everything but the staged bitstreams in two pieces (in front of and behind their region), the region's padding bytes in one
        // fill (neither FF nor 00, see entropy_stage), then one copy per scan: from the caller's pinned memory, or from the staging area
        // for the images of the batch that are not zero-copy; the zero-copy ones are pulled over by ONE kernel (gather_raw_kernel)
        hipStream_t s = (hipStream_t)stream;
        const size_t rb = std::min(staging_.streams, h2d_used_), re = std::min(staging_.coef, h2d_used_);
        if (rb > 0) e = hipMemcpyAsync(device_.data(), pinned_.data(), rb, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && re > rb) e = hipMemsetAsync(device_.data() + rb, 0x01, re - rb, s);
        if (e == hipSuccess && h2d_used_ > re) e = hipMemcpyAsync(device_.data() + re, pinned_.data() + re, h2d_used_ - re, hipMemcpyHostToDevice, s);
        for (const PlannedImage& im : images_) {
            if (e != hipSuccess) break;
            if (im.status != HIPJPEG_STATUS_SUCCESS || !im.gpu_entropy) continue;
            if (im.gpu_prog) {
                for (size_t sidx = 0; sidx < im.frame.scans.size() && e == hipSuccess; sidx++) {
                    const ScanHeader& sc = im.frame.scans[sidx];
                    const size_t len = sc.data_end - sc.data_begin;
                    if (len) e = hipMemcpyAsync(device_.data() + im.prog_raw_offset[sidx], pinned_.data() + im.prog_raw_offset[sidx], align_up(len, 16) + 16, hipMemcpyHostToDevice, s);
                }
                continue;
            }
            for (int sidx = 0; sidx < im.huff_count && e == hipSuccess && !im.input_pinned; sidx++) {  // (the pinned ones: one kernel for all of them, below)
                const PlannedImage::SeqScan& q = im.seq[sidx];
                e = hipMemcpyAsync(device_.data() + q.raw_offset, pinned_.data() + q.raw_offset, align_up((size_t)q.stream_bytes, 16) + 16, hipMemcpyHostToDevice, s);
            }
        }
        if (e == hipSuccess && launch_gather_raw(at<const HuffImage>(device_, staging_.huff_desc), at<const HuffUnit>(device_, staging_.huff_chunk_units),
                                                 (int)huff_chunk_units_.size(), stream) != 0) e = hipErrorLaunchFailure;
    }
    if (e == hipSuccess && kernels_on_other_stream) {
        if (!ensure_event(&copied_event_)) return HIPJPEG_STATUS_HIP_ERROR;
        e = hipEventRecord((hipEvent_t)copied_event_, (hipStream_t)stream);
        copy_pending_ = true;
    }
    return e == hipSuccess ? HIPJPEG_STATUS_SUCCESS : HIPJPEG_STATUS_HIP_ERROR;
}

// GPU entropy stage: remove the byte stuffing, synchronise the subsequence decoders, scan block counts, write the
// coefficient blocks, integrate DC.  The common case is enqueued without any host round trip: launch 1 leaves every workgroup in
// a local fixpoint (its tail kernel already enters every workgroup with the state in front of it as it is by then, so most
// boundaries are settled too), launch 2 repairs the remaining workgroup boundaries and counts the workgroups whose outgoing state moved; when
// that count is zero the states are the global fixpoint (no workgroup consumed a state that changed afterwards).  Only if
// it is not zero -- a correction crossed a whole workgroup -- more launches follow and the write passes are repeated.
// Blocks at the end: the host needs the per-image status to fall back to its own entropy decoder for streams the kernels
// flagged (corrupt or truncated data).
// Everything of the entropy stage that needs no answer from the device: enqueued, not waited for.
hipjpegStatus_t DecodeBatch::enqueue_gpu_entropy(void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    entropy_done_ = true;
    if (huff_units_.empty() && prog_units_.empty()) return HIPJPEG_STATUS_SUCCESS;
    EntropyLaunch L = entropy_launch_args();
    if (huff_chunk_units_.empty() && hipMemsetAsync(L.changed, 0, 256, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;  // (else: the compact kernel clears them)
    for (const ZeroFill& z : huff_zero_)
        if ((z.count == 1 ? hipMemsetAsync(z.ptr, 0, z.bytes, s) : hipMemset2DAsync(z.ptr, z.pitch, 0, z.bytes, z.count, s)) != hipSuccess)
            return HIPJPEG_STATUS_HIP_ERROR;
    // the per-chunk counts of bytes to drop came up with the bitstreams (the parser's marker walk sees every FF anyway);
    // HIPJPEG_DEVICE_DESTUFF_COUNT=1 counts them on the device as round 1 did (A/B and cross-check aid)
    static const bool force_device_count = getenv("HIPJPEG_DEVICE_DESTUFF_COUNT") != nullptr;
    const bool device_count = force_device_count || host_drops_missing_.load(std::memory_order_relaxed);
    if (launch_destuff(L.dimg, at<const HuffUnit>(device_, staging_.huff_chunk_units), (int)huff_chunk_units_.size(),
                       device_count ? at<uint32_t>(work_, scratch_.drops) : at<uint32_t>(device_, staging_.huff_drops),
                       device_count, L.changed, stream) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (!prog_units_.empty()) {
        const hipjpegStatus_t ps = enqueue_progressive(stream);
        if (ps != HIPJPEG_STATUS_SUCCESS) return ps;
    }
    if (huff_units_.empty()) {
        entropy_pending_ = true;
        return HIPJPEG_STATUS_SUCCESS;
    }
    static const int tail_after = getenv("HIPJPEG_TAIL_AFTER") ? atoi(getenv("HIPJPEG_TAIL_AFTER")) : 2;  // tuning aid; 0 = no tail kernel
    uint16_t* tail_tasks = at<uint16_t>(work_, scratch_.tail);
    uint32_t* tail_count = at<uint32_t>(work_, scratch_.tail + (size_t)max_huff_units_ * kTailTaskBytes);
    if (launch_huff_sync(L.dimg, L.dunits, L.nunits, at<const uint32_t>(device_, staging_.huff_pairs), (int)huff_pairs_.size(), L.states, L.incoming,
                         L.changed, 1, tail_after > 0 ? tail_after : 1 << 20,
                         tail_after > 0 ? tail_tasks : nullptr, tail_after > 0 ? tail_count : nullptr, L.records, L.pool_bytes, stream) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (launch_huff_sync(L.dimg, L.dunits, L.nunits, nullptr, 0, L.states, L.incoming, L.changed, 0, 1 << 20, nullptr, nullptr, L.records, L.pool_bytes, stream, 1) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    // The verdicts resolve() reads are stored by the stage's last kernel, into the pinned side itself: no copy command between the
    // entropy kernels and the pixel kernels.  Pinned memory from a caller's allocator may not be mapped into the device's address
    // space: the kernel stores to the scratch then and one copy follows.  (FUSED builds: the descriptors come back behind the pixel
    // kernels, see launch().)
    if (!entropy_write_passes(L, stream)) return HIPJPEG_STATUS_HIP_ERROR;
    if (L.verdicts_out != L.host_changed && hipMemcpyAsync(L.host_changed, L.verdicts_out, verdict_bytes(), hipMemcpyDeviceToHost, s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (fused_ && hipMemcpyAsync(L.himg, L.dimg, sizeof(HuffImage) * huff_images_.size(), hipMemcpyDeviceToHost, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    entropy_pending_ = true;
    return HIPJPEG_STATUS_SUCCESS;
}

// Progressive images: walk (block start positions of every scan, DC planes), replay (coefficient blocks), verdicts back.
hipjpegStatus_t DecodeBatch::enqueue_progressive(void* stream)
{
    ProgImage* dprog = at<ProgImage>(device_, staging_.prog_desc);
    const HuffImage* dimg = at<const HuffImage>(device_, staging_.huff_desc);
    const unsigned slot = (unsigned)align_up(std::max<unsigned>(prog_slot_words_, 256u), 64);
    unsigned dc_slots = 1, ac_waves = 0, rings = 0;  // per workgroup (= image): DC table slots, AC scans (one wave each), hand-over rings
    for (size_t q = 0; q < prog_walk_images_; q++) {  // the walk's images: the head of the array
        const ProgImage& pi = prog_images_[q];
        unsigned scans = 0, handovers = 0;
        for (int c = 0; c < 4; c++) {
            scans += pi.chain_len[c];
            handovers += pi.chain_len[c] > 0 ? pi.chain_len[c] - 1 : 0;
        }
        ac_waves = std::max(ac_waves, scans);
        rings = std::max(rings, handovers);
        for (uint32_t k = 0; k < pi.num_scans; k++)
            if (pi.scan[k].ss == 0 && pi.scan[k].ah == 0) dc_slots = std::max<unsigned>(dc_slots, pi.scan[k].ncomp);
    }
    static const bool debug_stats = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;
    if (debug_stats)
        fprintf(stderr, "[hipjpeg] progressive walk: %zu images, %u + 1 waves per workgroup, %u table slots of %u entries, %u rings; interval kernels: %zu images\n",
                prog_walk_images_, ac_waves, dc_slots + ac_waves, slot, rings, prog_images_.size() - prog_walk_images_);
    if (launch_prog_walk(dprog, dimg, (int)prog_walk_images_, slot, dc_slots, ac_waves, rings, stream) != 0) return HIPJPEG_STATUS_HIP_ERROR;
    if (!prog_iv_units_.empty()) {
        // the tail of the array: a lane per restart interval -- the AC chains in one launch, the DC scans in one launch per DC-scan index
        ProgImage* tail = dprog + prog_walk_images_;
        const ProgIntervalImage* ivs = at<const ProgIntervalImage>(device_, staging_.prog_iv_desc);
        const uint32_t* starts = at<const uint32_t>(device_, staging_.boundaries);
        const HuffUnit* units = at<const HuffUnit>(device_, staging_.prog_iv_units);
        if (launch_prog_interval_ac(tail, ivs, dimg, starts, units, (int)prog_iv_dc_first_[0], slot, stream) != 0) return HIPJPEG_STATUS_HIP_ERROR;
        for (size_t d = 0; d + 1 < prog_iv_dc_first_.size(); d++)
            if (launch_prog_interval_dc(tail, ivs, dimg, starts, units + prog_iv_dc_first_[d], (int)(prog_iv_dc_first_[d + 1] - prog_iv_dc_first_[d]), (unsigned)d,
                                        slot, stream) != 0)
                return HIPJPEG_STATUS_HIP_ERROR;
    }
    if (launch_prog_replay(dprog, dimg, at<const HuffUnit>(device_, staging_.prog_units), (int)prog_units_.size(), slot, stream) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (hipMemcpyAsync(pinned_.data() + staging_.prog_desc, dprog, sizeof(ProgImage) * prog_images_.size(), hipMemcpyDeviceToHost,
                       (hipStream_t)stream) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

DecodeBatch::EntropyLaunch DecodeBatch::entropy_launch_args()
{
    EntropyLaunch L;
    L.dimg = at<HuffImage>(device_, staging_.huff_desc);
    L.dunits = at<const HuffUnit>(device_, staging_.huff_units);
    L.dwunits = at<const HuffUnit>(device_, staging_.huff_wunits);
    L.ddc = at<const HuffUnit>(device_, staging_.huff_dc_units);
    L.states = at<unsigned long long>(work_, 0);
    L.first_block = at<uint32_t>(work_, scratch_.first_block);
    // HIPJPEG_POSITION_PASS=1: the position pass walks every subsequence, as before the records (A/B aid).  So it does for a batch
    // whose record offsets do not fit 32 bits (the kernels' offsets wrap inside the region: never read, never outside it).
    static const bool full_position_pass = getenv("HIPJPEG_POSITION_PASS") != nullptr && atoi(getenv("HIPJPEG_POSITION_PASS")) != 0;
    L.records = at<uint16_t>(work_, scratch_.records);
    L.use_records = !full_position_pass && total_subseq_ * kRecShorts * 2 < (1ull << 32) ? L.records : nullptr;
    L.walkers = at<uint32_t>(work_, scratch_.walkers);
    L.group_sums = at<int32_t>(work_, scratch_.group_sums);
    L.changed = at<unsigned int>(work_, scratch_.changed);
    L.incoming = at<unsigned long long>(work_, scratch_.incoming);
    L.pool_bytes = (unsigned)align_up(max_pool_words_ * 2, 256);
    L.nunits = (int)huff_units_.size();
    // behind the staged data, on the pinned side: the convergence counters, then a verdict word per HuffImage (huff_verdict())
    L.host_changed = at<unsigned int>(pinned_, staging_.h2d_bytes);
    L.verdicts = L.host_changed + kHuffVerdictCounters;
    L.verdicts_out = pinned_.custom() ? at<unsigned int>(work_, scratch_.verdicts) : L.host_changed;
    L.himg = at<HuffImage>(pinned_, staging_.huff_desc);
    return L;
}

bool DecodeBatch::entropy_write_passes(const EntropyLaunch& L, void* stream)
{
    return launch_huff_write(L.dimg, L.dunits, L.nunits, L.dwunits, (int)huff_wunits_.size(), L.states, L.first_block, L.use_records, L.walkers, L.group_sums, L.pool_bytes,
                             stream, fused_) == 0 &&
           launch_huff_dc(L.dimg, L.ddc, (int)huff_dc_units_.size(), L.dwunits, (int)huff_wunits_.size(), L.group_sums, L.changed, L.verdicts_out, stream) == 0;
}

hipjpegStatus_t DecodeBatch::wait_done()
{
    if (!in_flight_) return HIPJPEG_STATUS_SUCCESS;
    return hipEventSynchronize((hipEvent_t)done_event_) == hipSuccess ? HIPJPEG_STATUS_SUCCESS : HIPJPEG_STATUS_HIP_ERROR;
}

// Waits for the work enqueued on `stream` and settles what the entropy kernels reported: extra synchronisation launches if
// a correction crossed a whole workgroup, host entropy decoding for streams the kernels flagged (corrupt or truncated
// data) -- after either, the pixel kernels run again.  Per-image statuses are final afterwards.
hipjpegStatus_t DecodeBatch::resolve(void* stream)
{
    if (!entropy_pending_) return HIPJPEG_STATUS_SUCCESS;
    ScopedRange range("hipjpeg resolve (GPU entropy verdicts)");
    fault_point("resolve");
    hipStream_t s = (hipStream_t)stream;
    // wait for THIS batch's work only (a later batch may already be queued on the same stream)
    if (in_flight_ ? hipEventSynchronize((hipEvent_t)done_event_) != hipSuccess : hipStreamSynchronize(s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    entropy_pending_ = false;
    const EntropyLaunch L = entropy_launch_args();
    const size_t himg_bytes = sizeof(HuffImage) * huff_images_.size();
    bool redo_pixels = false;
    last_sync_launches_ = 2;
    static const bool debug_stats = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;
    if (debug_stats)  // host_changed[2..3]: correction rounds of the first sync launch (sum over workgroups, maximum)
        fprintf(stderr, "[hipjpeg] entropy: %d workgroups, launch 1 rounds avg %.2f max %u, tail rounds avg %.2f max %u; launch 2: %u rounds in total, max %u, %u boundary changes\n",
                L.nunits, (double)L.host_changed[2] / L.nunits, L.host_changed[3], (double)L.host_changed[6] / L.nunits, L.host_changed[7], L.host_changed[4],
                L.host_changed[5], L.host_changed[0]);
    bool converged = huff_units_.empty() || *L.host_changed == 0;
    // The ripple launch queued with the batch (pass 1) left groups whose last end state still moved: corrections that cross more
    // than one group border.  A few more launches settle a photograph; a periodic stream (stripes, a test pattern) would need one
    // launch per group, each a sequential walk through 255 subsequences -- those images go to the host decoder instead
    // (HuffImage::gave_up / moved_pass say which), 25 times faster for them.
    constexpr int kExtraRippleLaunches = 4;
    uint32_t last_pass = 1;
    std::vector<char> unsettled(huff_images_.size(), 0);
    // the common case reads the verdict words the stage's last kernel left; the descriptors themselves are fetched where the write
    // passes are repeated below (and by the FUSED builds, whose pixel kernels flag images too)
    bool from_desc = fused_;
    if (!converged) {
        from_desc = true;
        for (int pass = 0; pass < kExtraRippleLaunches && !converged; pass++) {
            if (hipMemsetAsync(L.changed, 0, sizeof(unsigned int), s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
            if (launch_huff_sync(L.dimg, L.dunits, L.nunits, nullptr, 0, L.states, L.incoming, L.changed, 0, 1 << 20, nullptr, nullptr, L.records, L.pool_bytes, stream, ++last_pass) != 0)
                return HIPJPEG_STATUS_HIP_ERROR;
            if (hipMemcpyAsync(L.host_changed, L.changed, sizeof(unsigned int), hipMemcpyDeviceToHost, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
            if (hipStreamSynchronize(s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
            last_sync_launches_++;
            converged = *L.host_changed == 0;
        }
        // the write passes queued with the batch ran on unsettled states: fetch the flags, clear the verdicts, repeat them
        if (hipMemcpyAsync(L.himg, L.dimg, himg_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        if (hipStreamSynchronize(s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        for (size_t g = 0; g < huff_to_image_.size(); g++) {
            unsettled[g] = L.himg[g].gave_up != 0 || (!converged && L.himg[g].moved_pass == last_pass);
            L.himg[g].status = 0;
        }
        if (hipMemcpyAsync(L.dimg, L.himg, himg_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        if (!entropy_write_passes(L, stream)) return HIPJPEG_STATUS_HIP_ERROR;
        // FUSED builds: the pixel kernels decode the blocks, so their verdicts belong to this read-back
        if (fused_ && pixels_launched_ && launch_pixel_kernels(stream, -1) != 0) return HIPJPEG_STATUS_HIP_ERROR;
        if (hipMemcpyAsync(L.himg, L.dimg, himg_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        if (hipStreamSynchronize(s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        redo_pixels = true;
    } else {
        // a group ran out of rounds in the tail kernel
        for (size_t g = 0; g < huff_to_image_.size(); g++) unsettled[g] = from_desc ? L.himg[g].gave_up != 0 : huff_verdict_gave_up(L.verdicts[g]);
    }
    // The kernels could not vouch for a stream (corrupt / truncated data, a periodic stream): the host entropy decoder produces
    // either the coefficients or the precise error.
    // A picture in several scans is taken over when any of them is flagged, once.
    std::vector<int> takeover;
    for (size_t g = 0; g < huff_to_image_.size(); g++) {
        const int i = huff_to_image_[g];
        const bool flagged = from_desc ? L.himg[g].status != 0 : huff_verdict_status(L.verdicts[g]) != 0;
        if (images_[i].status == HIPJPEG_STATUS_SUCCESS && (flagged || unsettled[g]) && (takeover.empty() || takeover.back() != i))
            takeover.push_back(i);
    }
    host_fallback_images_ = (int)takeover.size();
    const ProgImage* hprog = at<const ProgImage>(pinned_, staging_.prog_desc);
    if (debug_stats && !prog_to_image_.empty()) print_progressive_timing(hprog);
    interval_takeover_images_ = 0;
    for (size_t q = 0; q < prog_to_image_.size(); q++)
        if (images_[prog_to_image_[q]].status == HIPJPEG_STATUS_SUCCESS && hprog[q].status != 0) {
            takeover.push_back(prog_to_image_[q]);
            interval_takeover_images_ += q >= prog_walk_images_ ? 1 : 0;
        }
    const hipjpegStatus_t st = take_over_on_host(takeover, &redo_pixels);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    if (redo_pixels && pixels_launched_) {
        // the pixel kernels already ran on coefficients that have just been replaced
        if (launch_pixel_kernels(stream, -1) != 0 || hipStreamSynchronize(s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    }
    return HIPJPEG_STATUS_SUCCESS;
}

// HIPJPEG_DEBUG_TIMING: per scan of the progressive images, how long the walk took (read back with the ProgImage array).
void DecodeBatch::print_progressive_timing(const ProgImage* hprog) const
{
    const ProgImage& q0 = hprog[0];
    for (uint32_t k = 0; k < q0.num_scans; k++) {
        // the same scan over all images of the batch that have it (min / mean / max), and where image 0's wave ran
        uint32_t lo = ~0u, hi = 0, cnt = 0;
        double sum = 0;
        for (size_t q = 0; q < prog_to_image_.size(); q++) {
            if (hprog[q].num_scans <= k) continue;
            const uint32_t t = hprog[q].scan[k].walk_ticks;
            lo = std::min(lo, t);
            hi = std::max(hi, t);
            sum += t;
            cnt++;
        }
        const uint32_t hw = q0.scan[k].pad_ticks[0];  // HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13
        fprintf(stderr,
                "[hipjpeg] progressive image 0 scan %u (ss %u se %u ah %u al %u): walk %.3f ms, of which waiting for neighbours %.3f ms; se %u cu %u simd %u; "
                "all %u images: %.3f / %.3f / %.3f ms\n",
                k, q0.scan[k].ss, q0.scan[k].se, q0.scan[k].ah, q0.scan[k].al, q0.scan[k].walk_ticks * 1e-5, q0.scan[k].wait_ticks * 1e-5, (hw >> 13) & 7u,
                (hw >> 8) & 15u, (hw >> 4) & 3u, cnt, lo * 1e-5, cnt ? sum / cnt * 1e-5 : 0.0, hi * 1e-5);
    }
}

// The host entropy decoder takes over the images the kernels could not vouch for.  Decoding runs on the batch's thread pool when there
// is one -- a batch of test patterns hands over every image -- a helping of images at a time; the uploads follow on this thread.
hipjpegStatus_t DecodeBatch::take_over_on_host(const std::vector<int>& takeover, bool* redo_pixels)
{
    constexpr size_t kHelping = 32;
    for (size_t first = 0; first < takeover.size(); first += kHelping) {
        const size_t count = std::min(kHelping, takeover.size() - first);
        std::vector<std::vector<int16_t>> coefs(count);
        std::vector<EntropyStatus> verdict(count, kEntropyOk);
        auto decode_one = [&](int j) {
            const PlannedImage& im = images_[takeover[first + j]];
            const FrameInfo& f = im.frame;
            coefs[j].assign(f.total_blocks() * 64, 0);
            int16_t* coef[4] = {nullptr, nullptr, nullptr, nullptr};
            size_t off = 0;
            for (int c = 0; c < f.ncomp; c++) {
                coef[c] = coefs[j].data() + off;
                off += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64;
            }
            verdict[j] = decode_coefficients(im.data, im.size, f, coef, nullptr);
        };
        if (pool_ && count > 1)
            pool_->parallel_for((int)count, [&](int j, int) { decode_one(j); });
        else
            for (size_t j = 0; j < count; j++) decode_one((int)j);
        for (size_t j = 0; j < count; j++) {
            PlannedImage& im = images_[takeover[first + j]];
            if (verdict[j] != kEntropyOk) {
                im.status = verdict[j] == kEntropyTruncated ? HIPJPEG_STATUS_TRUNCATED : HIPJPEG_STATUS_CORRUPT;
                continue;
            }
            const FrameInfo& f = im.frame;
            size_t off = 0;
            for (int c = 0; c < f.ncomp; c++) {
                const size_t nblk = (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h;
                int16_t* coef = coefs[j].data() + off;
                off += nblk * 64;
                std::vector<int16_t> dc(nblk);  // the kernels take this image's DC values from its compact DC plane
                for (size_t b = 0; b < nblk; b++) {
                    dc[b] = coef[b * 64];
                    coef[b * 64] = 0;
                }
                if (hipMemcpy(device_.data() + im.coef_offset[c], coef, nblk * 128, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(work_.data() + scratch_.dc_diff + im.dc_plane_offset[c], dc.data(), nblk * 2, hipMemcpyHostToDevice) != hipSuccess)
                    return HIPJPEG_STATUS_HIP_ERROR;
            }
            if (fused_ && im.gpu_entropy && !im.gpu_prog) host_taken_.push_back(takeover[first + j]);
            *redo_pixels = true;
        }
    }
    return HIPJPEG_STATUS_SUCCESS;
}

// The plain K1 / K2 builds for the images in host_taken_: their units are those of the FUSED lists (same geometry), picked out by
// image, uploaded to a scratch buffer of their own.  Rare path (damaged or periodic streams): blocking copies are fine.
int DecodeBatch::launch_taken_pixels(void* stream, int which)
{
    const DecodeImage* dimg = at<const DecodeImage>(device_, staging_.desc);
    std::vector<char> taken(images_.size(), 0);
    for (int i : host_taken_) taken[(size_t)i] = 1;
    std::vector<WorkUnit> units;
    struct Run {
        int layout, variant;  // layout < 0: K1
        size_t first, count;
    };
    std::vector<Run> runs;
    auto pick = [&](const UnitList& from, int layout, int variant) {
        const size_t first = units.size();
        for (const WorkUnit& u : from.units)
            if (taken[u.image]) units.push_back(u);
        if (units.size() > first) runs.push_back(Run{layout, variant, first, units.size() - first});
    };
    if (which < 0 || which == 0) pick(fused_plane_units_, -1, 0);
    if (which < 0 || which == 1)
        for (int e = 0; e < kNumLumaLayouts; e++)
            for (int k = 0; k < kNumLumaVariants; k++) pick(fused_luma_units_[e][k], e, k);
    if (units.empty()) return 0;
    const size_t bytes = units.size() * sizeof(WorkUnit);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;  // an earlier launch may still read the scratch buffer
    if (bytes > taken_units_cap_) {
        if (taken_units_dev_) (void)hipFree(taken_units_dev_);
        taken_units_dev_ = nullptr;
        taken_units_cap_ = 0;
        if (hipMalloc(&taken_units_dev_, bytes * 2) != hipSuccess) return -1;
        taken_units_cap_ = bytes * 2;
    }
    if (hipMemcpy(taken_units_dev_, units.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return -1;
    const WorkUnit* du = static_cast<const WorkUnit*>(taken_units_dev_);
    int rc = 0;
    for (const Run& r : runs) {
        if (rc != 0) break;
        rc = r.layout < 0 ? launch_idct_plane(dimg, du + r.first, (int)r.count, stream, fast_idct_)
                          : launch_luma_color(r.layout, kLumaHs[r.variant], kLumaVs[r.variant], dimg, du + r.first, (int)r.count, stream, fast_idct_);
    }
    return rc;
}

int DecodeBatch::launch_pixel_kernels(void* stream, int which)
{
    const DecodeImage* dimg = at<const DecodeImage>(device_, staging_.desc);
    auto dev = [&](const UnitList& l) { return at<const WorkUnit>(device_, l.offset); };
    auto count = [](const UnitList& l) { return (int)l.units.size(); };
    int rc = 0;
    HuffImage* himg = at<HuffImage>(device_, staging_.huff_desc);
    const unsigned pool_bytes = (unsigned)align_up(max_pool_words_ * 2, 256);
    if (rc == 0 && (which < 0 || which == 0)) {
        rc = launch_idct_plane(dimg, dev(plane_units_), count(plane_units_), stream, fast_idct_);
        debug_check(stream, "idct_plane", count(plane_units_));
        if (rc == 0) rc = launch_idct_plane_fused(dimg, dev(fused_plane_units_), count(fused_plane_units_), himg, pool_bytes, stream);
        debug_check(stream, "idct_plane_fused", count(fused_plane_units_));
        if (rc == 0) rc = launch_idct_reduced_plane(dimg, dev(reduced_units_), count(reduced_units_), stream);
        debug_check(stream, "idct_reduced_plane", count(reduced_units_));
    }
    for (int e = 0; e < kNumLumaLayouts; e++)
        for (int k = 0; k < kNumLumaVariants && rc == 0 && (which < 0 || which == 1); k++) {
            const UnitList &plain = luma_units_[e][k], &fused = fused_luma_units_[e][k];
            rc = launch_luma_color(e, kLumaHs[k], kLumaVs[k], dimg, dev(plain), count(plain), stream, fast_idct_);
            debug_check(stream, "luma_color", count(plain));
            if (rc == 0) rc = launch_luma_color_fused(e, kLumaHs[k], kLumaVs[k], dimg, dev(fused), count(fused), himg, pool_bytes, stream);
            debug_check(stream, "luma_color_fused", count(fused));
        }
    // images the host entropy decoder took over: the plain builds, on the coefficients it uploaded
    if (rc == 0 && !host_taken_.empty() && (which < 0 || which == 0 || which == 1)) rc = launch_taken_pixels(stream, which);
    if (rc == 0 && (which < 0 || which == 2)) {
        rc = launch_generic_color(dimg, dev(generic_units_), count(generic_units_), stream);
        debug_check(stream, "generic_color", count(generic_units_));
    }
    if (rc == 0 && (which < 0 || which == 2)) {
        rc = launch_cmyk_color(dimg, dev(cmyk_units_), count(cmyk_units_), stream);
        debug_check(stream, "cmyk_color", count(cmyk_units_));
    }
    if (rc == 0 && (which < 0 || which == 2)) {  // scaled images: behind K1 and the reduced kernel, which filled their planes
        rc = launch_scaled_color(dimg, dev(scaled_color_units_), count(scaled_color_units_), stream);
        debug_check(stream, "scaled_color", count(scaled_color_units_));
    }
    if (rc == 0 && (which < 0 || which == 4)) {
        rc = launch_transform(at<const TransformImage>(device_, staging_.xform_desc), dev(xform_units_), count(xform_units_), stream);
        debug_check(stream, "transform", count(xform_units_));
    }
    return rc;
}

hipjpegStatus_t DecodeBatch::launch(void* stream, int which, void* entropy_stream)
{
    if (!finalized_) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    ScopedRange range("hipjpeg device stage (launch)");
    fault_point("launch");
    if (debug_sync()) {
        for (size_t i = 0; i < images_.size(); i++) {
            const DecodeImage& d = desc_[i];
            fprintf(stderr, "[hipjpeg] img %zu st=%d var=%d %dx%d ncomp=%d hmax=%d vmax=%d coef=%p,%p,%p plane=%p,%p,%p pitch=%u,%u,%u out=%p opitch=%u\n",
                    i, (int)images_[i].status, images_[i].variant, (int)d.width, (int)d.height, (int)d.ncomp, (int)d.hmax, (int)d.vmax,
                    (const void*)d.comp[0].coef, (const void*)d.comp[1].coef, (const void*)d.comp[2].coef, (void*)d.comp[0].plane,
                    (void*)d.comp[1].plane, (void*)d.comp[2].plane, d.comp[0].plane_pitch, d.comp[1].plane_pitch, d.comp[2].plane_pitch,
                    (void*)d.out[0], d.out_pitch[0]);
        }
        fprintf(stderr, "[hipjpeg] device=%p+%zu planes=%p+%zu unit offs plane=%zu generic=%zu coef_off=%zu staging=%zu\n", (void*)device_.data(),
                device_.capacity(), (void*)planes_.data(), planes_.capacity(), plane_units_.offset, generic_units_.offset, staging_.coef, staging_.total);
        debug_check(stream, "transfer", 0);
    }
    last_stream_ = stream;
    // With an entropy stream the (latency-bound) entropy kernels of this batch run beside the (VALU-bound) pixel kernels of
    // the batch before it; the pixel kernels on `stream` wait for them on the device.
    void* es_stream = (entropy_stream && which < 0 && !entropy_done_ && !(huff_units_.empty() && prog_units_.empty())) ? entropy_stream : stream;
    if (copied_event_ && copy_pending_) {
        // the H2D copy went out on another stream: the kernels wait for it on the device, the host does not
        if (hipStreamWaitEvent((hipStream_t)es_stream, (hipEvent_t)copied_event_, 0) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        if (es_stream != stream && hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)copied_event_, 0) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        copy_pending_ = false;
    }
    if ((which < 0 && !entropy_done_) || which == 3 || which == 6) {
        hipjpegStatus_t es = enqueue_gpu_entropy(es_stream);
        if (es != HIPJPEG_STATUS_SUCCESS) return es;
        if (which == 3) return resolve(stream);
        if (es_stream != stream) {
            if (!ensure_event(&entropy_event_) || hipEventRecord((hipEvent_t)entropy_event_, (hipStream_t)es_stream) != hipSuccess ||
                hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)entropy_event_, 0) != hipSuccess)
                return HIPJPEG_STATUS_HIP_ERROR;
        }
    }
    if (which != 6 && launch_pixel_kernels(stream, which) != 0) return HIPJPEG_STATUS_HIP_ERROR;
    if (which < 0) pixels_launched_ = true;
    if (fused_ && entropy_pending_ && !huff_units_.empty() && (which < 0 || which == 1)) {
        // the FUSED pixel kernels are part of the entropy decode: a block they cannot decode flags its image -- the verdicts are
        // fetched behind them (the copy queued with the entropy stage saw the position pass's verdicts only)
        EntropyLaunch L = entropy_launch_args();
        if (hipMemcpyAsync(L.himg, L.dimg, sizeof(HuffImage) * huff_images_.size(), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess)
            return HIPJPEG_STATUS_HIP_ERROR;
    }
    if (!ensure_event(&done_event_) || hipEventRecord((hipEvent_t)done_event_, (hipStream_t)stream) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    in_flight_ = true;
    return HIPJPEG_STATUS_SUCCESS;
}

// ---------------------------------------------------------------- coefficient tensors
// plan_tensors(): the caller's planes as the kernel reads them and the units of coef_to_decoder_kernel, image by image (sized by
// size_image()); images that failed get neither.
void DecodeBatch::build_tensor_units()
{
    tensor_table_.clear();
    tensor_units_.clear();
    imported_blocks_ = 0;
    if (!tensor_source_) return;
    tensor_table_.assign(images_.size() * 4, CoefPlane{nullptr, 0, 0, 0, 0});
    for (size_t i = 0; i < images_.size() && tensor_planes_; i++) {
        const PlannedImage& im = images_[i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const hipjpegCoefficientPlanes_t& p = tensor_planes_[i];
        for (int c = 0; c < im.frame.ncomp; c++) {
            const Component& k = im.frame.comp[c];
            const uint32_t real_w = (uint32_t)(k.samp_w + 7) / 8, real_h = (uint32_t)(k.samp_h + 7) / 8;
            tensor_table_[i * 4 + (size_t)c] = CoefPlane{static_cast<int16_t*>(p.coef[c]), p.pitch_blocks[c], real_w, real_h, 0};
            // (over the MCU-padded grid: the kernel writes the padding too, as zeros)
            for (uint32_t b = 0; b < (uint32_t)k.blocks_w * (uint32_t)k.blocks_h; b += kRelayoutBlocksPerUnit)
                tensor_units_.push_back(RelayoutUnit{(uint32_t)i, (uint32_t)c, b, 0});
            imported_blocks_ += (uint64_t)real_w * real_h;
        }
    }
    tensor_planes_ = nullptr;
}

hipjpegStatus_t DecodeBatch::import_tensors(void* stream)
{
    if (!tensor_source_ || !finalized_) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (tensor_units_.empty()) return HIPJPEG_STATUS_SUCCESS;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    // HIPJPEG_DEBUG_TIMING (debug aid): the kernel's own time on stderr (tools/prof_coefficient_pixels.py reads it); the aid waits for the kernel
    static const bool timing = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (timing && (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess || hipEventRecord(t0, s) != hipSuccess)) return HIPJPEG_STATUS_HIP_ERROR;
    if (launch_coef_to_decoder(at<const CoefPlane>(device_, staging_.tensor_planes), device_descriptors(), at<const RelayoutUnit>(device_, staging_.tensor_units),
                               (int)tensor_units_.size(), stream) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    debug_check(stream, "coef_to_decoder", (int)tensor_units_.size());
    if (timing) {
        float ms = 0;
        if (hipEventRecord(t1, s) != hipSuccess || hipEventSynchronize(t1) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        (void)hipEventElapsedTime(&ms, t0, t1);
        fprintf(stderr, "[hipjpeg] coef_to_decoder_kernel: %zu workgroups, %llu blocks, %.4f ms\n", tensor_units_.size(), (unsigned long long)imported_blocks_, ms);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
    }
    // the kernel writes this page's coefficient arena and reads the staged tables: nothing rewrites them before it has run
    if (!ensure_event(&done_event_) || hipEventRecord((hipEvent_t)done_event_, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    in_flight_ = true;
    last_stream_ = stream;
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t DecodeBatch::export_coefficients(const hipjpegCoefficientPlanes_t* planes, void* stream)
{
    exported_blocks_ = 0;
    if (!coef_only_ || !finalized_ || (!planes && !images_.empty())) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    std::vector<CoefPlane> table(images_.size() * 4, CoefPlane{nullptr, 0, 0, 0, 0});
    std::vector<RelayoutUnit> units;
    for (size_t i = 0; i < images_.size(); i++) {
        const PlannedImage& im = images_[i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        for (int c = 0; c < im.frame.ncomp; c++) {
            const uint32_t real_w = (uint32_t)(im.frame.comp[c].samp_w + 7) / 8, real_h = (uint32_t)(im.frame.comp[c].samp_h + 7) / 8;
            table[i * 4 + c] = CoefPlane{static_cast<int16_t*>(planes[i].coef[c]), planes[i].pitch_blocks[c], real_w, real_h, 0};
            for (uint32_t b = 0; b < real_w * real_h; b += kRelayoutBlocksPerUnit) units.push_back(RelayoutUnit{(uint32_t)i, (uint32_t)c, b, 0});
            exported_blocks_ += (uint64_t)real_w * real_h;
        }
    }
    if (units.empty()) return HIPJPEG_STATUS_SUCCESS;
    // (the previous export of this page has drained: plan_coefficients() waited for the event recorded below)
    Carve carve;
    const size_t table_at = carve.take(sizeof(CoefPlane) * table.size()), units_at = carve.take(sizeof(RelayoutUnit) * units.size());
    hipjpegStatus_t st;
    if ((st = export_pinned_.reserve(carve.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = export_device_.reserve(carve.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    copy_table(export_pinned_, table_at, table);
    copy_table(export_pinned_, units_at, units);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(export_device_.data(), export_pinned_.data(), carve.end, hipMemcpyHostToDevice, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    // HIPJPEG_DEBUG_TIMING (debug aid): the kernel's own time on stderr (tools/prof_coefficients.py reads it); the aid waits for the kernel
    static const bool timing = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (timing && (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess || hipEventRecord(t0, s) != hipSuccess)) return HIPJPEG_STATUS_HIP_ERROR;
    if (launch_coef_export(device_descriptors(), at<const CoefPlane>(export_device_, table_at), at<const RelayoutUnit>(export_device_, units_at),
                           (int)units.size(), stream) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    debug_check(stream, "coef_export", (int)units.size());
    if (timing) {
        float ms = 0;
        if (hipEventRecord(t1, s) != hipSuccess || hipEventSynchronize(t1) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        (void)hipEventElapsedTime(&ms, t0, t1);
        fprintf(stderr, "[hipjpeg] coef_export_kernel: %zu workgroups, %llu blocks, %.4f ms\n", units.size(), (unsigned long long)exported_blocks_, ms);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
    }
    // the kernel reads this page's coefficient arena and the tables above: nothing rewrites them before it has run
    if (!ensure_event(&done_event_) || hipEventRecord((hipEvent_t)done_event_, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    in_flight_ = true;
    last_stream_ = stream;
    return HIPJPEG_STATUS_SUCCESS;
}

void DecodeBatch::output_size(int i, int* w, int* h) const
{
    const PlannedImage& im = images_[i];
    int ow = im.pic_w, oh = im.pic_h;
    if (im.has_transform) {
        const int rw = im.transform.x1 - im.transform.x0, rh = im.transform.y1 - im.transform.y0;
        ow = im.transform.orientation >= 5 ? rh : rw;
        oh = im.transform.orientation >= 5 ? rw : rh;
    }
    *w = ow;
    *h = oh;
}

// Work units of K1 and K2 (per layout) in the FUSED lists, and with `plain` in the plain ones as well.
void DecodeBatch::unit_counts(bool plain, int32_t* plane, int32_t luma[kNumLumaLayouts]) const
{
    *plane = (int32_t)((plain ? plane_units_.units.size() : 0) + fused_plane_units_.units.size());
    for (int e = 0; e < kNumLumaLayouts; e++) {
        luma[e] = 0;
        for (int k = 0; k < kNumLumaVariants; k++) luma[e] += (int32_t)((plain ? luma_units_[e][k].units.size() : 0) + fused_luma_units_[e][k].units.size());
    }
}

int DecodeBatch::fused_units() const
{
    int32_t plane = 0, luma[kNumLumaLayouts];
    unit_counts(false, &plane, luma);
    return std::accumulate(luma, luma + kNumLumaLayouts, plane);
}

void DecodeBatch::stats(int32_t num_units[3], uint64_t* coef_bytes, uint64_t* output_bytes) const
{
    if (num_units) {
        int32_t luma[kNumLumaLayouts];
        flavour_units(&num_units[0], luma);
        num_units[1] = std::accumulate(luma, luma + kNumLumaLayouts, 0);
        num_units[2] = (int32_t)generic_units_.units.size();
    }
    if (coef_bytes) *coef_bytes = coef_bytes_;
    if (output_bytes) *output_bytes = output_bytes_;
}

}  // namespace hipjpeg
