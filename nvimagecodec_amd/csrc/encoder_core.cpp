// encoder_core.cpp -- see encoder_core.h
#include "encoder_core.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "coefficients_core.h"
#include "encode_kernels.h"
#include "huffman_encode_core.h"
#include "jpeg_syntax.h"
#include "progressive_encode.h"

namespace hipjpeg {

namespace {
constexpr int kTileBX = 32, kTileBY = 8;
constexpr size_t kHistBytes = 2 * 2 * 256 * sizeof(uint32_t);  // one image's symbol counts: [table][DC / AC][symbol]

// forward_pair_kernel's chroma sampling and input layout per flavour (hs = 0: not a pair flavour)
struct PairFlavour { int hs, vs; bool planar; };
constexpr PairFlavour kPair[kNumFwdFlavours] = {{0, 0, false}, {2, 2, false}, {2, 1, false}, {1, 1, false},
                                                {0, 0, false}, {2, 2, true},  {2, 1, true},  {1, 1, true}};
// launch order on the stream
constexpr EncodeFlavour kLaunchOrder[kNumFwdFlavours] = {kFwdOneLane,       kFwdPair420,       kFwdPair422,       kFwdPair444,
                                                         kFwdPlanarPair420, kFwdPlanarPair422, kFwdPlanarPair444, kFwdPlanes};

// The pair flavour of RGB / BGR input in (hs, vs) sampling, or the one-lane kernel when the pair kernel has no such flavour.
EncodeFlavour pair_flavour(int hs, int vs, bool planar)
{
    for (int f = 0; f < kNumFwdFlavours; f++)
        if (kPair[f].hs == hs && kPair[f].vs == vs && kPair[f].planar == planar) return (EncodeFlavour)f;
    return kFwdOneLane;
}
}  // namespace

EntropyEncodeOptions entropy_options(const hipjpegEncodeParams_t& p)
{
    return EntropyEncodeOptions{p.restart_interval, p.optimized_huffman != 0, p.progressive != 0};
}

EncodeBatch::EncodeBatch(int device_id, const MemoryHooks* hooks)
    : device_id_(device_id), pinned_desc_(Buffer::kPinned, hooks), device_(Buffer::kDevice, hooks), pinned_coef_(Buffer::kPinned, hooks),
      planes_pinned_(Buffer::kPinned, hooks), planes_device_(Buffer::kDevice, hooks),
      henc_(hooks), penc_(hooks)
{
}

EncodeBatch::~EncodeBatch()
{
    if (event_) {
        if (launched_) (void)hipEventSynchronize((hipEvent_t)event_);
        (void)hipEventDestroy((hipEvent_t)event_);
    }
}

const int16_t* EncodeBatch::host_coef(int i, int c) const { return at<const int16_t>(pinned_coef_, images_[i].coef_offset[c]); }

// ---------------------------------------------------------------- device_stage
hipjpegStatus_t EncodeBatch::device_stage(const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params, int n,
                                          hipjpegStatus_t* statuses, void* stream)
{
    if (n < 0 || (n > 0 && (!inputs || !params))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    if (launched_ && event_) (void)hipEventSynchronize((hipEvent_t)event_);  // previous use of the buffers must have drained
    launched_ = fetched_ = false;
    images_.assign(n, PlannedEncode());
    desc_.assign(n, EncodeImage());
    host_coder_.assign(n, 0);
    markers_.assign((size_t)n, std::vector<uint8_t>());
    units_.clear();
    relayout_units_.clear();
    coef_planes_.clear();
    for (auto& v : unit_lists_) v.clear();
    coef_total_ = 0;
    pixel_bytes_ = coef_bytes_ = 0;
    for (int i = 0; i < n; i++) prepare(i, inputs[i], params[i]);
    layout();
    hipjpegStatus_t st;
    if ((st = reserve()) != HIPJPEG_STATUS_SUCCESS) return st;
    bind_pointers();
    if (statuses)
        for (int i = 0; i < n; i++) statuses[i] = images_[i].status;
    stream_ = stream;
    if (staging_.coef && hipMemcpyAsync(device_.data(), pinned_desc_.data(), staging_.coef, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    return relaunch(stream);
}

// Checks, geometry, quantiser tables, descriptor and work units of image i.
void EncodeBatch::prepare(int i, const hipjpegEncodeInput_t& in, const hipjpegEncodeParams_t& p)
{
    PlannedEncode& im = images_[i];
    im.params = p;
    const EncodeGeometry& g = im.geom;
    const int fmt = p.input_format;
    // An unknown subsampling ends the checks.  After it every failing check overwrites the status: of several problems the
    // last one checked is reported.
    im.status = picture_setup(p, in.width, in.height, &im.geom, im.qlum, im.qchr);
    if (im.status == HIPJPEG_STATUS_UNSUPPORTED) return;
    if (fmt != HIPJPEG_OUTPUT_RGBI && fmt != HIPJPEG_OUTPUT_BGRI && fmt != HIPJPEG_OUTPUT_RGB_PLANAR && fmt != HIPJPEG_OUTPUT_BGR_PLANAR &&
        fmt != HIPJPEG_OUTPUT_Y && fmt != HIPJPEG_OUTPUT_YUV_PLANAR)
        im.status = HIPJPEG_STATUS_UNSUPPORTED;
    if (fmt == HIPJPEG_OUTPUT_Y && g.ncomp != 1) im.status = HIPJPEG_STATUS_UNSUPPORTED;  // gray pixels carry no chroma
    if (fmt == HIPJPEG_OUTPUT_YUV_PLANAR && g.ncomp != 3) im.status = HIPJPEG_STATUS_UNSUPPORTED;
    const int nplanes = (fmt == HIPJPEG_OUTPUT_RGB_PLANAR || fmt == HIPJPEG_OUTPUT_BGR_PLANAR || fmt == HIPJPEG_OUTPUT_YUV_PLANAR) ? 3 : 1;
    for (int c = 0; c < nplanes; c++)
        if (!in.plane[c]) im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (p.restart_interval < 0 || p.restart_interval > 65535) im.status = HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (im.status != HIPJPEG_STATUS_SUCCESS) return;

    EncodeImage& d = desc_[i];
    memset(&d, 0, sizeof d);
    d.width = (uint32_t)g.width;
    d.height = (uint32_t)g.height;
    d.ncomp = (uint32_t)g.ncomp;
    d.hs = (uint32_t)g.hs;
    d.vs = (uint32_t)g.vs;
    d.in_format = fmt == HIPJPEG_OUTPUT_Y ? (uint32_t)kInGray : (uint32_t)fmt;  // RGBI/BGRI/planar/YUV values coincide with InFormat
    for (int c = 0; c < 3; c++) {
        d.in[c] = static_cast<const uint8_t*>(in.plane[c]);
        d.in_pitch[c] = in.pitch[c];
    }
    for (int c = 0; c < g.ncomp; c++) {
        d.blocks_w[c] = (uint32_t)g.blocks_w[c];
        d.blocks_h[c] = (uint32_t)g.blocks_h[c];
        d.real_w[c] = (uint32_t)g.real_w[c];
        d.real_h[c] = (uint32_t)g.real_h[c];
        im.coef_offset[c] = coef_total_;
        coef_total_ += (size_t)g.blocks_w[c] * g.blocks_h[c] * 128;
    }
    for (int t = 0; t < 2; t++) {
        const uint16_t* q = t ? im.qchr : im.qlum;
        for (int k = 0; k < 64; k++) {
            const uint32_t div = 8u * q[kZigzagNatural[k]];
            d.quant[t].magic[k] = (1u << 28) / div + 1;
            d.quant[t].half[k] = div >> 1;
            const int nat = kZigzagNatural[k], tr = (nat & 7) * 8 + (nat >> 3);
            d.qnat[t].magic[tr] = d.quant[t].magic[k];
            d.qnat[t].half16[tr] = (div >> 1) << 4;
        }
    }
    add_units(i, fmt);
    pixel_bytes_ += (uint64_t)g.width * g.height * (g.ncomp == 1 ? 1 : 3);
    for (int c = 0; c < g.ncomp; c++) coef_bytes_ += (uint64_t)g.real_w[c] * g.real_h[c] * 128;
}

// Work units of image i on the list of its flavour.
void EncodeBatch::add_units(int i, int fmt)
{
    const EncodeGeometry& g = images_[i].geom;
    if (fmt == HIPJPEG_OUTPUT_YUV_PLANAR) {
        // planes that are components already: one lane per real block of each component
        for (int c = 0; c < 3; c++)
            for (int b = 0; b < g.real_w[c] * g.real_h[c]; b += 256) unit_lists_[kFwdPlanes].push_back(EncodeUnit{(uint32_t)i, (uint32_t)b, 0u, (uint32_t)c});
        return;
    }
    // Interleaved or planar RGB / BGR into 4:2:0 / 4:2:2 / 4:4:4 has a kernel of its own (encode_kernels.hip forward_pair_kernel).
    // HIPJPEG_ENCODE_ONE_LANE_KERNEL (read per batch) sends everything to the one-lane-per-block kernel: the cross-check
    // campaigns compare the two on the same pixels.
    EncodeFlavour flavour = kFwdOneLane;
    const bool interleaved = fmt == HIPJPEG_OUTPUT_RGBI || fmt == HIPJPEG_OUTPUT_BGRI;
    const bool planar_rgb = fmt == HIPJPEG_OUTPUT_RGB_PLANAR || fmt == HIPJPEG_OUTPUT_BGR_PLANAR;
    if (g.ncomp == 3 && (interleaved || planar_rgb) && getenv("HIPJPEG_ENCODE_ONE_LANE_KERNEL") == nullptr) flavour = pair_flavour(g.hs, g.vs, planar_rgb);
    // tiles cover the real luma blocks only
    const int tiles_x = (g.real_w[0] + kTileBX - 1) / kTileBX, tiles_y = (g.real_h[0] + kTileBY - 1) / kTileBY;
    for (int ty = 0; ty < tiles_y; ty++)
        for (int tx = 0; tx < tiles_x; tx++) unit_lists_[flavour].push_back(EncodeUnit{(uint32_t)i, (uint32_t)tx, (uint32_t)ty, 0u});
}

// One units table, the flavours back to back, and the descriptor arena around it.
void EncodeBatch::layout()
{
    for (int f = 0; f < kNumFwdFlavours; f++) {
        unit_first_[f] = units_.size();
        units_.insert(units_.end(), unit_lists_[f].begin(), unit_lists_[f].end());
    }
    Carve c;
    staging_.desc = c.take(sizeof(EncodeImage) * desc_.size());
    staging_.units = c.take(sizeof(EncodeUnit) * units_.size());
    staging_.relayout = c.take(sizeof(RelayoutUnit) * relayout_units_.size());
    staging_.flags = c.take(relayout_units_.empty() ? 0 : sizeof(uint32_t) * images_.size());
    staging_.planes = c.take(sizeof(CoefPlane) * coef_planes_.size());
    staging_.coef = c.take(coef_total_);
    staging_.total = c.end;
}

hipjpegStatus_t EncodeBatch::reserve()
{
    hipjpegStatus_t st;
    if ((st = pinned_desc_.reserve(staging_.coef + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = device_.reserve(staging_.total + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    return pinned_coef_.reserve(coef_total_ + 256);
}

void EncodeBatch::bind_pointers()
{
    for (int i = 0; i < (int)images_.size(); i++) {
        if (images_[i].status != HIPJPEG_STATUS_SUCCESS) continue;
        for (int c = 0; c < images_[i].geom.ncomp; c++) desc_[i].coef[c] = at<int16_t>(device_, staging_.coef + images_[i].coef_offset[c]);
    }
    copy_table(pinned_desc_, staging_.desc, desc_);
    copy_table(pinned_desc_, staging_.units, units_);
    copy_table(pinned_desc_, staging_.relayout, relayout_units_);
    copy_table(pinned_desc_, staging_.planes, coef_planes_);
    if (!relayout_units_.empty()) memset(pinned_desc_.data() + staging_.flags, 0, sizeof(uint32_t) * images_.size());
}

hipjpegStatus_t EncodeBatch::relaunch(void* stream)
{
    const EncodeImage* dimg = at<const EncodeImage>(device_, staging_.desc);
    int rc = 0;
    for (int k = 0; k < kNumFwdFlavours && rc == 0; k++) {
        const EncodeFlavour f = kLaunchOrder[k];
        const EncodeUnit* u = at<const EncodeUnit>(device_, staging_.units) + unit_first_[f];
        const int nu = (int)unit_lists_[f].size();
        rc = f == kFwdOneLane ? launch_forward(dimg, u, nu, stream)
           : f == kFwdPlanes  ? launch_forward_planes(dimg, u, nu, stream)
                              : launch_forward_pair(kPair[f].hs, kPair[f].vs, kPair[f].planar, dimg, u, nu, stream);
    }
    if (rc != 0) return HIPJPEG_STATUS_HIP_ERROR;
    if (!event_) {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        event_ = ev;
    }
    if (hipEventRecord((hipEvent_t)event_, (hipStream_t)stream) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    launched_ = true;
    fetched_ = false;
    stream_ = stream;
    return HIPJPEG_STATUS_SUCCESS;
}

// ---------------------------------------------------------------- coefficient_stage
hipjpegStatus_t EncodeBatch::coefficient_stage(const CoefficientPicture* pics, int n, const DecodeImage* src, void* stream)
{
    if (n > 0 && !src) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return coefficient_fill(pics, n, src, nullptr, stream);
}

hipjpegStatus_t EncodeBatch::import_stage(const CoefficientPicture* pics, const hipjpegCoefficientPlanes_t* planes, int n, void* stream)
{
    if (n > 0 && !planes) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return coefficient_fill(pics, n, nullptr, planes, stream);
}

hipjpegStatus_t EncodeBatch::coefficient_fill(const CoefficientPicture* pics, int n, const DecodeImage* src, const hipjpegCoefficientPlanes_t* planes,
                                              void* stream)
{
    if (n < 0 || (n > 0 && !pics)) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    if (launched_ && event_) (void)hipEventSynchronize((hipEvent_t)event_);  // previous use of the buffers must have drained
    launched_ = fetched_ = false;
    images_.assign(n, PlannedEncode());
    desc_.assign(n, EncodeImage());
    host_coder_.assign(n, 0);
    markers_.assign((size_t)n, std::vector<uint8_t>());
    units_.clear();
    relayout_units_.clear();
    coef_planes_.assign(planes ? (size_t)n * 4 : 0, CoefPlane{nullptr, 0, 0, 0, 0});
    for (auto& v : unit_lists_) v.clear();
    coef_total_ = 0;
    pixel_bytes_ = coef_bytes_ = 0;
    relayout_blocks_ = 0;
    gpu_entropy_images_ = 0;
    std::vector<RelayoutUnit> turned;
    uint64_t turned_blocks = 0;
    for (int i = 0; i < n; i++) {
        PlannedEncode& im = images_[i];
        im.status = pics[i].status;
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        im.geom = pics[i].picture.geom;
        im.params = pics[i].params;
        memcpy(im.qlum, pics[i].picture.qlum, sizeof im.qlum);
        memcpy(im.qchr, pics[i].picture.qchr, sizeof im.qchr);
        markers_[(size_t)i] = pics[i].markers;
        const EncodeGeometry& g = im.geom;
        // cropped at an origin: the turned kernel, with turn 0 if need be (the origin of the unit's component rides behind the turn)
        // (caller memory holds the picture itself: neither turn nor origin)
        const bool moved = !planes && (pics[i].turn != 0 || pics[i].origin.any());
        EncodeImage& d = desc_[i];
        memset(&d, 0, sizeof d);
        d.width = (uint32_t)g.width;
        d.height = (uint32_t)g.height;
        d.ncomp = (uint32_t)g.ncomp;
        d.hs = (uint32_t)g.hs;
        d.vs = (uint32_t)g.vs;
        for (int c = 0; c < g.ncomp; c++) {
            d.blocks_w[c] = (uint32_t)g.blocks_w[c];
            d.blocks_h[c] = (uint32_t)g.blocks_h[c];
            d.real_w[c] = (uint32_t)g.real_w[c];
            d.real_h[c] = (uint32_t)g.real_h[c];
            im.coef_offset[c] = coef_total_;
            coef_total_ += (size_t)g.blocks_w[c] * g.blocks_h[c] * 128;
            const uint32_t nreal = (uint32_t)(g.real_w[c] * g.real_h[c]);
            std::vector<RelayoutUnit>& list = moved ? turned : relayout_units_;
            const uint32_t pad = planes ? 0u : pics[i].turn | ((uint32_t)pics[i].origin.ox[c] << kOriginShiftX) | ((uint32_t)pics[i].origin.oy[c] << kOriginShiftY);
            if (planes)
                coef_planes_[(size_t)i * 4 + c] = CoefPlane{static_cast<int16_t*>(planes[i].coef[c]), planes[i].pitch_blocks[c], (uint32_t)g.real_w[c], (uint32_t)g.real_h[c], 0};
            for (uint32_t b = 0; b < nreal; b += kRelayoutBlocksPerUnit) list.push_back(RelayoutUnit{(uint32_t)i, (uint32_t)c, b, pad});
            relayout_blocks_ += nreal;
            if (moved) turned_blocks += nreal;
        }
    }
    identity_units_ = relayout_units_.size();
    relayout_units_.insert(relayout_units_.end(), turned.begin(), turned.end());
    coef_bytes_ = relayout_blocks_ * 128;
    layout();
    hipjpegStatus_t st;
    if ((st = reserve()) != HIPJPEG_STATUS_SUCCESS) return st;
    bind_pointers();
    stream_ = stream;
    hipStream_t s = (hipStream_t)stream;
    if (staging_.coef && hipMemcpyAsync(device_.data(), pinned_desc_.data(), staging_.coef, hipMemcpyHostToDevice, s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    // HIPJPEG_DEBUG_TIMING (debug aid, as in the decode host stage): the kernel's own time on stderr (tools/prof_transcode.py reads it)
    static const bool timing = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr;
    if (timing && (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess || hipEventCreate(&t2) != hipSuccess || hipEventRecord(t0, s) != hipSuccess))
        return HIPJPEG_STATUS_HIP_ERROR;
    const EncodeImage* dimg = at<const EncodeImage>(device_, staging_.desc);
    const RelayoutUnit* dunits = at<const RelayoutUnit>(device_, staging_.relayout);
    const int nturned = (int)(relayout_units_.size() - identity_units_);
    const int rc = planes ? launch_coef_import(at<const CoefPlane>(device_, staging_.planes), dimg, dunits, (int)identity_units_, at<uint32_t>(device_, staging_.flags), stream)
                          : launch_coef_relayout(src, dimg, dunits, (int)identity_units_, at<uint32_t>(device_, staging_.flags), stream);
    if (rc != 0) return HIPJPEG_STATUS_HIP_ERROR;
    if (timing && hipEventRecord(t1, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    if (launch_coef_transform(src, dimg, dunits + identity_units_, nturned, at<uint32_t>(device_, staging_.flags), stream) != 0) return HIPJPEG_STATUS_HIP_ERROR;
    if (timing && hipEventRecord(t2, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    uint32_t* flags = at<uint32_t>(pinned_desc_, staging_.flags);
    if (!relayout_units_.empty() &&
        hipMemcpyAsync(flags, device_.data() + staging_.flags, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (!event_) {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        event_ = ev;
    }
    if (hipEventRecord((hipEvent_t)event_, s) != hipSuccess || hipEventSynchronize((hipEvent_t)event_) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    launched_ = true;
    if (timing) {
        float ms = 0, ms_turned = 0;
        (void)hipEventSynchronize(t2);
        (void)hipEventElapsedTime(&ms, t0, t1);
        (void)hipEventElapsedTime(&ms_turned, t1, t2);
        if (identity_units_ || !nturned)
            fprintf(stderr, "[hipjpeg] %s: %zu workgroups, %llu blocks, %.4f ms\n", planes ? "coef_import_kernel" : "coef_relayout_kernel", identity_units_,
                    (unsigned long long)(relayout_blocks_ - turned_blocks), ms);
        if (nturned)
            fprintf(stderr, "[hipjpeg] coef_transform_kernel: %d workgroups, %llu blocks, %.4f ms\n", nturned, (unsigned long long)turned_blocks, ms_turned);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
        (void)hipEventDestroy(t2);
    }
    // the range guard: such values are outside what the coders' tables cover, so no coder gets to see them
    for (int i = 0; i < n && !relayout_units_.empty(); i++)
        if (images_[i].status == HIPJPEG_STATUS_SUCCESS && flags[i] != 0) images_[i].status = HIPJPEG_STATUS_UNSUPPORTED;
    return HIPJPEG_STATUS_SUCCESS;
}

// ---------------------------------------------------------------- planes_stage
hipjpegStatus_t EncodeBatch::planes_stage(const hipjpegCoefficientPlanes_t* planes, hipjpegStatus_t* statuses, void* stream)
{
    planes_blocks_ = 0;
    const size_t n = images_.size();
    if (!launched_ || stream != stream_ || (n > 0 && !planes)) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    std::vector<CoefPlane> table(n * 4, CoefPlane{nullptr, 0, 0, 0, 0});
    std::vector<RelayoutUnit> units;
    for (size_t i = 0; i < n; i++) {
        PlannedEncode& im = images_[i];
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        const EncodeGeometry& g = im.geom;
        const int32_t real_w[4] = {g.real_w[0], g.real_w[1], g.real_w[2], 0};
        im.status = coefficient_planes_ok(g.ncomp, real_w, planes[i]);
        if (statuses) statuses[i] = im.status;
        if (im.status != HIPJPEG_STATUS_SUCCESS) continue;
        for (int c = 0; c < g.ncomp; c++) {
            const uint32_t nreal = (uint32_t)(g.real_w[c] * g.real_h[c]);
            table[i * 4 + (size_t)c] = CoefPlane{static_cast<int16_t*>(planes[i].coef[c]), planes[i].pitch_blocks[c], (uint32_t)g.real_w[c], (uint32_t)g.real_h[c], 0};
            for (uint32_t b = 0; b < nreal; b += kRelayoutBlocksPerUnit) units.push_back(RelayoutUnit{(uint32_t)i, (uint32_t)c, b, 0});
            planes_blocks_ += nreal;
        }
    }
    if (units.empty()) return HIPJPEG_STATUS_SUCCESS;
    // (the previous use of these two buffers has drained: device_stage() waited for the event recorded below)
    Carve carve;
    const size_t table_at = carve.take(sizeof(CoefPlane) * table.size()), units_at = carve.take(sizeof(RelayoutUnit) * units.size());
    hipjpegStatus_t st;
    if ((st = planes_pinned_.reserve(carve.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = planes_device_.reserve(carve.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    copy_table(planes_pinned_, table_at, table);
    copy_table(planes_pinned_, units_at, units);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(planes_device_.data(), planes_pinned_.data(), carve.end, hipMemcpyHostToDevice, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    // HIPJPEG_DEBUG_TIMING (debug aid): the kernel's own time on stderr (tools/prof_coefficient_pixels.py reads it); the aid waits for the kernel
    static const bool timing = getenv("HIPJPEG_DEBUG_TIMING") != nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (timing && (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess || hipEventRecord(t0, s) != hipSuccess)) return HIPJPEG_STATUS_HIP_ERROR;
    if (launch_coef_from_coder(at<const EncodeImage>(device_, staging_.desc), at<const CoefPlane>(planes_device_, table_at),
                               at<const RelayoutUnit>(planes_device_, units_at), (int)units.size(), stream) != 0)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (timing) {
        float ms = 0;
        if (hipEventRecord(t1, s) != hipSuccess || hipEventSynchronize(t1) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
        (void)hipEventElapsedTime(&ms, t0, t1);
        fprintf(stderr, "[hipjpeg] coef_from_coder_kernel: %zu workgroups, %llu blocks, %.4f ms\n", units.size(), (unsigned long long)planes_blocks_, ms);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
    }
    // the kernel reads the coefficient area and the tables above: nothing rewrites them before it has run
    if (hipEventRecord((hipEvent_t)event_, s) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t EncodeBatch::fetch_coefficients()
{
    if (!launched_) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (fetched_) return HIPJPEG_STATUS_SUCCESS;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    if (coef_total_ &&
        hipMemcpyAsync(pinned_coef_.data(), device_.data() + staging_.coef, coef_total_, hipMemcpyDeviceToHost, (hipStream_t)stream_) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    if (hipEventRecord((hipEvent_t)event_, (hipStream_t)stream_) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    if (hipEventSynchronize((hipEvent_t)event_) != hipSuccess) return HIPJPEG_STATUS_HIP_ERROR;
    fetched_ = true;
    return HIPJPEG_STATUS_SUCCESS;
}

// ---------------------------------------------------------------- entropy coding
hipjpegStatus_t EncodeBatch::route_entropy(bool gpu_huffman, bool gpu_restart, bool gpu_progressive_restart)
{
    for (size_t i = 0; i < images_.size(); i++) host_coder_[i] = images_[i].status == HIPJPEG_STATUS_SUCCESS;
    hipjpegStatus_t st;
    if (gpu_huffman && (st = gpu_entropy_stage(gpu_restart, gpu_progressive_restart)) != HIPJPEG_STATUS_SUCCESS) return st;
    host_images_ = (int)std::count(host_coder_.begin(), host_coder_.end(), 1);
    // the host coder needs the coefficients on its side of PCIe
    return host_images_ ? fetch_coefficients() : HIPJPEG_STATUS_SUCCESS;
}

void EncodeBatch::entropy_stage(int i)
{
    PlannedEncode& im = images_[i];
    if (!host_coder_[i] || im.status != HIPJPEG_STATUS_SUCCESS) return;
    const int16_t* coef[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < im.geom.ncomp; c++) coef[c] = host_coef(i, c);
    im.bitstream.clear();
    im.gpu_bitstream = nullptr;
    im.gpu_bitstream_len = 0;
    EntropyEncodeOptions opt = entropy_options(im.params);
    opt.markers = markers_of(i);
    encode_jfif(im.geom, im.qlum, im.qchr, coef, opt, &im.bitstream);
}

// ---------------------------------------------------------------- GPU entropy coder
namespace {
// Baseline output.  Phase-1 device arena (henc_.dev): descriptors | length units | standard tables | optimized tables [the upload,
// staged at the same offsets at the start of henc_.pinned) | block bit lengths | block bit offsets | total bits | histograms
struct HencLayout1 {
    size_t desc, units, tables, opt_tables, bits, off, totals, hist, end;
    size_t upload() const { return bits; }
};
// Progressive output (progressive_encode.h).  Phase-1 device arena (penc_.dev): scans | length units | AC scans | segment descriptors
// [the upload, staged at the same offsets at the start of penc_.pinned) | code tables [uploaded after the statistics] | symbol counts |
// per block: summaries, pre / post flushes, pieces, flushers, rel, own bits, bits, offsets | total bits per scan.
struct PencLayout1 {
    size_t scans, units, ac, segs, codes, hist, sum, pre, post, piece, flusher, rel, own, bits, off, totals, end;
};
// Either flavour's pinned arena behind what phase 1 stages in it: symbol counts | total bits per segment | segment lengths | segment
// offsets | phase-2 upload (at the phase-2 arena's offsets; last, because its size follows from the total bits: `end` is set then)
struct HencPinnedLayout { size_t hist, totals, len, foff, up2, end; };
// Phase-2 device arena (dev2): segment descriptors | chunk units | headers [the upload) | 0xFF counts per chunk | chunk outputs |
// segment lengths | segment offsets | bit buffers | files (unused when they go straight to `out`)
struct HencLayout2 {
    size_t desc, units, headers, ff, out, len, foff, raw, arena, end;
    size_t upload() const { return ff; }
};

HencPinnedLayout henc_pinned_layout(size_t start, size_t hist_bytes, size_t nseg)
{
    Carve c{start};
    HencPinnedLayout p;
    p.hist = c.take(hist_bytes);
    p.totals = c.take(nseg * 4);
    p.len = c.take(nseg * 4);
    p.foff = c.take(nseg * 8);
    p.up2 = p.end = c.take(0);
    return p;
}
}  // namespace

struct EncodeBatch::SegmentPlan {
    std::vector<int> idx;                       // images taken, in batch order: one file each
    std::vector<int> first_seg;                 // per file: index of its first segment (one more entry: the end)
    std::vector<HencImage> segs;                // every segment of those files: the scan / count / layout / expand kernels' descriptors
    std::vector<std::vector<uint8_t>> headers;  // per segment: baseline SOI .. SOS; progressive [frame header] DHT.. SOS
    std::vector<HencUnit> chunk_units;          // count / expand units (kHencChunk bytes of one segment each)
    std::vector<size_t> raw_off, hdr_off;       // per segment: offsets inside the bit-buffer area and the header area
    size_t raw_total = 0, hdr_total = 0, arena_cap = 0;
    HencPinnedLayout pin{};
    HencLayout2 d2{};
};

struct EncodeBatch::HencPlan : SegmentPlan {
    std::vector<HencUnit> units;  // length / write units (256 blocks each)
    std::vector<int> opt_slot;    // slot among the images with tables of their own (optimized_huffman), or -1
    bool restart = false;         // an image has restart intervals: every launch takes the kernels' flavour that carries them
    int nopt = 0;
    size_t total_blocks = 0;  // entries of the per-block arrays
    HencLayout1 d1{};
};

struct EncodeBatch::PencPlan : SegmentPlan {
    std::vector<PencScan> scans;     // every scan of the images taken, one per segment (device pointers inside)
    std::vector<HencUnit> units;     // length / write units (256 blocks of one scan, image = scan)
    std::vector<uint32_t> ac_scans;  // scans with end-of-band runs
    bool restart = false;            // an image has restart intervals: every launch takes the kernels' flavour that carries them
    size_t total_blocks = 0;
    PencLayout1 d1{};
};

hipjpegStatus_t EncodeBatch::gpu_entropy_stage(bool gpu_restart, bool gpu_progressive_restart)
{
    gpu_entropy_images_ = 0;
    if (!launched_) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (hipSetDevice(device_id_) != hipSuccess) return HIPJPEG_STATUS_NO_DEVICE;
    HencPlan p;
    PencPlan q;
    henc_choose(p, q, gpu_restart, gpu_progressive_restart);
    hipjpegStatus_t st;
    if (!p.idx.empty()) {
        const HencLayout1& d1 = p.d1;
        const auto write = [&](const HencImage* dsegs) {
            return launch_henc_write(dsegs, at<const HencUnit>(henc_.dev, d1.units), (int)p.units.size(), at<const StandardCodeTables>(henc_.dev, d1.tables),
                                     at<const uint32_t>(henc_.dev, d1.off), at<const uint16_t>(henc_.dev, d1.bits), stream_, p.restart);
        };
        bool direct = false;
        henc_describe(p);
        if ((st = henc_stage_phase1(p)) != HIPJPEG_STATUS_SUCCESS || (p.nopt > 0 && (st = henc_histograms(p)) != HIPJPEG_STATUS_SUCCESS) ||
            (st = henc_lengths(p)) != HIPJPEG_STATUS_SUCCESS)
            return st;
        henc_chunks(p, henc_);
        if ((st = henc_assemble(p, henc_, write, &direct, p.restart)) != HIPJPEG_STATUS_SUCCESS || (st = henc_collect(p, henc_, direct)) != HIPJPEG_STATUS_SUCCESS)
            return st;
    }
    if (!q.idx.empty()) {
        const PencLayout1& d1 = q.d1;
        const auto write = [&](const HencImage* dsegs) {
            const Buffer& dev = penc_.dev;
            const PencBlockArrays a{at<const uint8_t>(dev, d1.sum),    at<const uint32_t>(dev, d1.pre),     at<const uint32_t>(dev, d1.post),
                                    at<const uint32_t>(dev, d1.piece), at<const uint32_t>(dev, d1.flusher), at<const uint16_t>(dev, d1.rel),
                                    at<const uint16_t>(dev, d1.own),   at<const uint16_t>(dev, d1.bits),    at<const uint32_t>(dev, d1.off)};
            return launch_penc_write(at<const PencScan>(dev, d1.scans), dsegs, at<const HencUnit>(dev, d1.units), (int)q.units.size(), a, stream_, q.restart);
        };
        bool direct = false;
        penc_describe(q);
        if ((st = penc_statistics(q)) != HIPJPEG_STATUS_SUCCESS || (st = penc_lengths(q)) != HIPJPEG_STATUS_SUCCESS) return st;
        henc_chunks(q, penc_);
        if ((st = henc_assemble(q, penc_, write, &direct, q.restart)) != HIPJPEG_STATUS_SUCCESS || (st = henc_collect(q, penc_, direct)) != HIPJPEG_STATUS_SUCCESS) return st;
    }
    return HIPJPEG_STATUS_SUCCESS;
}

// Every image the host coder would code and the GPU coder takes: baseline ones into p, progressive ones into q.  Restart intervals:
// baseline images when the caller asked for them (HIPJPEG_FLAG_GPU_RESTART_INTERVALS), progressive ones when the caller asked for those
// (HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART: jcphuff.c emit_restart also flushes the EOB run, progressive_encode_core.h); the two switches
// are independent.
void EncodeBatch::henc_choose(HencPlan& p, PencPlan& q, bool gpu_restart, bool gpu_progressive_restart)
{
    for (int i = 0; i < (int)images_.size(); i++) {
        PlannedEncode& im = images_[i];
        im.gpu_bitstream = nullptr;
        im.gpu_bitstream_len = 0;
        if (!host_coder_[i] || (im.params.restart_interval != 0 && !(im.params.progressive ? gpu_progressive_restart : gpu_restart))) continue;
        host_coder_[i] = 0;
        (im.params.progressive ? q.idx : p.idx).push_back(i);
    }
}

// Descriptors, length units, table slots and the standard headers of the images taken.
void EncodeBatch::henc_describe(HencPlan& p)
{
    const int ng = (int)p.idx.size();
    p.segs.resize(ng);
    p.opt_slot.assign(ng, -1);
    p.headers.resize(ng);
    for (int g = 0; g < ng; g++) {
        const PlannedEncode& im = images_[p.idx[g]];
        const EncodeGeometry& eg = im.geom;
        HencImage& h = p.segs[g];
        memset(&h, 0, sizeof h);
        for (int c = 0; c < eg.ncomp; c++) {
            h.coef[c] = desc_[p.idx[g]].coef[c];
            h.blocks_w[c] = (uint32_t)eg.blocks_w[c];
            h.real_w[c] = (uint32_t)eg.real_w[c];
            h.real_h[c] = (uint32_t)eg.real_h[c];
        }
        h.mcus_x = (uint32_t)eg.mcus_x;
        h.mcus_y = (uint32_t)eg.mcus_y;
        h.ncomp = (uint32_t)eg.ncomp;
        h.hs = (uint32_t)eg.hs;
        h.vs = (uint32_t)eg.vs;
        h.bpm = eg.ncomp == 3 ? (uint32_t)(eg.hs * eg.vs + 2) : 1u;
        h.total_blocks = h.mcus_x * h.mcus_y * h.bpm;
        h.first_block = (uint32_t)p.total_blocks;
        h.rst_blocks = (uint32_t)im.params.restart_interval * h.bpm;
        if (h.rst_blocks) p.restart = true;
        h.nseg = 1;  // a baseline file is one segment, with or without restart intervals
        h.last_seg = 1;
        p.first_seg.push_back(g);
        for (uint32_t b = 0; b < h.total_blocks; b += 256) p.units.push_back(HencUnit{(uint32_t)g, b});
        p.total_blocks += (h.total_blocks + 63) & ~(size_t)63;
        if (im.params.optimized_huffman) p.opt_slot[g] = p.nopt++;
        write_standard_headers(eg, im.qlum, im.qchr, &p.headers[g], im.params.restart_interval, markers_of(p.idx[g]));
    }
    p.first_seg.push_back(ng);
}

// Lays out the phase-1 device arena and the start of henc_.pinned; stages descriptors, units and standard tables.
hipjpegStatus_t EncodeBatch::henc_stage_phase1(HencPlan& p)
{
    const int ng = (int)p.idx.size();
    HencLayout1& d1 = p.d1;
    Carve c;
    d1.desc = c.take(sizeof(HencImage) * (size_t)ng);
    d1.units = c.take(sizeof(HencUnit) * p.units.size());
    d1.tables = c.take(sizeof(StandardCodeTables));
    d1.opt_tables = c.take(sizeof(StandardCodeTables) * (size_t)p.nopt);
    d1.bits = c.take(p.total_blocks * 2);
    d1.off = c.take(p.total_blocks * 4);
    d1.totals = c.take((size_t)ng * 4);
    d1.hist = c.take(kHistBytes * (size_t)p.nopt);
    d1.end = c.take(0);
    p.pin = henc_pinned_layout(d1.upload(), kHistBytes * (size_t)p.nopt, (size_t)ng);
    // henc_.pinned grows again in phase 2, after the totals have been read (reserve() keeps no contents)
    hipjpegStatus_t st;
    if ((st = henc_.dev.reserve(d1.end + 256)) != HIPJPEG_STATUS_SUCCESS || (st = henc_.pinned.reserve(p.pin.up2 + 256)) != HIPJPEG_STATUS_SUCCESS)
        return st;
    copy_table(henc_.pinned, d1.desc, p.segs);
    copy_table(henc_.pinned, d1.units, p.units);
    standard_code_tables(at<StandardCodeTables>(henc_.pinned, d1.tables));
    return HIPJPEG_STATUS_SUCCESS;
}

// Phase 0: symbol statistics on the device, optimal tables on the host (a few dozen microseconds per image); the tables go up
// with phase 1.  The coefficients never leave HBM; what crosses PCIe is 4 KB of counts and 1.6 KB of tables per image.
hipjpegStatus_t EncodeBatch::henc_histograms(HencPlan& p)
{
    const HencLayout1& d1 = p.d1;
    const size_t hist_bytes = kHistBytes * (size_t)p.nopt;
    hipStream_t s = (hipStream_t)stream_;
    for (size_t g = 0; g < p.idx.size(); g++)
        if (p.opt_slot[g] >= 0) p.segs[g].hist = at<uint32_t>(henc_.dev, d1.hist + kHistBytes * (size_t)p.opt_slot[g]);
    copy_table(henc_.pinned, d1.desc, p.segs);
    if (hipMemcpyAsync(henc_.dev.data(), henc_.pinned.data(), d1.opt_tables, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(henc_.dev.data() + d1.hist, 0, hist_bytes, s) != hipSuccess ||
        launch_henc_hist(at<const HencImage>(henc_.dev, d1.desc), at<const HencUnit>(henc_.dev, d1.units), (int)p.units.size(), stream_, p.restart) != 0 ||
        hipMemcpyAsync(henc_.pinned.data() + p.pin.hist, henc_.dev.data() + d1.hist, hist_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    for (size_t g = 0; g < p.idx.size(); g++) {
        const int k = p.opt_slot[g];
        if (k < 0) continue;
        const PlannedEncode& im = images_[p.idx[g]];
        const auto* counts = at<const uint32_t[2][256]>(henc_.pinned, p.pin.hist + kHistBytes * (size_t)k);
        const size_t tables = d1.opt_tables + sizeof(StandardCodeTables) * (size_t)k;
        p.headers[g].clear();
        optimal_code_tables(counts, im.geom, im.qlum, im.qchr, at<StandardCodeTables>(henc_.pinned, tables), &p.headers[g], im.params.restart_interval,
                            markers_of(p.idx[(size_t)g]));
        p.segs[g].hist = nullptr;
        p.segs[g].tables = at<const StandardCodeTables>(henc_.dev, tables);
    }
    copy_table(henc_.pinned, d1.desc, p.segs);
    return HIPJPEG_STATUS_SUCCESS;
}

// Phase 1: descriptors, units and tables up; block lengths, their prefix sums, and every image's total bits back.
hipjpegStatus_t EncodeBatch::henc_lengths(HencPlan& p)
{
    const HencLayout1& d1 = p.d1;
    const int ng = (int)p.idx.size();
    const HencImage* dimg = at<const HencImage>(henc_.dev, d1.desc);
    hipStream_t s = (hipStream_t)stream_;
    if (hipMemcpyAsync(henc_.dev.data(), henc_.pinned.data(), d1.upload(), hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_henc_length(dimg, at<const HencUnit>(henc_.dev, d1.units), (int)p.units.size(), at<const StandardCodeTables>(henc_.dev, d1.tables),
                           at<uint16_t>(henc_.dev, d1.bits), stream_, p.restart) != 0 ||
        launch_henc_scan(dimg, ng, at<const uint16_t>(henc_.dev, d1.bits), at<uint32_t>(henc_.dev, d1.off), at<uint32_t>(henc_.dev, d1.totals), stream_,
                         p.restart) != 0 ||
        hipMemcpyAsync(henc_.pinned.data() + p.pin.totals, henc_.dev.data() + d1.totals, (size_t)ng * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

// ---------------------------------------------------------------- GPU entropy coder, progressive output
// Scans, units, segments and the frame headers of the progressive images taken.
void EncodeBatch::penc_describe(PencPlan& q)
{
    const int ng = (int)q.idx.size();
    for (int g = 0; g < ng; g++) {
        const PlannedEncode& im = images_[q.idx[g]];
        const int16_t* coef[3] = {desc_[q.idx[g]].coef[0], desc_[q.idx[g]].coef[1], desc_[q.idx[g]].coef[2]};
        const size_t s0 = q.scans.size();
        q.first_seg.push_back((int)s0);
        q.total_blocks += hipjpeg::penc_describe(im.geom, coef, q.total_blocks, &q.scans, im.params.restart_interval);
        if (im.params.restart_interval) q.restart = true;
        for (size_t k = s0; k < q.scans.size(); k++) {
            const PencScan& sc = q.scans[k];
            for (uint32_t b = 0; b < sc.nblocks; b += 256) q.units.push_back(HencUnit{(uint32_t)k, b});
            if (sc.kind >= kPencAcFirst) q.ac_scans.push_back((uint32_t)k);
            HencImage h;
            memset(&h, 0, sizeof h);
            h.total_blocks = sc.nblocks;  // what henc_scan reads
            h.first_block = sc.first_block;
            // what henc_scan, henc_chunks (the marker bitmap behind the bit buffer) and count / expand read: a segment that writes
            // markers without it would write past its buffer
            h.rst_blocks = sc.rst_blocks;
            h.nseg = k == s0 ? (uint32_t)(q.scans.size() - s0) : 0u;
            h.last_seg = k + 1 == q.scans.size() ? 1u : 0u;
            q.segs.push_back(h);
            q.headers.emplace_back();
        }
        write_progressive_frame_header(im.geom, im.qlum, im.qchr, &q.headers[s0], markers_of(q.idx[g]));
    }
    q.first_seg.push_back((int)q.scans.size());
}

// Phase 0: descriptors up; block summaries, run resolution and the symbol counts of every scan on the device; the counts back in one
// copy (1 KB per scan); optimal tables, DHT and SOS per scan on the host.
hipjpegStatus_t EncodeBatch::penc_statistics(PencPlan& q)
{
    const size_t ns = q.scans.size(), nb = q.total_blocks;
    PencLayout1& d1 = q.d1;
    Carve c;
    d1.scans = c.take(sizeof(PencScan) * ns);
    d1.units = c.take(sizeof(HencUnit) * q.units.size());
    d1.ac = c.take(4 * q.ac_scans.size());
    d1.segs = c.take(sizeof(HencImage) * ns);
    d1.codes = c.take(1024 * ns);
    d1.hist = c.take(1024 * ns);
    d1.sum = c.take(nb);
    d1.pre = c.take(4 * nb);
    d1.post = c.take(4 * nb);
    d1.piece = c.take(4 * nb);
    d1.flusher = c.take(4 * nb);
    d1.rel = c.take(2 * nb);
    d1.own = c.take(2 * nb);
    d1.bits = c.take(2 * nb);
    d1.off = c.take(4 * nb);
    d1.totals = c.take(4 * ns);
    d1.end = c.take(0);
    q.pin = henc_pinned_layout(d1.hist, 1024 * ns, ns);
    hipjpegStatus_t st;
    if ((st = penc_.dev.reserve(d1.end + 256)) != HIPJPEG_STATUS_SUCCESS || (st = penc_.pinned.reserve(q.pin.up2 + 256)) != HIPJPEG_STATUS_SUCCESS)
        return st;
    for (size_t k = 0; k < ns; k++) {
        PencScan& sc = q.scans[k];
        sc.hist = sc.kind == kPencDcRefine ? nullptr : at<uint32_t>(penc_.dev, d1.hist + 1024 * k);
        sc.codes = at<const uint32_t>(penc_.dev, d1.codes + 1024 * k);
    }
    copy_table(penc_.pinned, d1.scans, q.scans);
    copy_table(penc_.pinned, d1.units, q.units);
    copy_table(penc_.pinned, d1.ac, q.ac_scans);
    copy_table(penc_.pinned, d1.segs, q.segs);
    const PencScan* dscans = at<const PencScan>(penc_.dev, d1.scans);
    uint8_t* dev = penc_.dev.data();
    hipStream_t s = (hipStream_t)stream_;
    if (hipMemcpyAsync(dev, penc_.pinned.data(), d1.codes, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(dev + d1.hist, 0, 1024 * ns, s) != hipSuccess || hipMemsetAsync(dev + d1.pre, 0, 4 * nb, s) != hipSuccess ||
        hipMemsetAsync(dev + d1.post, 0, 4 * nb, s) != hipSuccess ||
        launch_penc_summary(dscans, at<const HencUnit>(penc_.dev, d1.units), (int)q.units.size(), dev + d1.sum, stream_, q.restart) != 0 ||
        launch_penc_runs(dscans, at<const uint32_t>(penc_.dev, d1.ac), (int)q.ac_scans.size(), dev + d1.sum, at<uint32_t>(penc_.dev, d1.pre),
                         at<uint32_t>(penc_.dev, d1.post), at<uint32_t>(penc_.dev, d1.piece), at<uint32_t>(penc_.dev, d1.flusher),
                         at<uint16_t>(penc_.dev, d1.rel), stream_, q.restart) != 0 ||
        hipMemcpyAsync(penc_.pinned.data() + q.pin.hist, dev + d1.hist, 1024 * ns, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    for (size_t g = 0; g + 1 < q.first_seg.size(); g++) {
        const std::vector<ScanSpec> script = simple_progression(images_[q.idx[g]].geom.ncomp);
        for (int k = q.first_seg[g]; k < q.first_seg[g + 1]; k++)  // DRI once, in the first scan's header
            progressive_scan_header(script[k - q.first_seg[g]], at<const uint32_t>(penc_.pinned, q.pin.hist + 1024 * (size_t)k),
                                    at<uint32_t>(penc_.pinned, d1.codes + 1024 * (size_t)k), &q.headers[k],
                                    k == q.first_seg[g] ? images_[q.idx[g]].params.restart_interval : 0);
    }
    return HIPJPEG_STATUS_SUCCESS;
}

// Phase 1: the code tables up; block lengths, their prefix sums per scan, and every scan's total bits back.
hipjpegStatus_t EncodeBatch::penc_lengths(PencPlan& q)
{
    const PencLayout1& d1 = q.d1;
    const int ns = (int)q.scans.size();
    hipStream_t s = (hipStream_t)stream_;
    if (hipMemcpyAsync(penc_.dev.data() + d1.codes, penc_.pinned.data() + d1.codes, d1.hist - d1.codes, hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_penc_length(at<const PencScan>(penc_.dev, d1.scans), at<const HencUnit>(penc_.dev, d1.units), (int)q.units.size(),
                           at<const uint32_t>(penc_.dev, d1.pre), at<const uint32_t>(penc_.dev, d1.post), at<uint16_t>(penc_.dev, d1.own),
                           at<uint16_t>(penc_.dev, d1.bits), stream_, q.restart) != 0 ||
        launch_henc_scan(at<const HencImage>(penc_.dev, d1.segs), ns, at<const uint16_t>(penc_.dev, d1.bits), at<uint32_t>(penc_.dev, d1.off),
                         at<uint32_t>(penc_.dev, d1.totals), stream_, q.restart) != 0 ||
        hipMemcpyAsync(penc_.pinned.data() + q.pin.totals, penc_.dev.data() + d1.totals, (size_t)ns * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

// ---------------------------------------------------------------- GPU entropy coder, phase 2 of either flavour
// From the total bits: every segment's bit buffer, stuffing chunks and header slot, and the capacity of the file arena.
void EncodeBatch::henc_chunks(SegmentPlan& p, const HencArenas& a)
{
    const uint32_t* totals = at<const uint32_t>(a.pinned, p.pin.totals);
    Carve raw, hdr;  // the bit-buffer area and the header area of the phase-2 arena
    p.raw_off.resize(p.segs.size());
    p.hdr_off.resize(p.segs.size());
    for (size_t f = 0; f < p.idx.size(); f++) {
        size_t file_bytes = 2;  // EOI
        for (int k = p.first_seg[f]; k < p.first_seg[f + 1]; k++) {
            HencImage& h = p.segs[k];
            h.raw_bytes = (totals[k] + 7) / 8;
            h.first_chunk = (uint32_t)p.chunk_units.size();
            h.num_chunks = (h.raw_bytes + kHencChunk - 1) / kHencChunk;
            for (uint32_t c = 0; c < h.num_chunks; c++) p.chunk_units.push_back(HencUnit{(uint32_t)k, c});
            h.header_bytes = (uint32_t)p.headers[k].size();
            // a segment with restart intervals: the markers are part of raw_bytes (the scan counted them), and the marker bitmap lies
            // behind the buffer -- zeroed with it, one bit per byte (huffman_encode_core.h)
            p.raw_off[k] = raw.take(h.rst_blocks ? (size_t)henc_map_offset(h.raw_bytes) + henc_map_bytes(h.raw_bytes) : (size_t)h.raw_bytes + 16);
            p.hdr_off[k] = hdr.take(p.headers[k].size(), 16);
            file_bytes += (size_t)h.header_bytes + 2 * (size_t)h.raw_bytes;  // every byte could be 0xFF (a marker's is, and is not stuffed)
        }
        // as henc_layout_kernel places them: a file's segments back to back, every file at a 16-byte boundary
        p.arena_cap += align_up(file_bytes, 16);
    }
    p.raw_total = raw.take(0);
    p.hdr_total = hdr.take(0, 16);
}

// Phase 2: bit buffers (`write`: the flavour's kernel that fills them), stuffing, assembly of the segments into files; segment
// lengths and offsets back.  The finished files go straight into pinned host memory when it is ours (hipHostMalloc: mapped into the
// device's address space): the expand kernel's stores cross PCIe themselves and no copy follows.  With a caller-supplied pinned
// allocator the mapping is unknown, so the files are assembled in HBM.
template <class Write>
hipjpegStatus_t EncodeBatch::henc_assemble(SegmentPlan& p, HencArenas& a, Write write, bool* direct, bool restart)
{
    const int ns = (int)p.segs.size();
    const size_t nchunks = p.chunk_units.size();
    HencLayout2& d2 = p.d2;
    Carve c;
    d2.desc = c.take(sizeof(HencImage) * (size_t)ns);
    d2.units = c.take(sizeof(HencUnit) * nchunks);
    d2.headers = c.take(p.hdr_total);
    d2.ff = c.take(nchunks * 4);
    d2.out = c.take(nchunks * 4);
    d2.len = c.take((size_t)ns * 4);
    d2.foff = c.take((size_t)ns * 8);
    d2.raw = c.take(p.raw_total);
    d2.arena = c.take(p.arena_cap);
    d2.end = c.end;
    p.pin.end = p.pin.up2 + d2.upload();
    hipjpegStatus_t st;
    if ((st = a.dev2.reserve(d2.end + 256)) != HIPJPEG_STATUS_SUCCESS || (st = a.pinned.reserve(p.pin.end + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
    for (int k = 0; k < ns; k++) {
        p.segs[k].raw = a.dev2.data() + d2.raw + p.raw_off[k];
        p.segs[k].header = a.dev2.data() + d2.headers + p.hdr_off[k];
        copy_table(a.pinned, p.pin.up2 + d2.headers + p.hdr_off[k], p.headers[k]);
    }
    copy_table(a.pinned, p.pin.up2 + d2.desc, p.segs);
    copy_table(a.pinned, p.pin.up2 + d2.units, p.chunk_units);
    *direct = a.out.reserve(p.arena_cap + 256) == HIPJPEG_STATUS_SUCCESS && !a.out.custom();
    const HencImage* dsegs = at<const HencImage>(a.dev2, d2.desc);
    const HencUnit* dchunks = at<const HencUnit>(a.dev2, d2.units);
    uint32_t *chunk_ff = at<uint32_t>(a.dev2, d2.ff), *chunk_out = at<uint32_t>(a.dev2, d2.out), *len = at<uint32_t>(a.dev2, d2.len);
    unsigned long long* foff = at<unsigned long long>(a.dev2, d2.foff);
    hipStream_t s = (hipStream_t)stream_;
    if (hipMemcpyAsync(a.dev2.data(), a.pinned.data() + p.pin.up2, d2.upload(), hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_henc_zero(a.dev2.data() + d2.raw, p.raw_total, stream_) != 0 || write(dsegs) != 0 ||
        launch_henc_count(dsegs, dchunks, (int)nchunks, chunk_ff, stream_, restart) != 0 ||
        launch_henc_layout(dsegs, ns, chunk_ff, chunk_out, len, foff, stream_) != 0 ||
        launch_henc_expand(dsegs, dchunks, (int)nchunks, chunk_out, len, foff, *direct ? a.out.data() : a.dev2.data() + d2.arena, stream_, restart) != 0 ||
        hipMemcpyAsync(a.pinned.data() + p.pin.len, len, (size_t)ns * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(a.pinned.data() + p.pin.foff, foff, (size_t)ns * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return HIPJPEG_STATUS_HIP_ERROR;
    return HIPJPEG_STATUS_SUCCESS;
}

// The files' places in `out` (copied down first when they were assembled in HBM): a file starts at its first segment and runs
// over all of them.
hipjpegStatus_t EncodeBatch::henc_collect(SegmentPlan& p, HencArenas& a, bool direct)
{
    const uint32_t* len = at<const uint32_t>(a.pinned, p.pin.len);
    const unsigned long long* foff = at<const unsigned long long>(a.pinned, p.pin.foff);
    size_t used = 0;  // the end of the last file, padded as henc_layout_kernel pads it
    for (size_t f = 0; f < p.idx.size(); f++) {
        PlannedEncode& im = images_[p.idx[f]];
        im.gpu_bitstream_len = 0;
        for (int k = p.first_seg[f]; k < p.first_seg[f + 1]; k++) im.gpu_bitstream_len += len[k];
        used = (size_t)foff[p.first_seg[f]] + align_up(im.gpu_bitstream_len, 16);
    }
    if (used > p.arena_cap) return HIPJPEG_STATUS_HIP_ERROR;  // cannot happen: the capacity assumes every byte is stuffed
    if (!direct) {
        hipjpegStatus_t st;
        if ((st = a.out.reserve(used + 256)) != HIPJPEG_STATUS_SUCCESS) return st;
        if (hipMemcpyAsync(a.out.data(), a.dev2.data() + p.d2.arena, used, hipMemcpyDeviceToHost, (hipStream_t)stream_) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream_) != hipSuccess)
            return HIPJPEG_STATUS_HIP_ERROR;
    }
    for (size_t f = 0; f < p.idx.size(); f++) images_[p.idx[f]].gpu_bitstream = a.out.data() + foff[p.first_seg[f]];
    gpu_entropy_images_ += (uint64_t)p.idx.size();
    return HIPJPEG_STATUS_SUCCESS;
}

}  // namespace hipjpeg
