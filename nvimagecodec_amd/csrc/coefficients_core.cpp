// coefficients_core.cpp -- see coefficients_core.h
#include "coefficients_core.h"

#include <algorithm>
#include <cstring>
#include <new>

namespace hipjpeg {

hipjpegStatus_t coefficient_parse_status(ParseStatus ps)
{
    return ps == kParseOk ? HIPJPEG_STATUS_SUCCESS : ps == kParseUnsupported ? HIPJPEG_STATUS_UNSUPPORTED : ps == kParseTruncated ? HIPJPEG_STATUS_TRUNCATED : HIPJPEG_STATUS_BAD_JPEG;
}

void coefficient_info(const FrameInfo& f, hipjpegCoefficientInfo_t* info)
{
    memset(info, 0, sizeof *info);
    info->width = f.width;
    info->height = f.height;
    info->num_components = f.ncomp;
    info->color_model = (int32_t)f.color;
    NaturalPlanes area;
    natural_area(f, &area);
    for (int c = 0; c < f.ncomp; c++) {
        info->h[c] = f.comp[c].h;
        info->v[c] = f.comp[c].v;
        info->blocks_w[c] = area.blocks_w[c];
        info->blocks_h[c] = area.blocks_h[c];
        memcpy(info->qtable[c], f.qtab[c], sizeof info->qtable[c]);
    }
}

hipjpegStatus_t coefficient_planes_ok(int ncomp, const int32_t blocks_w[4], const hipjpegCoefficientPlanes_t& planes)
{
    for (int c = 0; c < ncomp; c++) {
        if (!planes.coef[c] || (reinterpret_cast<uintptr_t>(planes.coef[c]) & 15u) != 0) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        if (blocks_w[c] < 0 || planes.pitch_blocks[c] < (uint32_t)blocks_w[c]) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    }
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t coefficient_picture(const hipjpegCoefficientInfo_t& info, const hipjpegCoefficientPlanes_t& planes, const hipjpegTranscodeParams_t& params,
                                    TranscodePicture* pic)
{
    if (params.orientation != 0 || transcode_params_ok(params) != HIPJPEG_STATUS_SUCCESS) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (info.width < 1 || info.height < 1 || info.width > 65535 || info.height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    // a component count or a sampling factor no JPEG frame has: nothing the writer writes, and no geometry to judge the rest by
    if (info.num_components < 1 || info.num_components > 4) return HIPJPEG_STATUS_UNSUPPORTED;
    // the frame the `info` describes, as the parser would hand it on
    FrameInfo f;
    f.width = info.width;
    f.height = info.height;
    f.precision = 8;
    f.ncomp = info.num_components;
    f.sof = 0xC0;
    f.color = (ColorModel)info.color_model;
    for (int c = 0; c < f.ncomp; c++) {
        if (info.h[c] < 1 || info.h[c] > 4 || info.v[c] < 1 || info.v[c] > 4) return HIPJPEG_STATUS_UNSUPPORTED;
        f.hmax = std::max(f.hmax, info.h[c]);
        f.vmax = std::max(f.vmax, info.v[c]);
    }
    for (int c = 0; c < f.ncomp; c++) {
        Component& k = f.comp[c];
        k.h = info.h[c];
        k.v = info.v[c];
        k.samp_w = (f.width * k.h + f.hmax - 1) / f.hmax;
        k.samp_h = (f.height * k.v + f.vmax - 1) / f.vmax;
        // (the grid transcode_picture measures the coder's real area against: here the caller's own real area)
        k.blocks_w = (k.samp_w + 7) / 8;
        k.blocks_h = (k.samp_h + 7) / 8;
        if (info.blocks_w[c] != k.blocks_w || info.blocks_h[c] != k.blocks_h) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        memcpy(f.qtab[c], info.qtable[c], sizeof f.qtab[c]);
    }
    const hipjpegStatus_t st = coefficient_planes_ok(f.ncomp, info.blocks_w, planes);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    return transcode_picture(f, /*grayscale=*/false, pic);
}

}  // namespace hipjpeg

using namespace hipjpeg;

namespace {
template <class F>
hipjpegStatus_t guarded(F&& body) noexcept  // no C++ exception crosses the C boundary
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return HIPJPEG_STATUS_ALLOC_FAILED;
    } catch (...) {
        return HIPJPEG_STATUS_INTERNAL_ERROR;
    }
}

NaturalPlanes natural_planes(int ncomp, const int32_t blocks_w[4], const int32_t blocks_h[4], const hipjpegCoefficientPlanes_t& planes)
{
    NaturalPlanes p;
    for (int c = 0; c < ncomp; c++) {
        p.coef[c] = static_cast<int16_t*>(planes.coef[c]);
        p.pitch[c] = planes.pitch_blocks[c];
        p.blocks_w[c] = blocks_w[c];
        p.blocks_h[c] = blocks_h[c];
    }
    return p;
}
}  // namespace

// The host calls live here, not in hipjpeg_api.cpp, so that they link without the HIP runtime (tests/sanitizers).
extern "C" hipjpegStatus_t hipjpegGetCoefficientInfo(const uint8_t* data, size_t length, hipjpegCoefficientInfo_t* info)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!data || !info) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        memset(info, 0, sizeof *info);
        FrameInfo f;
        const hipjpegStatus_t st = coefficient_parse_status(parse_jpeg(data, length, &f));
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        coefficient_info(f, info);
        return HIPJPEG_STATUS_SUCCESS;
    });
}

extern "C" hipjpegStatus_t hipjpegDecodeCoefficientsHost(const uint8_t* data, size_t length, const hipjpegCoefficientPlanes_t* planes)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!data || !planes) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        FrameInfo f;
        hipjpegStatus_t st = coefficient_parse_status(parse_jpeg(data, length, &f));
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        hipjpegCoefficientInfo_t info;
        coefficient_info(f, &info);
        if ((st = coefficient_planes_ok(f.ncomp, info.blocks_w, *planes)) != HIPJPEG_STATUS_SUCCESS) return st;
        return decode_natural(data, length, f, natural_planes(f.ncomp, info.blocks_w, info.blocks_h, *planes));
    });
}

extern "C" hipjpegStatus_t hipjpegEncodeCoefficientsHost(const hipjpegCoefficientInfo_t* info, const hipjpegCoefficientPlanes_t* planes,
                                                         const hipjpegTranscodeParams_t* params, uint8_t* out, size_t capacity, size_t* out_length)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!info || !planes || !params || !out_length) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        TranscodePicture pic;
        hipjpegStatus_t st = coefficient_picture(*info, *planes, *params, &pic);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        std::vector<uint8_t> bytes;
        st = encode_natural(pic, natural_planes(pic.geom.ncomp, info->blocks_w, info->blocks_h, *planes), TranscodeOrigin(), 0u, transcode_options(*params), &bytes);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        *out_length = bytes.size();
        if (!out || capacity < bytes.size()) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
        memcpy(out, bytes.data(), bytes.size());
        return HIPJPEG_STATUS_SUCCESS;
    });
}
