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

hipjpegStatus_t coefficient_frame(const hipjpegCoefficientInfo_t& info, const hipjpegCoefficientPlanes_t& planes, FrameInfo* out)
{
    if (info.width < 1 || info.height < 1 || info.width > 65535 || info.height > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    if (info.num_components < 1 || info.num_components > 4) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    FrameInfo f;
    f.width = info.width;
    f.height = info.height;
    f.precision = 8;
    f.ncomp = info.num_components;
    f.sof = 0xC0;
    for (int c = 0; c < f.ncomp; c++) {
        if (info.h[c] < 1 || info.h[c] > 4 || info.v[c] < 1 || info.v[c] > 4) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        f.hmax = std::max(f.hmax, info.h[c]);
        f.vmax = std::max(f.vmax, info.v[c]);
    }
    // (jpeg_syntax.cpp finish_frame)
    f.mcus_x = (f.width + 8 * f.hmax - 1) / (8 * f.hmax);
    f.mcus_y = (f.height + 8 * f.vmax - 1) / (8 * f.vmax);
    for (int c = 0; c < f.ncomp; c++) {
        Component& k = f.comp[c];
        k.id = c + 1;
        k.h = info.h[c];
        k.v = info.v[c];
        k.blocks_w = f.mcus_x * k.h;
        k.blocks_h = f.mcus_y * k.v;
        k.samp_w = (f.width * k.h + f.hmax - 1) / f.hmax;
        k.samp_h = (f.height * k.v + f.vmax - 1) / f.vmax;
        if (info.blocks_w[c] != (k.samp_w + 7) / 8 || info.blocks_h[c] != (k.samp_h + 7) / 8) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        memcpy(f.qtab[c], info.qtable[c], sizeof f.qtab[c]);
    }
    const hipjpegStatus_t st = coefficient_planes_ok(f.ncomp, info.blocks_w, planes);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    if (f.ncomp == 4 || f.ncomp == 2) return HIPJPEG_STATUS_UNSUPPORTED;
    if (f.ncomp == 1)
        f.color = ColorModel::Gray;
    else if (info.color_model < (int32_t)ColorModel::Gray || info.color_model > (int32_t)ColorModel::RGB)
        return HIPJPEG_STATUS_UNSUPPORTED;
    else
        f.color = (ColorModel)info.color_model;
    *out = f;
    return HIPJPEG_STATUS_SUCCESS;
}

void encode_coefficient_info(const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], hipjpegCoefficientInfo_t* info)
{
    memset(info, 0, sizeof *info);
    info->width = g.width;
    info->height = g.height;
    info->num_components = g.ncomp;
    info->color_model = (int32_t)(g.ncomp == 1 ? ColorModel::Gray : ColorModel::YCbCr);
    for (int c = 0; c < g.ncomp; c++) {
        info->h[c] = c == 0 ? g.hs : 1;
        info->v[c] = c == 0 ? g.vs : 1;
        info->blocks_w[c] = g.real_w[c];
        info->blocks_h[c] = g.real_h[c];
        memcpy(info->qtable[c], c == 0 ? qlum : qchr, sizeof info->qtable[c]);
    }
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

extern "C" hipjpegStatus_t hipjpegGetEncodeCoefficientInfo(int32_t width, int32_t height, const hipjpegEncodeParams_t* params, hipjpegCoefficientInfo_t* info)
{
    return guarded([&]() -> hipjpegStatus_t {
        if (!params || !info) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        memset(info, 0, sizeof *info);
        EncodeGeometry g;
        uint16_t ql[64], qc[64];
        const hipjpegStatus_t st = picture_setup(*params, width, height, &g, ql, qc);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        encode_coefficient_info(g, ql, qc, info);
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
