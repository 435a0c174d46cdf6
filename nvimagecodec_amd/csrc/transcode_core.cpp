// transcode_core.cpp -- see transcode_core.h
#include "transcode_core.h"

#include <cstring>
#include <new>

#include "entropy_decode.h"

namespace hipjpeg {

hipjpegStatus_t transcode_picture(const FrameInfo& f, bool grayscale, TranscodePicture* p)
{
    if (f.precision != 8 || (f.sof != 0xC0 && f.sof != 0xC1 && f.sof != 0xC2)) return HIPJPEG_STATUS_UNSUPPORTED;
    if (f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535) return HIPJPEG_STATUS_UNSUPPORTED;
    EncodeGeometry& g = p->geom;
    g = EncodeGeometry();
    g.width = f.width;
    g.height = f.height;
    if (f.ncomp == 1) {
        // one component: its sampling factors mean nothing (the scan is not interleaved), the writer says 1x1
        g.ncomp = 1;
        g.hs = g.vs = 1;
    } else if (grayscale && f.ncomp == 3 && f.color == ColorModel::YCbCr) {
        // the luma component alone, written as one-component files are; it must cover the frame at full resolution
        if (f.comp[0].h != f.hmax || f.comp[0].v != f.vmax) return HIPJPEG_STATUS_UNSUPPORTED;
        g.ncomp = 1;
        g.hs = g.vs = 1;
    } else if (f.ncomp == 3 && f.color == ColorModel::YCbCr) {
        g.ncomp = 3;
        g.hs = f.comp[0].h;
        g.vs = f.comp[0].v;
        for (int c = 1; c < 3; c++)
            if (f.comp[c].h != 1 || f.comp[c].v != 1) return HIPJPEG_STATUS_UNSUPPORTED;
        const bool known = (g.vs == 1 && (g.hs == 1 || g.hs == 2 || g.hs == 4)) || (g.vs == 2 && (g.hs == 1 || g.hs == 2 || g.hs == 4));
        if (!known) return HIPJPEG_STATUS_UNSUPPORTED;
        if (memcmp(f.qtab[1], f.qtab[2], sizeof f.qtab[1]) != 0) return HIPJPEG_STATUS_UNSUPPORTED;  // the writer has one chroma table
    } else {
        return HIPJPEG_STATUS_UNSUPPORTED;
    }
    for (int c = 0; c < g.ncomp; c++)
        for (int j = 0; j < 64; j++)
            if (f.qtab[c][j] > 255 || f.qtab[c][j] == 0) return HIPJPEG_STATUS_UNSUPPORTED;  // the writer emits 8-bit DQTs
    compute_geometry(&g);
    // the decoder's grid must hold the blocks the coder reads (it always does: both pad to whole MCUs of the same frame)
    for (int c = 0; c < g.ncomp; c++)
        if (g.real_w[c] > f.comp[c].blocks_w || g.real_h[c] > f.comp[c].blocks_h) return HIPJPEG_STATUS_UNSUPPORTED;
    memcpy(p->qlum, f.qtab[0], sizeof p->qlum);
    memcpy(p->qchr, f.qtab[g.ncomp == 3 ? 1 : 0], sizeof p->qchr);
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t transcode_params_ok(const hipjpegTranscodeParams_t& p)
{
    if (p.restart_interval < 0 || p.restart_interval > 65535) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    const uint32_t o = (uint32_t)p.orientation, value = o & ~kTranscodeFlags;
    // (the identity is written 0: a 1 in this field was INVALID_ARGUMENT while the field was reserved, and callers rely on that)
    if (value == 1 || value > 8 || (value != 0 && (o & HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF))) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    return HIPJPEG_STATUS_SUCCESS;
}

int transcode_orientation(const hipjpegTranscodeParams_t& p, const uint8_t* data, size_t size)
{
    if (p.orientation & HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF) return exif_orientation(data, size);
    const int value = p.orientation & 15;
    return value == 0 ? 1 : value;
}

hipjpegStatus_t transcode_crop(const TranscodePicture& src, const hipjpegTranscodeRegion_t* region, bool expand, TranscodePicture* dst,
                               TranscodeOrigin* origin)
{
    *dst = src;
    *origin = TranscodeOrigin();
    if (!region || (region->x0 == 0 && region->y0 == 0 && region->x1 == 0 && region->y1 == 0)) return HIPJPEG_STATUS_SUCCESS;
    const EncodeGeometry& s = src.geom;
    int x0 = region->x0, y0 = region->y0;
    const int x1 = region->x1, y1 = region->y1;
    if (x0 < 0 || x0 >= x1 || x1 > s.width || y0 < 0 || y0 >= y1 || y1 > s.height) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    const int mcu_w = 8 * s.hs, mcu_h = 8 * s.vs;  // (one component: 8 x 8)
    if (x0 % mcu_w != 0 || y0 % mcu_h != 0) {
        if (!expand) return HIPJPEG_STATUS_UNSUPPORTED;
        x0 -= x0 % mcu_w;
        y0 -= y0 % mcu_h;
    }
    EncodeGeometry& g = dst->geom;
    g = EncodeGeometry();
    g.ncomp = s.ncomp;
    g.width = x1 - x0;
    g.height = y1 - y0;
    g.hs = s.hs;
    g.vs = s.vs;
    compute_geometry(&g);
    // component c starts at block (x0 / 8 * h_c / hs, y0 / 8 * v_c / vs): whole iMCUs in front of it, h_c x v_c blocks each
    for (int c = 0; c < g.ncomp; c++) {
        origin->ox[c] = c == 0 ? x0 / 8 : x0 / mcu_w;
        origin->oy[c] = c == 0 ? y0 / 8 : y0 / mcu_h;
    }
    return HIPJPEG_STATUS_SUCCESS;
}

void transcode_markers(const hipjpegTranscodeParams_t& p, int orientation, const uint8_t* data, size_t size, std::vector<uint8_t>* markers)
{
    markers->clear();
    if (!(p.orientation & HIPJPEG_TRANSCODE_COPY_MARKERS)) return;
    size_t exif_value = 0;
    bool little_endian = false;
    collect_marker_segments(data, size, markers, &exif_value, &little_endian);
    if (orientation != 1) reset_exif_orientation(markers, exif_value, little_endian);  // the file is upright now
}

hipjpegStatus_t transcode_turn(const TranscodePicture& src, int orientation, bool trim, TranscodePicture* dst, unsigned* turn)
{
    static const unsigned kTurns[9] = {0, 0, kTurnMirrorX, kTurnMirrorX | kTurnMirrorY, kTurnMirrorY, kTurnTranspose, kTurnTranspose | kTurnMirrorX,
                                       kTurnTranspose | kTurnMirrorX | kTurnMirrorY, kTurnTranspose | kTurnMirrorY};
    const unsigned t = kTurns[orientation];
    *turn = t;
    *dst = src;
    if (t == 0) return HIPJPEG_STATUS_SUCCESS;
    const EncodeGeometry& s = src.geom;
    const bool transpose = (t & kTurnTranspose) != 0;
    if (transpose && s.hs == 4) return HIPJPEG_STATUS_UNSUPPORTED;  // the writer has no 1x4 / 2x4
    // the output's mirrors in source terms: after a transpose the output's x axis is the source's y axis
    const bool mirror_sx = (t & (transpose ? kTurnMirrorY : kTurnMirrorX)) != 0, mirror_sy = (t & (transpose ? kTurnMirrorX : kTurnMirrorY)) != 0;
    int w = s.width, h = s.height;
    const int mcu_w = 8 * s.hs, mcu_h = 8 * s.vs;
    if (mirror_sx && w % mcu_w != 0) {
        if (!trim || w < mcu_w) return HIPJPEG_STATUS_UNSUPPORTED;
        w -= w % mcu_w;
    }
    if (mirror_sy && h % mcu_h != 0) {
        if (!trim || h < mcu_h) return HIPJPEG_STATUS_UNSUPPORTED;
        h -= h % mcu_h;
    }
    EncodeGeometry& g = dst->geom;
    g = EncodeGeometry();
    g.ncomp = s.ncomp;
    g.width = transpose ? h : w;
    g.height = transpose ? w : h;
    g.hs = transpose ? s.vs : s.hs;
    g.vs = transpose ? s.hs : s.vs;
    compute_geometry(&g);
    if (transpose)
        for (int j = 0; j < 64; j++) {
            const int tr = (j & 7) * 8 + (j >> 3);
            dst->qlum[j] = src.qlum[tr];
            dst->qchr[j] = src.qchr[tr];
        }
    return HIPJPEG_STATUS_SUCCESS;
}

EntropyEncodeOptions transcode_options(const hipjpegTranscodeParams_t& p)
{
    return EntropyEncodeOptions{p.restart_interval, p.optimized_huffman != 0, p.progressive != 0};
}

void natural_area(const FrameInfo& f, NaturalPlanes* p)
{
    *p = NaturalPlanes();
    for (int c = 0; c < f.ncomp; c++) {
        p->blocks_w[c] = (f.comp[c].samp_w + 7) / 8;
        p->blocks_h[c] = (f.comp[c].samp_h + 7) / 8;
    }
}

hipjpegStatus_t decode_natural(const uint8_t* data, size_t size, const FrameInfo& f, const NaturalPlanes& dst)
{
    // the decoder's blocks: column-major over the frame's MCU-padded grid
    std::vector<int16_t> src(f.total_blocks() * 64, 0);
    int16_t* sptr[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t off = 0;
    for (int c = 0; c < f.ncomp; c++) {
        sptr[c] = src.data() + off;
        off += (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64;
    }
    switch (decode_coefficients(data, size, f, sptr)) {
    case kEntropyOk: break;
    case kEntropyTruncated: return HIPJPEG_STATUS_TRUNCATED;
    case kEntropyMissingTable: return HIPJPEG_STATUS_BAD_JPEG;
    default: return HIPJPEG_STATUS_CORRUPT;
    }
    // nothing is written before the picture is known to be whole
    for (int c = 0; c < f.ncomp; c++)
        for (int by = 0; by < dst.blocks_h[c]; by++)
            for (int bx = 0; bx < dst.blocks_w[c]; bx++) {
                const int16_t* s = sptr[c] + ((size_t)by * f.comp[c].blocks_w + bx) * 64;
                int16_t* d = dst.coef[c] + ((size_t)by * dst.pitch[c] + bx) * 64;
                for (int j = 0; j < 64; j++) d[j] = s[(j & 7) * 8 + (j >> 3)];
            }
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t encode_natural(const TranscodePicture& pic, const NaturalPlanes& src, const TranscodeOrigin& origin, unsigned turn,
                               const EntropyEncodeOptions& opt, std::vector<uint8_t>* out)
{
    // the coder's blocks: zigzag order over its own grid; only the real area is read
    const EncodeGeometry& g = pic.geom;
    std::vector<int16_t> dst;
    size_t doff[3] = {0, 0, 0}, total = 0;
    for (int c = 0; c < g.ncomp; c++) {
        doff[c] = total;
        total += (size_t)g.blocks_w[c] * g.blocks_h[c] * 64;
    }
    dst.assign(total, 0);
    // zigzag index -> position in the source's block (row * 8 + column) -- read the other way round, the block comes out transposed --
    // and whether a mirror of the output negates it (odd u: mirror x, odd v: mirror y; both: twice)
    const bool transpose = (turn & kTurnTranspose) != 0;
    int from[64];
    bool negate[64];
    for (int k = 0; k < 64; k++) {
        const int u = kZigzagNatural[k] & 7, v = kZigzagNatural[k] >> 3;
        from[k] = transpose ? u * 8 + v : v * 8 + u;
        negate[k] = (((turn & kTurnMirrorX) != 0) & (u & 1)) ^ (((turn & kTurnMirrorY) != 0) & (v & 1));
    }
    for (int c = 0; c < g.ncomp; c++)
        for (int by = 0; by < g.real_h[c]; by++)
            for (int bx = 0; bx < g.real_w[c]; bx++) {
                // the source block: undo the output's mirrors over its real area, then the transpose, then the crop
                const int ty = (turn & kTurnMirrorY) ? g.real_h[c] - 1 - by : by, tx = (turn & kTurnMirrorX) ? g.real_w[c] - 1 - bx : bx;
                const int sy = origin.oy[c] + (transpose ? tx : ty), sx = origin.ox[c] + (transpose ? ty : tx);
                if (sy >= src.blocks_h[c] || sx >= src.blocks_w[c]) return HIPJPEG_STATUS_INTERNAL_ERROR;  // (the planning keeps every block inside)
                const int16_t* s = src.coef[c] + ((size_t)sy * src.pitch[c] + sx) * 64;
                int16_t* d = dst.data() + doff[c] + ((size_t)by * g.blocks_w[c] + bx) * 64;
                if (s[0] < kTranscodeDcMin || s[0] > kTranscodeDcMax) return HIPJPEG_STATUS_UNSUPPORTED;
                d[0] = s[0];
                for (int k = 1; k < 64; k++) {
                    const int v = s[from[k]];
                    if (v < -kTranscodeAcMax || v > kTranscodeAcMax) return HIPJPEG_STATUS_UNSUPPORTED;
                    d[k] = (int16_t)(negate[k] ? -v : v);
                }
            }
    const int16_t* coef[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < g.ncomp; c++) coef[c] = dst.data() + doff[c];
    encode_jfif(g, pic.qlum, pic.qchr, coef, opt, out);
    return HIPJPEG_STATUS_SUCCESS;
}

hipjpegStatus_t transcode_host(const uint8_t* data, size_t size, const hipjpegTranscodeParams_t& params, const hipjpegTranscodeRegion_t* region,
                               std::vector<uint8_t>* out)
{
    hipjpegStatus_t st = transcode_params_ok(params);
    if (st != HIPJPEG_STATUS_SUCCESS) return st;
    FrameInfo f;
    const ParseStatus ps = parse_jpeg(data, size, &f);
    if (ps != kParseOk) return ps == kParseUnsupported ? HIPJPEG_STATUS_UNSUPPORTED : ps == kParseTruncated ? HIPJPEG_STATUS_TRUNCATED : HIPJPEG_STATUS_BAD_JPEG;
    // drop chroma -> crop -> turn
    TranscodePicture source, cropped, pic;
    TranscodeOrigin origin;
    unsigned turn = 0;
    const int orientation = transcode_orientation(params, data, size);
    if ((st = transcode_picture(f, (params.orientation & HIPJPEG_TRANSCODE_GRAYSCALE) != 0, &source)) != HIPJPEG_STATUS_SUCCESS) return st;
    if ((st = transcode_crop(source, region, (params.orientation & HIPJPEG_TRANSCODE_CROP_EXPAND) != 0, &cropped, &origin)) != HIPJPEG_STATUS_SUCCESS)
        return st;
    if ((st = transcode_turn(cropped, orientation, (params.orientation & HIPJPEG_TRANSCODE_TRIM) != 0, &pic, &turn)) != HIPJPEG_STATUS_SUCCESS) return st;
    // the source's blocks in the public layout (natural order over the real area), then from there into the coder's: the two halves
    // hipjpegDecodeCoefficientsHost and hipjpegEncodeCoefficientsHost are made of
    NaturalPlanes planes;
    std::vector<int16_t> store;
    natural_area(f, &planes);
    size_t off = 0;
    for (int c = 0; c < f.ncomp; c++) off += (size_t)planes.blocks_w[c] * planes.blocks_h[c] * 64;
    store.assign(off, 0);
    off = 0;
    for (int c = 0; c < f.ncomp; c++) {
        planes.coef[c] = store.data() + off;
        planes.pitch[c] = (uint32_t)planes.blocks_w[c];
        off += (size_t)planes.blocks_w[c] * planes.blocks_h[c] * 64;
    }
    if ((st = decode_natural(data, size, f, planes)) != HIPJPEG_STATUS_SUCCESS) return st;
    std::vector<uint8_t> markers;
    transcode_markers(params, orientation, data, size, &markers);
    EntropyEncodeOptions opt = transcode_options(params);
    if (!markers.empty()) opt.markers = &markers;
    return encode_natural(pic, planes, origin, turn, opt, out);
}

}  // namespace hipjpeg

// The host route's C entry point lives here, not in hipjpeg_api.cpp, so that it links without the HIP runtime (tests/sanitizers).
extern "C" hipjpegStatus_t hipjpegTranscodeHostRegion(const uint8_t* data, size_t length, const hipjpegTranscodeParams_t* params,
                                                      const hipjpegTranscodeRegion_t* region, uint8_t* out, size_t capacity, size_t* out_length)
{
    try {  // no C++ exception crosses the C boundary
        if (!data || !params || !out_length) return HIPJPEG_STATUS_INVALID_ARGUMENT;
        std::vector<uint8_t> bytes;
        const hipjpegStatus_t st = hipjpeg::transcode_host(data, length, *params, region, &bytes);
        if (st != HIPJPEG_STATUS_SUCCESS) return st;
        *out_length = bytes.size();
        if (!out || capacity < bytes.size()) return HIPJPEG_STATUS_BUFFER_TOO_SMALL;
        memcpy(out, bytes.data(), bytes.size());
        return HIPJPEG_STATUS_SUCCESS;
    } catch (const std::bad_alloc&) {
        return HIPJPEG_STATUS_ALLOC_FAILED;
    } catch (...) {
        return HIPJPEG_STATUS_INTERNAL_ERROR;
    }
}

extern "C" hipjpegStatus_t hipjpegTranscodeHost(const uint8_t* data, size_t length, const hipjpegTranscodeParams_t* params, uint8_t* out,
                                                size_t capacity, size_t* out_length)
{
    return hipjpegTranscodeHostRegion(data, length, params, nullptr, out, capacity, out_length);
}

extern "C" hipjpegStatus_t hipjpegGetExifOrientation(const uint8_t* data, size_t length, int32_t* orientation)
{
    if (!data || !orientation) return HIPJPEG_STATUS_INVALID_ARGUMENT;
    *orientation = hipjpeg::exif_orientation(data, length);
    return HIPJPEG_STATUS_SUCCESS;
}
