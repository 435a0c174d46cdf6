// plane_color_kernels.hip -- the gfx950 kernels of the decode device stage that take no coefficient block: every component sits in its
// plane already (K1 or the reduced IDCTs of decode_kernels.hip have written it) and these bring the planes to the caller's output, or
// one output to another.
//   generic_color_kernel (K3)  sampling layouts K2 does not cover: replication, YCbCr / RGB, one thread per pixel
//   cmyk_color_kernel          four-component frames: libjpeg's upsampling, YCCK -> CMYK, the reference's CMYK -> RGB step
//   scaled_color_kernel        scaled decode: libjpeg's upsampling on the scaled groups, sixteen or four pixels per lane
//   transform_kernel           geometry pass: region of interest + EXIF orientation
// The sample function (plane_sample) and the scalar colour step (ycc_to_rgb) exist once, for all of them.  Arithmetic is that of
// libjpeg-turbo's jdsample.c / jdcolor.c, restated; results are compared bit-for-bit with the CPU oracle and with vectors from the
// library itself in tests/.
#include <hip/hip_runtime.h>

#include "decode_kernel_common.h"

namespace hipjpeg {

namespace {

// jdcolor.c ycc_rgb_convert with SCALEBITS = 16, one pixel in plain integers (K2 does the same on int16 pairs)
__device__ __forceinline__ void ycc_to_rgb(int y, int cb, int cr, int& R, int& G, int& B)
{
    const int rr = (cr * 91881 + (32768 - 128 * 91881)) >> 16;
    const int bb = (cb * 116130 + (32768 - 128 * 116130)) >> 16;
    const int gg = (cb * -22554 + cr * -46802 + (32768 + 128 * 22554 + 128 * 46802)) >> 16;
    R = min(max(y + rr, 0), 255);
    G = min(max(y + gg, 0), 255);
    B = min(max(y + bb, 0), 255);
}

// The three channels of pixel (x, y) to the output: swapped for BGR, a byte into each plane or three interleaved bytes
__device__ __forceinline__ void store_pixel(const DecodeImage& im, int x, int y, bool planar, bool bgr, int R, int G, int B)
{
    if (bgr) {
        const int t = R;
        R = B;
        B = t;
    }
    if (planar) {
        im.out[0][(size_t)y * im.out_pitch[0] + x] = (uint8_t)R;
        im.out[1][(size_t)y * im.out_pitch[1] + x] = (uint8_t)G;
        im.out[2][(size_t)y * im.out_pitch[2] + x] = (uint8_t)B;
    } else {
        uint8_t* p = im.out[0] + (size_t)y * im.out_pitch[0] + (size_t)x * 3;
        p[0] = (uint8_t)R;
        p[1] = (uint8_t)G;
        p[2] = (uint8_t)B;
    }
}

// ------------------------------------------------------------------------------------------------
// K3: generic colour stage for layouts the fused kernel does not cover (4:1:1, 4:1:0, ...): every component is in a
// plane already; libjpeg upsamples those by plain replication (jdsample.c int_upsample).  One thread = one pixel.
// The unit table is reused: block_base = pixel row, comp unused.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void generic_color_kernel(const DecodeImage* __restrict__ images, const WorkUnit* __restrict__ units)
{
    const WorkUnit u = units[blockIdx.x];
    const DecodeImage& im = images[u.image];
    const int W = im.width, H = im.height;
    const int y = u.block_base;
    if (y >= H) return;
    const int fmt = im.out_format;
    const bool planar = fmt == kOutPlanarRGB || fmt == kOutPlanarBGR;
    const bool bgr = fmt == kOutInterleavedBGR || fmt == kOutPlanarBGR;
    // Only three-component images take this path (gray goes through luma_color_kernel<0,0>), so the component
    // index is a compile-time constant everywhere below.
    const int hmax = im.hmax, vmax = im.vmax;
    const uint8_t* row0 = im.comp[0].plane + (size_t)(y * im.comp[0].v / vmax) * im.comp[0].plane_pitch;
    const uint8_t* row1 = im.comp[1].plane + (size_t)(y * im.comp[1].v / vmax) * im.comp[1].plane_pitch;
    const uint8_t* row2 = im.comp[2].plane + (size_t)(y * im.comp[2].v / vmax) * im.comp[2].plane_pitch;
    const int h0 = im.comp[0].h, h1 = im.comp[1].h, h2 = im.comp[2].h;
    for (int x = threadIdx.x; x < W; x += kThreads) {
        // (x * h / hmax, not plane_sample's x / (hmax / h): the two differ where hmax / h is no whole number, and
        //  tests/test_gpu_sampling_layouts.py pins such layouts)
        int s[3];
        s[0] = row0[x * h0 / hmax];
        s[1] = row1[x * h1 / hmax];
        s[2] = row2[x * h2 / hmax];
        int R, G, B;
        if (im.color_model == 1) {
            ycc_to_rgb(s[0], s[1], s[2], R, G, B);
        } else {
            R = s[0];
            G = s[1];
            B = s[2];
        }
        store_pixel(im, x, y, planar, bgr, R, G, B);
    }
}

// ------------------------------------------------------------------------------------------------
// One component's plane as the sample function below sees it: fx, fy = how many output pixels one of its samples covers.
//   full-size frames (CMYK / YCCK)   fx = hmax / h, fy = vmax / v
//   scaled decode                    jdsample.c jinit_upsampler on the scaled groups: a component of DCT_scaled_size s has h_in = h s / k
//                                    samples per group against h_out = hmax, so fx = hmax k / (h s), fy = vmax k / (v s)
// ------------------------------------------------------------------------------------------------
struct SamplePlane {
    const uint8_t* plane;
    unsigned pitch;
    int dw, dh, fx, fy;
};
// (the component index is a compile-time constant: a run-time one would reach the descriptor through a scalar load with a register offset)
template <int C>
__device__ __forceinline__ SamplePlane full_size_plane(const DecodeImage& im)
{
    const DecodeComponent& k = im.comp[C];
    return SamplePlane{k.plane, k.plane_pitch, (int)k.samp_w, (int)k.samp_h, (int)im.hmax / (int)k.h, (int)im.vmax / (int)k.v};
}
template <int C>
__device__ __forceinline__ SamplePlane scaled_plane(const DecodeImage& im)
{
    const DecodeComponent& k = im.comp[C];
    // (a gray image's unused components are zeros: max keeps the divisions defined)
    return SamplePlane{k.plane, k.plane_pitch, (int)k.samp_w, (int)k.samp_h, (int)(im.hmax * im.scale_k) / max((int)(k.h * k.scaled), 1),
                       (int)(im.vmax * im.scale_k) / max((int)(k.v * k.scaled), 1)};
}

// The sample of output pixel (x, y) the way libjpeg-turbo brings a component to full size (jdsample.c): h2v1 / h2v2 / h1v2 triangle
// filters when fancy upsampling is on and they apply (h2v1 and h2v2 only on planes more than two samples wide), else replication.
// (For a scaled decode the host has cleared kFlagFancyUpsampling where k = 1: libjpeg does no fancy upsampling there.)
__device__ __forceinline__ int plane_sample(const SamplePlane& k, int x, int y, bool fancy)
{
    const int fx = k.fx, fy = k.fy, dw = k.dw, dh = k.dh;
    const uint8_t* plane = k.plane;
    const size_t pitch = k.pitch;
    if (fx == 1 && fy == 1) return plane[(size_t)y * pitch + x];
    if (fx == 2 && fy == 1 && fancy && dw > 2) {
        const uint8_t* p = plane + (size_t)y * pitch;
        const int i = x >> 1;
        if (x == 0) return p[0];
        if (x == 2 * dw - 1) return p[dw - 1];
        return (x & 1) ? (3 * p[i] + p[i + 1] + 2) >> 2 : (3 * p[i] + p[i - 1] + 1) >> 2;
    }
    if (fx == 2 && fy == 2 && fancy && dw > 2) {
        const int r0 = y >> 1, r1 = min(max((y & 1) ? r0 + 1 : r0 - 1, 0), dh - 1);
        const uint8_t* p0 = plane + (size_t)r0 * pitch;
        const uint8_t* p1 = plane + (size_t)r1 * pitch;
        const int i = x >> 1, cs = 3 * p0[i] + p1[i];
        if (x == 0) return (cs * 4 + 8) >> 4;
        if (x == 2 * dw - 1) return (cs * 4 + 7) >> 4;
        return (x & 1) ? (3 * cs + (3 * p0[i + 1] + p1[i + 1]) + 7) >> 4 : (3 * cs + (3 * p0[i - 1] + p1[i - 1]) + 8) >> 4;
    }
    if (fx == 1 && fy == 2 && fancy) {
        const int r0 = y >> 1, r1 = min(max((y & 1) ? r0 + 1 : r0 - 1, 0), dh - 1);
        return (3 * plane[(size_t)r0 * pitch + x] + plane[(size_t)r1 * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    return plane[(size_t)(y / fy) * pitch + x / fx];
}

// ------------------------------------------------------------------------------------------------
// Four-component frames (CMYK, YCCK): every component sits in its plane; the kernel brings each to full size (plane_sample),
// turns a YCCK frame into CMYK (jdcolor.c ycck_cmyk_convert) and then applies the reference extension's own
// CMYK -> RGB step (extensions/libjpeg_turbo/jpeg_mem.cpp:292-337): with an Adobe marker r = k*c/255, without one
// r = (255-k)*(255-c)/255; P_Y = (uint8)(0.299f r + 0.587f g + 0.114f b).  One thread = one pixel; rare path.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cmyk_color_kernel(const DecodeImage* __restrict__ images, const WorkUnit* __restrict__ units)
{
    const WorkUnit u = units[blockIdx.x];
    const DecodeImage& im = images[u.image];
    const int W = im.width, H = im.height;
    const int y = u.block_base;
    if (y >= H) return;
    const int fmt = im.out_format;
    const bool planar = fmt == kOutPlanarRGB || fmt == kOutPlanarBGR;
    const bool bgr = fmt == kOutInterleavedBGR || fmt == kOutPlanarBGR;
    const bool fancy = (im.flags & kFlagFancyUpsampling) != 0, adobe = (im.flags & kFlagAdobeMarker) != 0;
    const bool ycck = im.color_model == 4;
    const SamplePlane k0 = full_size_plane<0>(im), k1 = full_size_plane<1>(im), k2 = full_size_plane<2>(im), k3 = full_size_plane<3>(im);
    for (int x = threadIdx.x; x < W; x += kThreads) {
        int c = plane_sample(k0, x, y, fancy), m = plane_sample(k1, x, y, fancy), ye = plane_sample(k2, x, y, fancy);
        const int k = plane_sample(k3, x, y, fancy);
        if (ycck) {
            int r, g, b;
            ycc_to_rgb(c, m, ye, r, g, b);
            c = 255 - r;
            m = 255 - g;
            ye = 255 - b;
        }
        int R, G, B;
        if (adobe) {
            R = (k * c) / 255;
            G = (k * m) / 255;
            B = (k * ye) / 255;
        } else {
            R = (255 - k) * (255 - c) / 255;
            G = (255 - k) * (255 - m) / 255;
            B = (255 - k) * (255 - ye) / 255;
        }
        if (fmt == kOutY) {
            // three products and two sums, each rounded to float on its own, as the reference's x86 build computes them
            // (a fused multiply-add would round differently)
            float yf;
            {
#pragma clang fp contract(off)
                const float pr = 0.299f * (float)R, pg = 0.587f * (float)G, pb = 0.114f * (float)B;
                yf = (pr + pg) + pb;
            }
            im.out[0][(size_t)y * im.out_pitch[0] + x] = (uint8_t)yf;
            continue;
        }
        store_pixel(im, x, y, planar, bgr, R, G, B);
    }
}

// ------------------------------------------------------------------------------------------------
// Scaled decode (hipjpegDecodeBatchSetScales: 1/2, 1/4, 1/8 -- libjpeg's scale_num / scale_denom): from the planes of a scaled image
// (K1 and idct_reduced_plane_kernel of decode_kernels.hip) to its output.
// ------------------------------------------------------------------------------------------------
// Three samples of one pixel -> its three output channels in store order
__device__ __forceinline__ void scaled_pixel(int s0, int s1, int s2, bool gray, bool ycc, bool bgr, int& a, int& b, int& c)
{
    int R = s0, G = s0, B = s0;
    if (!gray) {
        if (ycc) {
            ycc_to_rgb(s0, s1, s2, R, G, B);
        } else {
            G = s1;
            B = s2;
        }
    }
    a = bgr ? B : R;
    b = G;
    c = bgr ? R : B;
}

// four bytes to dst: one dword where the row is 4-byte aligned and all four belong to the picture, single bytes at a ragged edge
__device__ __forceinline__ void store_px4(uint8_t* dst, unsigned v, bool whole)
{
    if (whole)
        *reinterpret_cast<unsigned*>(dst) = v;
    else
        dst[0] = (uint8_t)v;  // (the caller has shifted the byte it wants into place)
}

// One workgroup = kScaledRowsPerUnit pixel rows, a wave per row in turn.  Where no component is left to upsample (gray, 4:4:4 and 4:2:0
// at every scale: libjpeg gives the chroma the larger IDCT instead) and the caller's rows are 16-byte aligned, a lane takes SIXTEEN
// pixels: one 16-byte load per plane, three 16-byte stores (interleaved) or one per plane -- the kernel is bound by the bytes it has in
// flight, not by arithmetic.  What is left of the row, and every other picture, goes in groups of FOUR pixels: a dword load per plane or
// plane_sample() per pixel, dword stores where the rows are 4-byte aligned, single bytes at a ragged edge.  Everything that picks a
// path -- format, colour model, filter, alignment -- is the same for the whole workgroup.
__global__ __launch_bounds__(kThreads) void scaled_color_kernel(const DecodeImage* __restrict__ images, const WorkUnit* __restrict__ units)
{
    const WorkUnit u = units[blockIdx.x];
    const DecodeImage& im = images[u.image];
    const int W = im.width, H = im.height;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fmt = im.out_format;
    const bool planar = fmt == kOutPlanarRGB || fmt == kOutPlanarBGR, only_y = fmt == kOutY;
    const bool bgr = fmt == kOutInterleavedBGR || fmt == kOutPlanarBGR;
    const bool fancy = (im.flags & kFlagFancyUpsampling) != 0;
    const bool gray = im.ncomp == 1 || only_y, ycc = im.color_model == 1;
    const SamplePlane k0 = scaled_plane<0>(im), k1 = scaled_plane<1>(im), k2 = scaled_plane<2>(im);
    const bool direct = k0.fx == 1 && k0.fy == 1 && (gray || (k1.fx == 1 && k1.fy == 1 && k2.fx == 1 && k2.fy == 1));
    uint8_t* const out0 = im.out[0];
    uint8_t* const out1 = im.out[1];
    uint8_t* const out2 = im.out[2];
    const unsigned op0 = im.out_pitch[0], op1 = im.out_pitch[1], op2 = im.out_pitch[2];
    const bool aligned = planar ? ((((uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)out2 | op0 | op1 | op2) & 3) == 0) : ((((uintptr_t)out0 | op0) & 3) == 0);
    const bool aligned16 = planar ? ((((uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)out2 | op0 | op1 | op2) & 15) == 0) : ((((uintptr_t)out0 | op0) & 15) == 0);
    const int wide_groups = (direct && aligned16) ? (W >> 4) : 0;
    const int groups = (W + 3) >> 2, row_end = min((int)u.block_base + kScaledRowsPerUnit, H);
    for (int y = (int)u.block_base + wave; y < row_end; y += kThreads / 64) {
        for (int g = lane; g < wide_groups; g += 64) {
            const int x = g * 16;
            // (planes are 16-byte aligned, pitch included, and x + 16 <= W lies inside the row)
            const u32x4 v0 = *reinterpret_cast<const u32x4*>(k0.plane + (size_t)y * k0.pitch + x);
            if (only_y) {
                *reinterpret_cast<u32x4*>(out0 + (size_t)y * op0 + x) = v0;
                continue;
            }
            u32x4 v1 = {0u, 0u, 0u, 0u}, v2 = {0u, 0u, 0u, 0u};
            if (!gray) {
                v1 = *reinterpret_cast<const u32x4*>(k1.plane + (size_t)y * k1.pitch + x);
                v2 = *reinterpret_cast<const u32x4*>(k2.plane + (size_t)y * k2.pitch + x);
            }
            const unsigned w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w}, w2[4] = {v2.x, v2.y, v2.z, v2.w};
            unsigned o[12];  // interleaved: the 48 bytes in order; planar: [0..3] first plane, [4..7] second, [8..11] third
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int a[4], b[4], c[4];
#pragma unroll
                for (int i = 0; i < 4; i++)
                    scaled_pixel((int)((w0[q] >> (8 * i)) & 255u), (int)((w1[q] >> (8 * i)) & 255u), (int)((w2[q] >> (8 * i)) & 255u), gray, ycc, bgr, a[i], b[i], c[i]);
                if (planar) {
                    o[q] = pack4(a[0], a[1], a[2], a[3]);
                    o[4 + q] = pack4(b[0], b[1], b[2], b[3]);
                    o[8 + q] = pack4(c[0], c[1], c[2], c[3]);
                } else {
                    o[3 * q] = pack4(a[0], b[0], c[0], a[1]);
                    o[3 * q + 1] = pack4(b[1], c[1], a[2], b[2]);
                    o[3 * q + 2] = pack4(c[2], a[3], b[3], c[3]);
                }
            }
            const u32x4 s0 = {o[0], o[1], o[2], o[3]}, s1 = {o[4], o[5], o[6], o[7]}, s2 = {o[8], o[9], o[10], o[11]};
            if (planar) {
                *reinterpret_cast<u32x4*>(out0 + (size_t)y * op0 + x) = s0;
                *reinterpret_cast<u32x4*>(out1 + (size_t)y * op1 + x) = s1;
                *reinterpret_cast<u32x4*>(out2 + (size_t)y * op2 + x) = s2;
            } else {
                u32x4* q = reinterpret_cast<u32x4*>(out0 + (size_t)y * op0 + (size_t)x * 3);  // (x * 3 is a multiple of 48)
                q[0] = s0;
                q[1] = s1;
                q[2] = s2;
            }
        }
        for (int g = wide_groups * 4 + lane; g < groups; g += 64) {
            const int x = g * 4, n = min(4, W - x);
            int s0[4], s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
            if (direct) {
                // (planes are 16-byte aligned with 16 bytes of slack per row: an aligned dword that starts inside the row is in bounds)
                const unsigned v0 = *reinterpret_cast<const unsigned*>(k0.plane + (size_t)y * k0.pitch + x);
                unsigned v1 = 0, v2 = 0;
                if (!gray) {
                    v1 = *reinterpret_cast<const unsigned*>(k1.plane + (size_t)y * k1.pitch + x);
                    v2 = *reinterpret_cast<const unsigned*>(k2.plane + (size_t)y * k2.pitch + x);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    s0[i] = (int)((v0 >> (8 * i)) & 255u);
                    s1[i] = (int)((v1 >> (8 * i)) & 255u);
                    s2[i] = (int)((v2 >> (8 * i)) & 255u);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int xi = min(x + i, W - 1);  // (past the right edge: a pixel that exists, its value is not stored)
                    s0[i] = plane_sample(k0, xi, y, fancy);
                    if (!gray) {
                        s1[i] = plane_sample(k1, xi, y, fancy);
                        s2[i] = plane_sample(k2, xi, y, fancy);
                    }
                }
            }
            const bool whole = aligned && n == 4;
            if (only_y) {
                uint8_t* d = out0 + (size_t)y * op0 + x;
                const unsigned v = pack4(s0[0], s0[1], s0[2], s0[3]);
                store_px4(d, v, whole);
#pragma unroll
                for (int i = 1; i < 4; i++)
                    if (!whole && i < n) d[i] = (uint8_t)(v >> (8 * i));
                continue;
            }
            int a[4], b[4], c[4];
#pragma unroll
            for (int i = 0; i < 4; i++) scaled_pixel(s0[i], s1[i], s2[i], gray, ycc, bgr, a[i], b[i], c[i]);
            if (planar) {
                uint8_t* d0 = out0 + (size_t)y * op0 + x;
                uint8_t* d1 = out1 + (size_t)y * op1 + x;
                uint8_t* d2 = out2 + (size_t)y * op2 + x;
                const unsigned va = pack4(a[0], a[1], a[2], a[3]), vb = pack4(b[0], b[1], b[2], b[3]), vc = pack4(c[0], c[1], c[2], c[3]);
                store_px4(d0, va, whole);
                store_px4(d1, vb, whole);
                store_px4(d2, vc, whole);
#pragma unroll
                for (int i = 1; i < 4; i++)
                    if (!whole && i < n) {
                        d0[i] = (uint8_t)(va >> (8 * i));
                        d1[i] = (uint8_t)(vb >> (8 * i));
                        d2[i] = (uint8_t)(vc >> (8 * i));
                    }
            } else {
                uint8_t* d = out0 + (size_t)y * op0 + (size_t)x * 3;
                if (whole) {
                    unsigned* q = reinterpret_cast<unsigned*>(d);  // (x * 3 is a multiple of 12)
                    q[0] = pack4(a[0], b[0], c[0], a[1]);
                    q[1] = pack4(b[1], c[1], a[2], b[2]);
                    q[2] = pack4(c[2], a[3], b[3], c[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (i < n) {
                            d[3 * i] = (uint8_t)a[i];
                            d[3 * i + 1] = (uint8_t)b[i];
                            d[3 * i + 2] = (uint8_t)c[i];
                        }
                }
            }
        }
    }
}

// Geometry pass: region of interest + EXIF orientation (DecodeBatch plans it for the images that ask for it; the pixel
// kernels have written those images into an intermediate buffer in stored-image coordinates).
// Upright pixel (ox, oy) comes from region pixel (u, v):
//   1: (ox, oy)            2: (rw-1-ox, oy)        3: (rw-1-ox, rh-1-oy)   4: (ox, rh-1-oy)
//   5: (oy, ox)            6: (oy, rh-1-ox)        7: (rw-1-oy, rh-1-ox)   8: (rw-1-oy, ox)
// (EXIF 2.32 orientation tag; 5 = transpose, 6 = stored picture must be turned 90 degrees clockwise, 7 = transverse,
//  8 = 270 degrees clockwise).  One workgroup = kTransformRowsPerUnit output rows; lanes walk along output rows, so the
// writes are coalesced whatever the reads look like.
__global__ __launch_bounds__(kThreads) void transform_kernel(const TransformImage* __restrict__ images, const WorkUnit* __restrict__ units)
{
    const WorkUnit wu = units[blockIdx.x];
    const TransformImage& t = images[wu.image];
    const int rw = t.rw, rh = t.rh, ow = t.out_w, o = t.orientation;
    const int row_end = min((int)wu.block_base + kTransformRowsPerUnit, t.out_h);
    for (int oy = (int)wu.block_base; oy < row_end; oy++) {
        for (int ox = threadIdx.x; ox < ow; ox += kThreads) {
            int u, v;
            switch (o) {
            case 2: u = rw - 1 - ox; v = oy; break;
            case 3: u = rw - 1 - ox; v = rh - 1 - oy; break;
            case 4: u = ox; v = rh - 1 - oy; break;
            case 5: u = oy; v = ox; break;
            case 6: u = oy; v = rh - 1 - ox; break;
            case 7: u = rw - 1 - oy; v = rh - 1 - ox; break;
            case 8: u = rw - 1 - oy; v = ox; break;
            default: u = ox; v = oy; break;
            }
            const int sx = t.x0 + u, sy = t.y0 + v;
            if (t.bpp == 3) {
                const uint8_t* s = t.src[0] + (size_t)sy * t.src_pitch[0] + (size_t)sx * 3;
                uint8_t* d = t.dst[0] + (size_t)oy * t.dst_pitch[0] + (size_t)ox * 3;
                d[0] = s[0];
                d[1] = s[1];
                d[2] = s[2];
            } else {
                for (int p = 0; p < t.nplanes; p++)
                    t.dst[p][(size_t)oy * t.dst_pitch[p] + ox] = t.src[p][(size_t)sy * t.src_pitch[p] + sx];
            }
        }
    }
}

}  // namespace

int launch_generic_color(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(generic_color_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units);
    return (int)hipGetLastError();
}

int launch_cmyk_color(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(cmyk_color_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units);
    return (int)hipGetLastError();
}

int launch_scaled_color(const DecodeImage* images, const WorkUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(scaled_color_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units);
    return (int)hipGetLastError();
}

int launch_transform(const TransformImage* images, const WorkUnit* units, int nunits, void* stream)
{
    if (nunits <= 0) return 0;
    hipLaunchKernelGGL(transform_kernel, dim3(nunits), dim3(kThreads), 0, (hipStream_t)stream, images, units);
    return (int)hipGetLastError();
}

}  // namespace hipjpeg
