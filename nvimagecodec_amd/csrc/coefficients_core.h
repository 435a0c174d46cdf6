// coefficients_core.h -- coefficient tensors (hipjpegGetCoefficientInfo, hipjpegGetEncodeCoefficientInfo, hipjpeg{Decode,Encode}Coefficients*,
// hipjpegCoefficientsToPixelsBatch, hipjpegPixelsToCoefficientsBatch): the argument and header
// rules of include/hipjpeg.h, shared by the host calls (coefficients_core.cpp, which links without the HIP runtime) and the batch calls
// (hipjpeg_api.cpp).  The layout itself and the two host routes through it are transcode_core.h's NaturalPlanes / decode_natural /
// encode_natural: hipjpegTranscodeHost is a read followed by a write.
#pragma once
#include "../../include/hipjpeg.h"
#include "jpeg_syntax.h"
#include "transcode_core.h"

namespace hipjpeg {

hipjpegStatus_t coefficient_parse_status(ParseStatus ps);
// Geometry, sampling factors, real block areas and tables of a parsed frame.
void coefficient_info(const FrameInfo& f, hipjpegCoefficientInfo_t* info);
// The planes of `ncomp` components against their real widths: INVALID_ARGUMENT for a null pointer, a pointer that is not 16-byte aligned,
// a pitch below blocks_w.
hipjpegStatus_t coefficient_planes_ok(int ncomp, const int32_t blocks_w[4], const hipjpegCoefficientPlanes_t& planes);
// Writing: everything the `info`, the planes' description and the parameters settle (the range rule is left to whoever reads the blocks).
// INVALID_ARGUMENT first (sizes, block areas, pitches, pointers, parameters), then transcode_picture's header rules (UNSUPPORTED);
// SUCCESS and the picture as the coder takes it.
hipjpegStatus_t coefficient_picture(const hipjpegCoefficientInfo_t& info, const hipjpegCoefficientPlanes_t& planes, const hipjpegTranscodeParams_t& params,
                                    TranscodePicture* pic);
// To pixels (hipjpegCoefficientsToPixelsBatch): the frame the `info` describes, as the parser would hand it to the decoder -- the
// inverse of coefficient_info(); no scans, no Huffman tables, no JFIF / Adobe segment.  INVALID_ARGUMENT: a size outside 1..65535, a
// component count outside 1..4, sampling factors outside 1..4, block areas that are not what the geometry gives, whatever
// coefficient_planes_ok() refuses.  UNSUPPORTED: four components (the CMYK -> RGB formula turns on the Adobe segment, which the `info`
// does not record), a colour model no frame of that many components has.  The quantizers are taken as given.
hipjpegStatus_t coefficient_frame(const hipjpegCoefficientInfo_t& info, const hipjpegCoefficientPlanes_t& planes, FrameInfo* f);
// From pixels (hipjpegGetEncodeCoefficientInfo): the `info` of the file the encoder writes for a geometry and its two quality-scaled
// tables (picture_setup()).
void encode_coefficient_info(const EncodeGeometry& g, const uint16_t qlum[64], const uint16_t qchr[64], hipjpegCoefficientInfo_t* info);

}  // namespace hipjpeg
