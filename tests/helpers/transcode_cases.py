"""What the lossless-transcode tests share: the targets, the goldens, and the eligibility rules of include/hipjpeg.h computed
WITHOUT the calls under test -- from the header (lowlevel.get_image_info) and from the oracle's coefficients and tables."""
import glob
import os

import numpy as np

import oracle
from conftest import GOLDEN
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

# name -> keyword arguments of transcode_host / BatchTranscoder.transcode
TARGETS = {
    "annexk": dict(),
    "optimized": dict(optimized_huffman=True),
    "progressive": dict(progressive=True),
    "annexk_rst3": dict(restart_interval=3),
}

LUMA_FACTORS = {(1, 1), (2, 1), (2, 2), (1, 2), (4, 1), (4, 2)}
SUCCESS, UNSUPPORTED, TRUNCATED, BUFFER_TOO_SMALL = 0, 3, 4, 9


def golden_files(directory):
    """[(name, bytes)] of tests/golden/<directory>/*.jpg, sorted"""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, directory, "*.jpg"))):
        with open(path, "rb") as f:
            out.append((os.path.basename(path)[:-4], f.read()))
    return out


def frame_eligible(data):
    """Frame type, components and colour model, sampling factors."""
    try:
        info = lowlevel.get_image_info(data)
    except N.HipJpegError:
        return False
    if info["sof_marker"] not in (0xC0, 0xC1, 0xC2):
        return False
    if info["num_components"] == 1:
        return True
    if info["num_components"] != 3 or info["color_model"] != 1:
        return False
    if any((info["h"][c], info["v"][c]) != (1, 1) for c in (1, 2)):
        return False
    return (info["h"][0], info["v"][0]) in LUMA_FACTORS


def real_area(data):
    """per component (rows, columns) of blocks that carry samples"""
    info = lowlevel.get_image_info(data)
    return [((info["samp_h"][c] + 7) // 8, (info["samp_w"][c] + 7) // 8) for c in range(info["num_components"])]


def tables_eligible(qts):
    if any(int(q.max()) > 255 for q in qts):
        return False
    return len(qts) == 1 or np.array_equal(qts[1], qts[2])


def range_eligible(data, coefs):
    """jchuff.c's limits for 8-bit data over the blocks a transcode carries over: DC in [-1024, 1023], AC in [-1023, 1023]"""
    for c, (rh, rw) in zip(coefs, real_area(data)):
        blk = c[:rh, :rw].astype(np.int32)
        dc, ac = blk[:, :, 0], blk[:, :, 1:]
        if dc.min() < -1024 or dc.max() > 1023 or ac.min() < -1023 or ac.max() > 1023:
            return False
    return True


def header_eligible(data):
    """The rules a look at the header settles: the frame's and the quantization tables'."""
    return frame_eligible(data) and tables_eligible(oracle.decode_coefficients(data)[1])


def expected_eligible(data):
    """-> (header rules hold, header and range rules hold)"""
    if not header_eligible(data):
        return False, False
    return True, range_eligible(data, oracle.decode_coefficients(data)[0])


def same_picture(source, out):
    """The transcoded file holds the source's coefficients (over the real block area) and tables."""
    c1, q1 = oracle.decode_coefficients(source)
    c2, q2 = oracle.decode_coefficients(out)
    assert len(c1) == len(c2)
    for a, b, (rh, rw), qa, qb in zip(c1, c2, real_area(source), q1, q2):
        assert np.array_equal(a[:rh, :rw], b[:rh, :rw]) and np.array_equal(qa, qb)
