"""hipjpegGetEncodeCoefficientInfo (lowlevel.encode_coefficient_info), no GPU: the `info` of the file the encoder writes for a size, a
subsampling and a quality -- what a caller allocates from before hipjpegPixelsToCoefficientsBatch -- equals, in every field and every
table, what hipjpegGetCoefficientInfo reads from the file the oracle (libjpeg-turbo) writes for such a picture."""
import numpy as np
import pytest

import oracle
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

INVALID_ARGUMENT, UNSUPPORTED = 1, 3
SIZES = [(1, 1), (17, 13), (50, 37), (320, 200), (2056, 8)]
SUBSAMPLINGS = sorted(N.CSS)  # every subsampling subsampling_factors knows
QUALITIES = [1, 50, 90, 100]


def test_every_subsampling_is_listed():
    assert SUBSAMPLINGS == ["410", "411", "420", "422", "440", "444", "gray"]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_info_is_the_written_files(size):
    w, h = size
    pixels = synth_image(w, h)
    for sub in SUBSAMPLINGS:
        for q in QUALITIES:
            got = lowlevel.encode_coefficient_info(w, h, sub, q)
            want = lowlevel.coefficient_info(oracle.encode(pixels, sub, q))
            assert set(got) == set(want)
            for k in want:
                if k == "qtables":
                    assert len(got[k]) == len(want[k]) and all(np.array_equal(a, b) for a, b in zip(got[k], want[k])), (sub, q)
                else:
                    assert got[k] == want[k], (sub, q, k)


def test_only_quality_and_subsampling_are_read():
    import ctypes
    want = lowlevel.encode_coefficient_info(50, 37, "422", 75)
    p = N.EncodeParams(75, N.CSS["422"], N.OUTPUT_Y, 7, 1, 1)
    ci = N.CoefficientInfo()
    assert N.load().hipjpegGetEncodeCoefficientInfo(50, 37, ctypes.byref(p), ctypes.byref(ci)) == 0
    got = lowlevel._info_dict(ci)
    assert {k: v for k, v in got.items() if k != "qtables"} == {k: v for k, v in want.items() if k != "qtables"}
    assert all(np.array_equal(a, b) for a, b in zip(got["qtables"], want["qtables"]))


@pytest.mark.parametrize("args,status", [((5, 5, "no_such"), UNSUPPORTED), ((5, 5, 7), UNSUPPORTED), ((5, 5, -1), UNSUPPORTED),
                                         ((0, 5, "420"), INVALID_ARGUMENT), ((5, 0, "420"), INVALID_ARGUMENT),
                                         ((65536, 5, "420"), INVALID_ARGUMENT), ((5, 65536, "gray"), INVALID_ARGUMENT),
                                         ((0, 5, "no_such"), UNSUPPORTED)])
def test_refusals(args, status):
    with pytest.raises(N.HipJpegError) as e:
        lowlevel.encode_coefficient_info(*args)
    assert e.value.status == status


def test_null_arguments():
    import ctypes
    p, ci = N.EncodeParams(90, N.CSS["420"], N.OUTPUT_RGBI, 0, 0, 0), N.CoefficientInfo()
    assert N.load().hipjpegGetEncodeCoefficientInfo(8, 8, None, ctypes.byref(ci)) == INVALID_ARGUMENT
    assert N.load().hipjpegGetEncodeCoefficientInfo(8, 8, ctypes.byref(p), None) == INVALID_ARGUMENT
    assert N.load().hipjpegGetEncodeCoefficientInfo(65535, 65535, ctypes.byref(p), ctypes.byref(ci)) == 0
    assert list(ci.blocks_w)[:3] == [8192, 4096, 4096]
