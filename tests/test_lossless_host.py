"""Lossless JPEG (SOF3) on the host: the parser's rules, the entropy stage, the plain reconstruction and the reconstruction kernels'
schedule run lane by lane, all against the goldens libjpeg-turbo produced (tests/golden/make_golden_lossless.py).  No GPU."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_files as LF
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import abi as A
from nvimagecodec_amd import lowlevel

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_lossless.json")))
CASES = MANIFEST["lossless"]
REFUSED = {r["name"]: r for r in MANIFEST["refused"]}


def golden(name):
    return open(os.path.join(GOLDEN, "lossless", name + ".jpg"), "rb").read()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except N.HipJpegError as e:
        return N.STATUS_NAMES[e.status]
    return "SUCCESS"


def test_the_golden_set_is_the_one_the_issue_asks_for():
    have = {(c["predictor"], c["precision"], c["point_transform"], c["components"]) for c in CASES}
    for ps in range(1, 8):
        for P in (2, 8, 12, 16):
            for pt in ((0, 1) if P == 2 else (0, 2)):
                for n in (1, 3):
                    assert (ps, P, pt, n) in have
    assert {c["components"] for c in CASES} == {1, 2, 3, 4}
    assert {c["restart_rows"] for c in CASES} >= {0, 1, 3}
    assert {c["precision"] for c in CASES if c["name"].startswith("range")} == {2, 8, 9, 12}
    assert any(c["name"].startswith("ssss16") for c in CASES) and any(c["stuffed"] for c in CASES)
    assert set(REFUSED) == {"refused_dri_not_rows", "refused_ps0", "refused_ps8", "refused_al_ge_p", "refused_symbol17"}
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "lossless", c["name"] + ".jpg")) == c["bytes"] < 64 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_info_and_host_decodes_equal_the_library(case):
    data = golden(case["name"])
    info = lowlevel.lossless_info(data)
    assert (info["width"], info["height"], info["num_components"], info["precision"], info["predictor"], info["point_transform"],
            info["restart_rows"]) == (case["width"], case["height"], case["components"], case["precision"], case["predictor"],
                                      case["point_transform"], case["restart_rows"])
    dtype = np.dtype(case["dtype"])
    assert sha(lowlevel.decode_lossless_host(data, dtype=dtype)) == case["sha256"]
    algorithms = (0, 2) + ((1,) if case["predictor"] == 1 else ())
    for algorithm in algorithms:
        assert sha(lowlevel.decode_lossless_host(data, dtype=dtype, algorithm=algorithm)) == case["sha256"], algorithm
    if dtype == np.uint8:
        # the same state, sixteen bits of it
        wide = lowlevel.decode_lossless_host(data, dtype=np.uint16)
        assert sha((wide & 0xFF).astype(np.uint8)) == case["sha256"]
    planar = lowlevel.decode_lossless_host(data, dtype=dtype, planar=True, algorithm=0)
    assert sha(np.moveaxis(planar, 0, 2)) == case["sha256"]


def test_a_stuffed_byte_on_demand_decodes():
    d = LF.with_stuffed_byte(np.random.default_rng(3).integers(-5, 6, size=(3, 9, 1)), at=(1, 4, 0))
    data = LF.write_differences(d, 16, 1, table=LF.FLAT)
    assert LF.has_stuffed_byte(data)
    assert np.array_equal(lowlevel.decode_lossless_host(data), LF.model_decode(d, 16, 1))


def test_component_ids_are_reported():
    assert lowlevel.lossless_info(golden("p12_ps4_c4_id67"))["component_id"] == [67, 77, 89, 75]
    assert lowlevel.lossless_info(golden("p8_ps1_c2_id0"))["component_id"] == [0, 255]


def test_the_rows_schedule_refuses_other_predictors():
    assert status_of(lowlevel.decode_lossless_host, golden("p16_ps4_pt0_c1"), algorithm=1) == "INVALID_ARGUMENT"


@pytest.mark.parametrize("ps", range(1, 8))
def test_schedules_on_their_seams_equal_the_model(ps):
    """band and tile edges of the wavefront schedule, chunk edges of the rows schedule, restart intervals that end on a band's last row
    and on its first"""
    k = lowlevel.lossless_kernel_shape()
    B, T, K = k["band_rows"], k["tile_columns"], k["chunk_samples"]
    shapes = [(B + 1, T + 1, 0), (2 * B + 1, 2 * T + 1, 0), (B - 1, T - 1, 0), (2 * B + 2, 5, B), (2 * B + 2, 5, B + 1), (B + 3, 3, 1)]
    if ps == 1:
        shapes += [(3, K - 1, 0), (3, K + 1, 2), (2, 2 * K + 1, 1)]
    for i, (h, w, rr) in enumerate(shapes):
        rng = np.random.default_rng(ps * 100 + i)
        d = rng.integers(0, 65536, size=(h, w, 1))
        data = LF.write_differences(d, 16, ps, 0, rr, table=LF.FLAT)
        want = LF.model_decode(d, 16, ps, 0, rr)
        for algorithm in (None, 0, 2) + ((1,) if ps == 1 else ()):
            assert np.array_equal(lowlevel.decode_lossless_host(data, algorithm=algorithm), want), (h, w, rr, algorithm)


def test_refusals():
    want = {"refused_dri_not_rows": "UNSUPPORTED", "refused_ps0": "BAD_JPEG", "refused_ps8": "BAD_JPEG", "refused_al_ge_p": "BAD_JPEG",
            "refused_symbol17": "BAD_JPEG"}
    for name, status in want.items():
        assert status_of(lowlevel.lossless_info, golden(name)) == status, name
        assert status_of(lowlevel.decode_lossless_host, golden(name)) == status, name
    d = LF.differences_of_states(LF.random_samples(5, 6, 8, 3, 8), 8, 1)
    # valid files outside the rules
    assert status_of(lowlevel.lossless_info, LF.write_differences(d, 8, 1, sampling=[(2, 2), (1, 1), (1, 1)])) == "UNSUPPORTED"
    one_scan_per_component = LF.write_differences(d[:, :, :1], 8, 1, comp_ids=[1])
    three = LF.write_differences(d, 8, 1)
    sof = three.index(b"\xff\xc3")
    sos = one_scan_per_component.index(b"\xff\xda")
    assert status_of(lowlevel.lossless_info, three[:three.index(b"\xff\xda")] + one_scan_per_component[sos:]) == "UNSUPPORTED"
    assert sof > 0
    # malformed ones
    assert status_of(lowlevel.lossless_info, LF.write_differences(d, 8, 1, scan_header=(1, 1, 0, 0))) == "BAD_JPEG"  # Se != 0
    assert status_of(lowlevel.lossless_info, LF.write_differences(d, 8, 1, scan_header=(1, 0, 1, 0))) == "BAD_JPEG"  # Ah != 0
    no_table = LF.write_differences(d[:, :, :1], 8, 1)
    dht = no_table.index(b"\xff\xc4")
    length = int.from_bytes(no_table[dht + 2:dht + 4], "big")
    assert status_of(lowlevel.lossless_info, no_table[:dht] + no_table[dht + 2 + length:]) == "BAD_JPEG"
    for precision in (1, 17):
        bad = bytearray(three)
        bad[sof + 4] = precision
        assert status_of(lowlevel.lossless_info, bytes(bad)) == "BAD_JPEG"
    # a DCT file is not this decoder's
    dct = open(os.path.join(GOLDEN, "decode", json.load(open(os.path.join(GOLDEN, "manifest.json")))["decode"][0]["name"] + ".jpg"), "rb").read()
    assert status_of(lowlevel.lossless_info, dct) == "UNSUPPORTED"
    # uint8 samples of a file of more than eight bits
    assert status_of(lowlevel.decode_lossless_host, golden("p12_ps1_pt0_c1"), dtype=np.uint8) == "UNSUPPORTED"


def test_truncated_and_corrupt_streams():
    data = golden("p16_ps7_pt0_c3")
    sos = data.index(b"\xff\xda")
    body = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    for cut in (body, body + 1, (body + len(data)) // 2, len(data) - 3):
        assert status_of(lowlevel.decode_lossless_host, data[:cut]) == "TRUNCATED", cut
        assert status_of(lowlevel.decode_lossless_host, data[:cut] + b"\xff\xd9") == "TRUNCATED", cut
    assert status_of(lowlevel.decode_lossless_host, data[:sos + 3]) == "TRUNCATED"  # inside the scan header
    rst = golden("rst1_p12_ps3_c1")
    first = rst.index(b"\xff\xd0")
    wrong = bytearray(rst)
    wrong[first + 1] = 0xD3
    assert status_of(lowlevel.decode_lossless_host, bytes(wrong)) == "CORRUPT"
    assert status_of(lowlevel.decode_lossless_host, rst[:first] + rst[first + 2:]) == "CORRUPT"  # the marker is missing
    early = rst[:first - 1] + rst[first:]  # a byte of the first interval is missing: the marker comes where bits should be
    assert status_of(lowlevel.decode_lossless_host, early) in ("CORRUPT", "TRUNCATED")
    # a code no table holds: the long table leaves code words free
    d = np.zeros((4, 40, 1), dtype=np.int64)
    f = bytearray(LF.write_differences(d, 16, 1, table=LF.LONG))
    sos = f.index(b"\xff\xda")
    body = sos + 2 + int.from_bytes(f[sos + 2:sos + 4], "big")
    f[body:body + 4] = b"\xff\x00\xfe\xfe"  # sixteen one-bits are no code word
    assert status_of(lowlevel.decode_lossless_host, bytes(f)) == "CORRUPT"


def test_damaged_files_neither_crash_nor_hang():
    rng = np.random.default_rng(7)
    names = [c["name"] for c in CASES]
    seen = set()
    for i in range(200):
        data = bytearray(golden(names[int(rng.integers(len(names)))]))
        for _ in range(int(rng.integers(1, 6))):
            kind = int(rng.integers(3))
            at = int(rng.integers(2, len(data)))
            if kind == 0:
                data[at] = int(rng.integers(256))
            elif kind == 1:
                del data[at:at + int(rng.integers(1, 9))]
            else:
                data[at:at] = bytes(rng.integers(0, 256, size=int(rng.integers(1, 5)), dtype=np.uint8))
        data = bytes(data)
        st = status_of(lowlevel.lossless_info, data)
        seen.add(st)
        if st != "SUCCESS":
            continue
        info = lowlevel.lossless_info(data)
        if info["width"] * info["height"] > 1 << 22:
            continue  # a damaged size field: nothing to learn from a huge empty picture
        for algorithm in (None, 0):
            seen.add(status_of(lowlevel.decode_lossless_host, data, algorithm=algorithm))
    assert seen <= {"SUCCESS", "BAD_JPEG", "UNSUPPORTED", "TRUNCATED", "CORRUPT"}, seen
    assert len(seen) >= 3


def test_the_other_entry_points_still_call_a_lossless_frame_unsupported():
    data = golden("p8_ps1_pt0_c3")
    assert status_of(lowlevel.get_image_info, data) == "UNSUPPORTED"
    assert status_of(lowlevel.entropy_decode_host, data) == "UNSUPPORTED"
    assert status_of(lowlevel.coefficient_info, data) == "UNSUPPORTED"
    assert status_of(lowlevel.decode_coefficients_host, data) == "UNSUPPORTED"
    assert status_of(lowlevel.transcode_host, data) == "UNSUPPORTED"
    assert status_of(lowlevel.transcode_host, golden("p16_ps4_pt0_c1")) == "UNSUPPORTED"


@pytest.mark.parametrize("name,sixteen", [("p16_ps4_pt0_c1", True), ("p12_ps2_pt2_c3", True), ("p8_ps1_pt0_c3", False)])
def test_the_host_harness_reports_size_sample_type_and_precision(name, sixteen):
    case = next(c for c in CASES if c["name"] == name)
    lib = A.bind(N.load_host())
    ci = A.init(A.InstanceCreateInfo, A.ST_INSTANCE_CREATE_INFO, load_builtin_modules=1, load_extension_modules=0)
    inst = ctypes.c_void_p()
    assert lib.nvimgcodecInstanceCreate(ctypes.byref(inst), ctypes.byref(ci)) == 0
    try:
        arr = np.frombuffer(golden(name), dtype=np.uint8)
        cs = ctypes.c_void_p()
        assert lib.nvimgcodecCodeStreamCreateFromHostMem(inst, ctypes.byref(cs), arr.ctypes.data, arr.size) == 0
        ji = A.init(A.JpegImageInfo, A.ST_JPEG_IMAGE_INFO)
        info = A.init(A.ImageInfo, A.ST_IMAGE_INFO, struct_next=ctypes.addressof(ji))
        assert lib.nvimgcodecCodeStreamGetImageInfo(cs, ctypes.byref(info)) == 0
        assert info.codec_name == b"jpeg"
        assert info.num_planes == case["components"]
        for p in range(info.num_planes):
            pi = info.plane_info[p]
            assert (pi.width, pi.height, pi.num_channels, pi.precision) == (case["width"], case["height"], 1, case["precision"])
            assert pi.sample_type == (A.SAMPLE_DATA_TYPE_UINT16 if sixteen else A.SAMPLE_DATA_TYPE_UINT8)
        assert ji.encoding == 0xC3  # NVIMGCODEC_JPEG_ENCODING_LOSSLESS_HUFFMAN
        lib.nvimgcodecCodeStreamDestroy(cs)
    finally:
        lib.nvimgcodecInstanceDestroy(inst)
