"""Goldens for the lossless (SOF3) decoder: tests/golden/lossless/*.jpg and manifest_lossless.json.  Run by hand where Pillow and its
bundled libjpeg-turbo are installed; the tests only read what it wrote.

The files come from tests/helpers/lossless_files.py; the samples they must decode to come from the LIVE libjpeg-turbo that Pillow
ships, driven through the ctypes binding of make_golden_plain_upsampling.py with jpeg12_read_scanlines / jpeg16_read_scanlines
added (samples of precision 9..12 leave through the former, 13..16 through the latter, 2..8 through jpeg_read_scanlines).

The binding is validated, not trusted: data_precision (the int at offset 296 of jpeg_decompress_struct) must read back the P of
every file, and the 8-bit files must equal Pillow's own decode.  The generator asserts that the library decodes EVERY golden, none
refused, and that the numpy model of the helper equals the library on every one; the manifest keeps the sha256 of the library's
samples.  Files the library refuses (its error exit ends the process, so each is tried in a child) are a separate named list.

    python tests/golden/make_golden_lossless.py
"""
import ctypes as C
import hashlib
import io
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_plain_upsampling as B  # noqa: E402
from helpers import lossless_files as LF  # noqa: E402

OUT = os.path.join(HERE, "lossless")
OFF_DATA_PRECISION = 296
OFF_JPEG_COLOR_SPACE = 60  # J_COLOR_SPACE jpeg_color_space, in front of out_color_space


def load():
    lib = B.load()
    for name in ("jpeg12_read_scanlines", "jpeg16_read_scanlines"):
        fn = getattr(lib, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        fn.restype = C.c_uint
    return lib


class Decoder:
    def __init__(self):
        self.lib = load()
        self.size = B.struct_size()
        assert 400 < self.size < 1024, self.size

    def decode(self, data, unchanged=False):
        """-> (samples H x W x N, uint8 for precision <= 8 else uint16, exactly what the library wrote; data_precision)"""
        lib = self.lib
        err = C.create_string_buffer(1024)
        cinfo = C.create_string_buffer(self.size + 64)
        base = C.addressof(cinfo)

        def i32(off):
            return C.cast(base + off, C.POINTER(C.c_int))

        lib.jpeg_std_error(err)  # the default error_exit ends the process
        C.cast(cinfo, C.POINTER(C.c_void_p))[0] = C.addressof(err)
        lib.jpeg_CreateDecompress(cinfo, 62, self.size)
        buf = C.create_string_buffer(bytes(data), len(data))
        lib.jpeg_mem_src(cinfo, buf, len(data))
        assert lib.jpeg_read_header(cinfo, 1) == 1
        precision = i32(OFF_DATA_PRECISION)[0]
        if unchanged:
            i32(B.OFF_OUT_COLOR_SPACE)[0] = i32(OFF_JPEG_COLOR_SPACE)[0]  # the components as stored
        lib.jpeg_start_decompress(cinfo)
        ow, oh, oc = i32(B.OFF_OUTPUT_WIDTH)[0], i32(B.OFF_OUTPUT_HEIGHT)[0], i32(B.OFF_OUTPUT_COMPONENTS)[0]
        assert (ow, oh, oc) == (i32(B.OFF_IMAGE_WIDTH)[0], i32(B.OFF_IMAGE_HEIGHT)[0], i32(B.OFF_NUM_COMPONENTS)[0])
        read = lib.jpeg_read_scanlines if precision <= 8 else lib.jpeg12_read_scanlines if precision <= 12 else lib.jpeg16_read_scanlines
        out = np.zeros((oh, ow * oc), dtype=np.uint8 if precision <= 8 else np.uint16)
        row = (C.c_void_p * 1)()
        while i32(B.OFF_OUTPUT_SCANLINE)[0] < oh:
            row[0] = out.ctypes.data + i32(B.OFF_OUTPUT_SCANLINE)[0] * out.strides[0]
            assert read(cinfo, row, 1) == 1
        lib.jpeg_finish_decompress(cinfo)
        lib.jpeg_destroy_decompress(cinfo)
        return out.reshape(oh, ow, oc), precision


def golden_cases():
    """-> [(name, file bytes, dict of parameters, differences)]"""
    cases = []

    def add(name, diffs, P, ps, pt, rr=0, **kw):
        data = LF.write_differences(diffs, P, ps, pt, rr, **kw)
        h, w, n = diffs.shape
        cases.append((name, data, {"name": name, "width": w, "height": h, "components": n, "precision": P, "predictor": ps,
                                   "point_transform": pt, "restart_rows": rr}, diffs))

    def of_samples(seed, h, w, n, P, ps, pt, rr=0, smooth=True):
        s = LF.random_samples(seed, h, w, n, P, pt, smooth)
        return LF.differences_of_states(s >> pt, P, ps, pt, rr)

    seed = 0
    for ps in range(1, 8):
        for P in (2, 8, 12, 16):
            for pt in ((0, 1) if P == 2 else (0, 2)):
                for n in (1, 3):
                    seed += 1
                    table = (LF.OPTIMAL, LF.FLAT, LF.LONG)[seed % 3]
                    add(f"p{P}_ps{ps}_pt{pt}_c{n}", of_samples(seed, 19, 23, n, P, ps, pt, smooth=seed % 2 == 0), P, ps, pt, table=table)
    for n, ids in ((2, (1, 2)), (4, (67, 77, 89, 75)), (2, (0, 255)), (4, (1, 2, 3, 4))):
        for ps, P in ((1, 8), (4, 12), (7, 16)):
            seed += 1
            add(f"p{P}_ps{ps}_c{n}_id{ids[0]}", of_samples(seed, 11, 17, n, P, ps, 0), P, ps, 0, comp_ids=ids)
    for rr in (1, 3):
        for ps in range(1, 8):
            for n, P in ((1, 12), (3, 8)):
                seed += 1
                add(f"rst{rr}_p{P}_ps{ps}_c{n}", of_samples(seed, 10, 21, n, P, ps, 0, rr), P, ps, 0, rr)
    # JFIF / Adobe markers change nothing about three stored components
    jfif = LF._marker(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    adobe = LF._marker(0xEE, b"Adobe\0\x64\0\0\0\0\x01")
    add("jfif_p8_ps1_c3", of_samples(901, 9, 13, 3, 8, 1, 0), 8, 1, 0, extra_markers=jfif)
    add("adobe_p8_ps4_c3", of_samples(902, 9, 13, 3, 8, 4, 0), 8, 4, 0, extra_markers=adobe)
    # SSSS = 16: a difference of 32768
    rng = np.random.default_rng(16)
    for ps in (1, 5, 7):
        d = rng.integers(0, 65536, size=(9, 15, 1))
        d[::2, ::3] = 32768
        add(f"ssss16_ps{ps}", d, 16, ps, 0, table=LF.FLAT)
    d = rng.integers(0, 65536, size=(6, 9, 3))
    d[1::2, 1::2] = 32768
    add("ssss16_c3_rst2", d, 16, 6, 0, 2, table=LF.LONG)
    # a stuffed byte for certain: 32767 under the flat table is nineteen one-bits in a row
    d = rng.integers(-3, 4, size=(5, 11, 1))
    d[2, 3:6] = 32767
    add("stuffed_p16_ps1", d, 16, 1, 0, table=LF.FLAT)
    # states outside 0 .. 2^P - 1: nothing clamps them
    for P in (2, 8, 9, 12):
        for ps in (1, 4, 7):
            d = rng.integers(-40, 41, size=(8, 13, 1))
            d[0, 0] = 40000 - (1 << (P - 1))  # the first state is 40000
            d[3, 5] = 30000
            d[5, 2] = -20000
            add(f"range_p{P}_ps{ps}", d, P, ps, 0)
    d = rng.integers(-300, 301, size=(7, 10, 3))
    d[0, 0] = 40000 - 256
    add("range_p9_ps5_pt1_c3", d, 9, 5, 1)
    return cases


def refused_cases():
    d = LF.differences_of_states(LF.random_samples(77, 6, 8, 1, 8), 8, 1)
    return [
        ("refused_dri_not_rows", LF.write_differences(d, 8, 1, restart_interval=5), "a restart interval that is not whole rows"),
        ("refused_ps0", LF.write_differences(d, 8, 1, scan_header=(0, 0, 0, 0)), "Ss = 0"),
        ("refused_ps8", LF.write_differences(d, 8, 1, scan_header=(8, 0, 0, 0)), "Ss = 8"),
        ("refused_al_ge_p", LF.write_differences(d, 8, 1, scan_header=(1, 0, 0, 8)), "Al >= P"),
        ("refused_symbol17", LF.write_differences(d, 8, 1, tables=[([0] * 5 + [18] + [0] * 11, list(range(18)))]), "a table symbol of 17"),
    ]


def try_decode(path):
    """Runs in a child: exit 0 when the library decodes the file"""
    Decoder().decode(open(path, "rb").read())


def main():
    from PIL import Image, features
    dec = Decoder()
    os.makedirs(OUT, exist_ok=True)
    entries, total, pillow_checked = [], 0, 0
    for name, data, entry, diffs in golden_cases():
        assert len(data) < 64 * 1024, name
        # a refusal ends the process: none may be refused.  A JFIF or Adobe marker makes the library call three components YCbCr, and
        # the RGB it would convert them to by default is a request lossless mode refuses ("Unsupported color conversion request"):
        # those files are read with out_color_space = jpeg_color_space, which is what "as stored" means to the library
        got, precision = dec.decode(data, unchanged=name.startswith(("jfif", "adobe")))
        assert precision == entry["precision"], ("data_precision does not read back P", name, precision)
        model = LF.model_decode(diffs, entry["precision"], entry["predictor"], entry["point_transform"], entry["restart_rows"])
        assert got.dtype == model.dtype and np.array_equal(got, model), ("the model is not the library", name)
        if entry["precision"] == 8 and entry["components"] in (1, 3) and not name.startswith(("range", "jfif", "adobe")):
            pil = np.asarray(Image.open(io.BytesIO(data)))
            assert np.array_equal(pil.reshape(got.shape), got), ("the binding's samples are not Pillow's", name)
            pillow_checked += 1
        entry["bytes"] = len(data)
        entry["stuffed"] = b"\xff\x00" in data
        entry["sha256"] = hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()
        entry["dtype"] = str(got.dtype)
        open(os.path.join(OUT, name + ".jpg"), "wb").write(data)
        entries.append(entry)
        total += len(data)
    assert pillow_checked >= 20, pillow_checked
    assert total < 1024 * 1024, total
    refused = []
    for name, data, why in refused_cases():
        path = os.path.join(OUT, name + ".jpg")
        open(path, "wb").write(data)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--try", path], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0, ("the library takes a file this list calls refused", name)
        refused.append({"name": name, "why": why, "library_says": r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""})
    out = {"generator": "tests/golden/make_golden_lossless.py", "libjpeg_turbo": features.version_feature("libjpeg_turbo"),
           "library": os.path.basename(B.library_path()), "jpeg_decompress_struct_bytes": dec.size, "pillow_checked": pillow_checked,
           "lossless": entries, "refused": refused}
    json.dump(out, open(os.path.join(HERE, "manifest_lossless.json"), "w"), indent=1)
    print("wrote manifest_lossless.json:", len(entries), "files,", total, "bytes;", len(refused), "refused;", pillow_checked, "checked against Pillow")


if __name__ == "__main__":
    if "--probe" in sys.argv:
        B.probe_struct_size()
    elif "--try" in sys.argv:
        try_decode(sys.argv[sys.argv.index("--try") + 1])
    else:
        main()
