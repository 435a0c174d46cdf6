"""Goldens for the lossless (SOF3) coder: tests/golden/lossless_encode/*.jpg and manifest_lossless_encode.json.  Run by hand where
Pillow and its bundled libjpeg-turbo are installed; the tests only read what it wrote.

The files come from the LIVE libjpeg-turbo that Pillow ships, driven through ctypes: jpeg_CreateCompress, jpeg_mem_dest,
jpeg_set_defaults, jpeg_enable_lossless and jpeg_write_scanlines / jpeg12_write_scanlines / jpeg16_write_scanlines (precision 2..8,
9..12, 13..16).  The jpeg_compress_struct fields used (libjpeg-turbo 3.x, 64-bit): image_width @48, image_height @52,
input_components @56, in_color_space @60, data_precision @72, restart_in_rows @284; the structure is 520 bytes.

The binding is validated, not trusted.  For every file the SOF3 read back must hold the P, H, W and N asked for, SOS the predictor and
the point transform, DRI restart_rows * W, and the library's own decompressor (the binding of make_golden_lossless.py) must return
(samples >> Pt) << Pt.  Every case runs in a child process, because the library's error exit ends the process.  The generator then
asserts that the numpy model (tests/helpers/lossless_encode_model.py) writes the very same bytes.

Files whose entropy-coded segment exceeds 4 KB are kept as sha256 only.

    python tests/golden/make_golden_lossless_encode.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_lossless as D  # noqa: E402
import make_golden_plain_upsampling as B  # noqa: E402
from helpers import lossless_encode_model as M  # noqa: E402

OUT = os.path.join(HERE, "lossless_encode")
MANIFEST = os.path.join(HERE, "manifest_lossless_encode.json")
STRUCT_BYTES = 520
OFF_IMAGE_WIDTH, OFF_IMAGE_HEIGHT, OFF_INPUT_COMPONENTS, OFF_IN_COLOR_SPACE, OFF_DATA_PRECISION, OFF_RESTART_IN_ROWS = 48, 52, 56, 60, 72, 284
JCS = {1: 1, 2: 0, 3: 2, 4: 4}  # components -> JCS_GRAYSCALE, JCS_UNKNOWN, JCS_RGB, JCS_CMYK
KEEP_BYTES = 4096


def load():
    lib = D.load()
    lib.jpeg_CreateCompress.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.jpeg_mem_dest.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)]
    lib.jpeg_set_defaults.argtypes = [C.c_void_p]
    lib.jpeg_enable_lossless.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.jpeg_start_compress.argtypes = [C.c_void_p, C.c_int]
    for name in ("jpeg_write_scanlines", "jpeg12_write_scanlines", "jpeg16_write_scanlines"):
        fn = getattr(lib, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        fn.restype = C.c_uint
    lib.jpeg_finish_compress.argtypes = [C.c_void_p]
    lib.jpeg_destroy_compress.argtypes = [C.c_void_p]
    return lib


def compress(samples, precision, ps, pt, restart_rows):
    """samples: H x W x N, uint8 (precision <= 8) or uint16.  -> the library's file"""
    lib = load()
    s = np.ascontiguousarray(samples)
    h, w, n = s.shape
    err = C.create_string_buffer(1024)
    cinfo = C.create_string_buffer(STRUCT_BYTES + 64)
    base = C.addressof(cinfo)

    def i32(off):
        return C.cast(base + off, C.POINTER(C.c_int))

    lib.jpeg_std_error(err)  # the default error_exit ends the process
    C.cast(cinfo, C.POINTER(C.c_void_p))[0] = C.addressof(err)
    lib.jpeg_CreateCompress(cinfo, 62, STRUCT_BYTES)
    out, size = C.c_void_p(), C.c_ulong(0)
    lib.jpeg_mem_dest(cinfo, C.byref(out), C.byref(size))
    i32(OFF_IMAGE_WIDTH)[0], i32(OFF_IMAGE_HEIGHT)[0], i32(OFF_INPUT_COMPONENTS)[0], i32(OFF_IN_COLOR_SPACE)[0] = w, h, n, JCS[n]
    i32(OFF_DATA_PRECISION)[0] = precision
    lib.jpeg_set_defaults(cinfo)
    i32(OFF_DATA_PRECISION)[0] = precision
    lib.jpeg_enable_lossless(cinfo, ps, pt)
    i32(OFF_RESTART_IN_ROWS)[0] = restart_rows
    lib.jpeg_start_compress(cinfo, 1)
    write = lib.jpeg_write_scanlines if precision <= 8 else lib.jpeg12_write_scanlines if precision <= 12 else lib.jpeg16_write_scanlines
    assert s.dtype == (np.uint8 if precision <= 8 else np.uint16)
    row = (C.c_void_p * 1)()
    for y in range(h):
        row[0] = s.ctypes.data + y * s.strides[0]
        assert write(cinfo, row, 1) == 1
    lib.jpeg_finish_compress(cinfo)
    data = C.string_at(out.value, size.value)
    lib.jpeg_destroy_compress(cinfo)
    return data


def cases():
    """-> manifest entries without the results"""
    out = []

    def add(name, seed, h, w, n, P, ps, pt=0, rr=0, smooth=True, kind="random"):
        out.append({"name": name, "seed": seed, "height": h, "width": w, "components": n, "precision": P, "predictor": ps, "point_transform": pt,
                    "restart_rows": rr, "smooth": smooth, "kind": kind})

    seed = 100
    for ps in range(1, 8):
        for k, P in enumerate((2, 8, 9, 12, 16)):
            seed += 1
            n = 1 + (ps + k) % 4
            pt = (0, 1, 0, 2, 3)[(ps + k) % 5] if P > 2 else (ps % 2)
            rr = (0, 1, 3, 0, 5)[(ps + 2 * k) % 5]  # 13 rows: 1 gives 13 intervals (RSTn wraps), 3 and 5 do not divide the height
            add(f"p{P}_ps{ps}_pt{pt}_c{n}_rst{rr}", seed, 13, 17, n, P, ps, pt, rr, smooth=seed % 2 == 0)
    for n in (1, 2, 3, 4):
        add(f"noisy_p16_c{n}", 200 + n, 9, 21, n, 16, 4, 0, 2, smooth=False)
        add(f"smooth_p8_c{n}", 210 + n, 9, 21, n, 8, 1, 0, 0, smooth=True)
    add("constant_p8", 77, 8, 11, 3, 8, 1, kind="constant")
    add("constant_p12_rst1", 1234, 10, 7, 1, 12, 7, 0, 1, kind="constant")
    add("ssss16_p16", 300, 7, 12, 1, 16, 1, kind="ssss16", smooth=False)
    add("ssss16_p16_c2_rst2", 301, 6, 10, 2, 16, 1, 0, 2, kind="ssss16", smooth=False)
    add("one_by_one_p8", 310, 1, 1, 1, 8, 1)
    add("one_by_one_p16_c3", 311, 1, 1, 3, 16, 5)
    add("one_row_p12", 312, 1, 29, 3, 12, 6, 1)
    add("one_column_p8_rst1", 313, 23, 1, 1, 8, 2, 0, 1)
    add("one_column_p16_c4", 314, 23, 1, 4, 16, 3, 2)
    add("rst_above_height_p8", 315, 5, 9, 3, 8, 4, 0, 9)
    # larger than a few KB: sha256 only.  The second one is two stuffing chunks and more than one workgroup of the write kernel.
    add("large_noisy_p16_c3", 400, 48, 64, 3, 16, 7, 0, 0, smooth=False)
    add("large_smooth_p12_rst4", 401, 70, 129, 1, 12, 1, 1, 4, smooth=True)
    add("large_noisy_p8_c4_rst1", 402, 40, 100, 4, 8, 2, 0, 1, smooth=False)
    return out


def child(spec_path, out_path):
    """One case in a process of its own: compress, check with the library's decompressor, write the file"""
    e = json.load(open(spec_path))
    s = M.case_samples(e)
    data = compress(s, e["precision"], e["predictor"], e["point_transform"], e["restart_rows"])
    got, precision = D.Decoder().decode(data, unchanged=True)
    assert precision == e["precision"], ("data_precision", precision)
    want = M.expected(s, e["point_transform"])
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), "the library does not decode its own file to (s >> Pt) << Pt"
    open(out_path, "wb").write(data)


def main():
    from PIL import features
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    entries, kept = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        for e in cases():
            spec, path = os.path.join(tmp, "spec.json"), os.path.join(tmp, "out.jpg")
            json.dump(e, open(spec, "w"))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, path], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, ("the library refused or failed a case", e["name"], r.stderr[-2000:])
            data = open(path, "rb").read()
            os.remove(path)
            # the binding is validated: the markers must say what was asked for
            m = M.parse(data)
            h, w, n = e["height"], e["width"], e["components"]
            assert (m["precision"], m["height"], m["width"], m["components"]) == (e["precision"], h, w, n), (e["name"], m)
            assert (m["predictor"], m["point_transform"], m["se"], m["ah"]) == (e["predictor"], e["point_transform"], 0, 0), (e["name"], m)
            assert m["dri"] == e["restart_rows"] * w, (e["name"], m["dri"])
            assert m["dht"] == [0] and m["scan_tables"] == [0] * n and m["ids"] == list(M.COMPONENT_IDS[n]) == m["scan_ids"], (e["name"], m)
            s = M.case_samples(e)
            if e["point_transform"]:
                assert (s.astype(np.int64) & ((1 << e["point_transform"]) - 1)).any() or e["kind"] == "constant", e["name"]
            if e["kind"] == "ssss16":
                assert (M.differences(s, 16, e["predictor"], 0, e["restart_rows"]) == 32768).any(), e["name"]
            model = M.model_file(s, e["precision"], e["predictor"], e["point_transform"], e["restart_rows"])
            assert model == data, ("the numpy model is not the library", e["name"], len(model), len(data))
            e["bytes"] = len(data)
            e["scan_bytes"] = len(data) - m["scan_at"] - 2
            e["sha256"] = hashlib.sha256(data).hexdigest()
            e["stored"] = e["scan_bytes"] <= KEEP_BYTES
            if e["stored"]:
                open(os.path.join(OUT, e["name"] + ".jpg"), "wb").write(data)
                kept += len(data)
            entries.append(e)
    assert kept < 512 * 1024, kept
    out = {"generator": "tests/golden/make_golden_lossless_encode.py", "libjpeg_turbo": features.version_feature("libjpeg_turbo"),
           "library": os.path.basename(B.library_path()), "jpeg_compress_struct_bytes": STRUCT_BYTES, "lossless_encode": entries}
    json.dump(out, open(MANIFEST, "w"), indent=1)
    print("wrote manifest_lossless_encode.json:", len(entries), "cases,", sum(e["stored"] for e in entries), "files kept,", kept, "bytes")


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()
