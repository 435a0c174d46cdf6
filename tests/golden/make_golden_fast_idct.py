#!/usr/bin/env python3
"""Golden hashes for the fast integer IDCT (JDCT_IFAST; the decoder option `fast_idct=1`), from the REAL libjpeg-turbo.  Dev-container only.

The reference's libjpeg_turbo_decoder maps `fast_idct` to JDCT_FASTEST = JDCT_IFAST (extensions/libjpeg_turbo/jpeg_mem.cpp:177).  Pillow
cannot choose the DCT method, so this script drives the libjpeg-turbo that Pillow ships through its C API with the binding of
make_golden_plain_upsampling.py (struct size measured, field offsets validated there) and writes cinfo.dct_method = JDCT_IFAST in between.
That the switch reached the library is asserted: the pixels differ from the ISLOW goldens on subsampled, 4:4:4 and gray files alike.

Output: manifest_fast_idct.json (hashes only, no pixel files):
  * "decode": per file of tests/golden/decode, sha256 of the H x W x 3 RGB pixels (gray files expanded to RGB like the other manifests)
    with fancy upsampling on ("rgb_sha256") and off ("plain_rgb_sha256");
  * "cmyk": sha256 of the library's CMYK samples of every file of tests/golden/cmyk (fancy upsampling on);
  * "gamut": the 43 out-of-gamut vectors of tests/golden/gamut, each decoded in a child process under default dispatch, JSIMD_FORCESSE2=1 and
    JSIMD_FORCENONE=1 (gray files as H x W, colour as H x W x 3); the first two must agree ("simd_sha256"), the third is the C routine's
    ("c_sha256");
  * "roi": regions of interest decoded with the reference's crop recipe (the windows make_golden_plain_upsampling.py chose), fancy upsampling
    on and off, each asserted equal to the same window of the full decode.
Usage: make_golden_fast_idct.py [--out PATH] (default: manifest_fast_idct.json beside this script)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_plain_upsampling as mp  # noqa: E402

JDCT_ISLOW, JDCT_IFAST = 0, 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Decoder(mp.Decoder):
    def decode(self, data, fancy, roi=None, dct=JDCT_IFAST, expand=True):
        """make_golden_plain_upsampling.Decoder.decode with the DCT method chosen too"""
        lib = self.lib
        err = C.create_string_buffer(1024)
        cinfo = C.create_string_buffer(self.size + 64)
        base = C.addressof(cinfo)

        def i32(off):
            return C.cast(base + off, C.POINTER(C.c_int))

        lib.jpeg_std_error(err)
        C.cast(cinfo, C.POINTER(C.c_void_p))[0] = C.addressof(err)
        lib.jpeg_CreateDecompress(cinfo, 62, self.size)
        buf = C.create_string_buffer(bytes(data), len(data))
        lib.jpeg_mem_src(cinfo, buf, len(data))
        assert lib.jpeg_read_header(cinfo, 1) == 1
        ncomp = i32(mp.OFF_NUM_COMPONENTS)[0]
        assert i32(mp.OFF_DCT_METHOD)[0] == JDCT_ISLOW and i32(mp.OFF_DO_FANCY)[0] == 1
        i32(mp.OFF_DO_FANCY)[0] = 1 if fancy else 0
        i32(mp.OFF_DCT_METHOD)[0] = dct
        lib.jpeg_start_decompress(cinfo)
        ow, oh, oc = i32(mp.OFF_OUTPUT_WIDTH)[0], i32(mp.OFF_OUTPUT_HEIGHT)[0], i32(mp.OFF_OUTPUT_COMPONENTS)[0]
        assert oc == ncomp
        row = (C.c_void_p * 1)()
        if roi is None:
            out = np.zeros((oh, ow * oc), dtype=np.uint8)
            while i32(mp.OFF_OUTPUT_SCANLINE)[0] < oh:
                y = i32(mp.OFF_OUTPUT_SCANLINE)[0]
                row[0] = out.ctypes.data + y * out.strides[0]
                assert lib.jpeg_read_scanlines(cinfo, row, 1) == 1
            lib.jpeg_finish_decompress(cinfo)
            out = out.reshape(oh, ow, oc)
        else:
            x, y, w, h = roi
            left = 0 if x == 0 else 1
            right = max(0, min(1, ow - (x + w)))
            cx, cw = C.c_uint(x - left), C.c_uint(w + left + right)
            lib.jpeg_crop_scanline(cinfo, C.byref(cx), C.byref(cw))
            assert lib.jpeg_skip_scanlines(cinfo, y) == y
            out = np.zeros((h, cw.value * oc), dtype=np.uint8)
            for r in range(h):
                row[0] = out.ctypes.data + r * out.strides[0]
                assert lib.jpeg_read_scanlines(cinfo, row, 1) == 1
            lib.jpeg_abort_decompress(cinfo)
            out = out.reshape(h, cw.value, oc)[:, x - cx.value:x - cx.value + w]
        lib.jpeg_destroy_decompress(cinfo)
        if oc == 1:
            return np.repeat(out, 3, axis=2) if expand else out[:, :, 0]
        return out


def child(paths):
    """Runs in a child process (the SIMD dispatch is chosen once per process from the environment): one hash per file."""
    dec = Decoder()
    for p in paths:
        print(sha(dec.decode(open(p, "rb").read(), True, expand=False)), flush=True)


def gamut_hashes(paths, env_extra):
    env = dict(os.environ)
    for k in ("JSIMD_FORCENONE", "JSIMD_FORCESSE2", "JSIMD_FORCEAVX2"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + paths, env=env, capture_output=True, text=True, timeout=600,
                         check=True).stdout.split()
    assert len(out) == len(paths), out
    return out


def main(out_path=os.path.join(HERE, "manifest_fast_idct.json")):
    from PIL import features
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    assert features.version_feature("libjpeg_turbo") == manifest["libjpeg_turbo"], "the goldens come from another library version"
    plain = {c["name"]: c for c in json.load(open(os.path.join(HERE, "manifest_plain.json")))["decode"]}
    dec = Decoder()
    cases, differ = [], {}
    for c in manifest["decode"]:
        data = open(os.path.join(HERE, "decode", c["name"] + ".jpg"), "rb").read()
        # the binding decodes with ISLOW exactly what the other manifests hold
        assert sha(dec.decode(data, True, dct=JDCT_ISLOW)) == c["rgb_sha256"], c["name"]
        assert sha(dec.decode(data, False, dct=JDCT_ISLOW)) == plain[c["name"]]["plain_rgb_sha256"], c["name"]
        on, off = sha(dec.decode(data, True)), sha(dec.decode(data, False))
        kind = "sub" if c["sub"] not in ("444", "gray") else c["sub"]
        differ.setdefault(kind, 0)
        differ[kind] += int(on != c["rgb_sha256"])
        cases.append({"name": c["name"], "sub": c["sub"], "width": c["width"], "height": c["height"], "rgb_sha256": on, "plain_rgb_sha256": off})
    # the switch reached the library: IFAST pixels differ from ISLOW on every kind of file
    assert differ["sub"] > 40 and differ["444"] > 20 and differ["gray"] > 15, differ
    # regions of interest: the windows of manifest_plain.json (one spare pixel left and right, jpeg_crop_scanline, jpeg_skip_scanlines)
    rois = []
    for r in json.load(open(os.path.join(HERE, "manifest_plain.json")))["roi"]:
        data = open(os.path.join(HERE, "decode", r["name"] + ".jpg"), "rb").read()
        x, y, w, h = r["roi"]
        got = dec.decode(data, r["fancy"], roi=(x, y, w, h))
        full = dec.decode(data, r["fancy"])
        assert np.array_equal(got, full[y:y + h, x:x + w]), ("a region of interest that is not the window of the full decode", r)
        rois.append({"name": r["name"], "fancy": r["fancy"], "roi": r["roi"], "rgb_sha256": sha(got)})
    # four-component files: the library's CMYK samples (the reference turns them into RGB itself, jpeg_mem.cpp:292-337)
    cmyk = []
    for c in json.load(open(os.path.join(HERE, "manifest_cmyk.json")))["cmyk"]:
        data = open(os.path.join(HERE, "cmyk", c["name"] + ".jpg"), "rb").read()
        ref = np.fromfile(os.path.join(HERE, "cmyk", c["name"] + ".cmyk"), dtype=np.uint8).reshape(c["height"], c["width"], 4)
        assert np.array_equal(dec.decode(data, True, dct=JDCT_ISLOW), ref), c["name"]
        cmyk.append({"name": c["name"], "kind": c["kind"], "subsampled": c["subsampled"], "width": c["width"], "height": c["height"],
                     "cmyk_sha256": sha(dec.decode(data, True))})
    # out-of-gamut vectors: which IFAST routine is the judge
    gm = json.load(open(os.path.join(HERE, "manifest_gamut.json")))["gamut"]
    paths = [os.path.join(HERE, "gamut", g["name"] + ".jpg") for g in gm]
    simd, sse2, plain_c = gamut_hashes(paths, {}), gamut_hashes(paths, {"JSIMD_FORCESSE2": "1"}), gamut_hashes(paths, {"JSIMD_FORCENONE": "1"})
    assert simd == sse2, "default dispatch and JSIMD_FORCESSE2=1 disagree"
    gamut = [{"name": g["name"], "width": g["width"], "height": g["height"], "mode": g["mode"], "simd_sha256": a, "c_sha256": b, "simd_equals_c": a == b}
             for g, a, b in zip(gm, simd, plain_c)]
    out = {"generator": "tests/golden/make_golden_fast_idct.py", "libjpeg_turbo": manifest["libjpeg_turbo"], "library": os.path.basename(mp.library_path()),
           "dct_method": "JDCT_IFAST", "files_that_differ_from_islow": differ,
           "dispatch": "gamut: default == JSIMD_FORCESSE2=1 (simd_sha256); c_sha256 from JSIMD_FORCENONE=1",
           "decode": cases, "cmyk": cmyk, "gamut": gamut, "roi": rois}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote manifest_fast_idct.json:", len(cases), "files", differ, "differ from ISLOW;", len(rois), "regions;", len(cmyk), "CMYK;",
          len(gamut), "gamut vectors,", sum(not g["simd_equals_c"] for g in gamut), "where SIMD and C differ")


if __name__ == "__main__":
    if "--probe" in sys.argv:
        mp.probe_struct_size()
    elif "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1:])
    elif "--out" in sys.argv:
        main(sys.argv[sys.argv.index("--out") + 1])
    else:
        main()
