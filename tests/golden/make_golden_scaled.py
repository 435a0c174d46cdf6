#!/usr/bin/env python3
"""Golden hashes for decoding at 1/2, 1/4 and 1/8 scale (scale_num / scale_denom), from the REAL libjpeg-turbo.  Dev-container only.

The binding is make_golden_plain_upsampling.py's (ctypes on the libjpeg-turbo Pillow ships, struct size and offsets validated there); this
script adds three fields of `struct jpeg_decompress_struct` (libjpeg API 6.2, LP64): scale_num at 68, scale_denom at 72 (both must read 1
behind jpeg_read_header) and dct_method at 96 (JDCT_ISLOW = 0, JDCT_IFAST = 1).  Pillow's draft() is NOT the reference: it equals no one
setting of the library on subsampled files.

Files: every file of manifest.json["decode"], the files of manifest_sampling.json (rebuilt by tests/helpers/sampling_goldens.py, the
layouts the library refuses included), the 43 files of gamut/, and a set of tiny files this script writes itself into scaled/:
1x1, 7x5, 17x9 and 33x17 in gray, 4:4:4, 4:2:2, 4:2:0 and 4:4:0, each baseline and progressive (Pillow writes them; 4:4:0 comes from the
oracle's encoder, its progressive twin from the same coefficients through tests/helpers/jpeg_from_coefficients.py).

Output: manifest_scaled.json -- per file and denominator 2, 4, 8: the scaled size (asserted against ceil(w k / 8), k = 8 / denominator),
the sha256 of the H x W x 3 RGB pixels with JDCT_ISLOW and fancy upsampling (gray files expanded to RGB like the other goldens), and the
hashes of (ISLOW, plain), (IFAST, fancy), (IFAST, plain) ONLY where they differ from the first.  Four-component files have "components": 4
and the hash of the library's CMYK samples (the decoder refuses them at a scale).  The scaled/ files carry "y_sha256" as well: the
library's JCS_GRAYSCALE decode (ISLOW, fancy).  A (file, denominator) the library refuses -- its error_exit ends the process, so every
decode runs in a worker child -- is recorded as "refused": true.

Self-checks (a dead switch cannot pass): some 4:2:2 file differs between fancy and plain at 1/2 and at 1/4, none at 1/8; some 4:2:0 file
differs between ISLOW and IFAST at 1/2; no 4:4:4 or gray file differs under either switch."""
import ctypes as C
import glob
import hashlib
import io
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import make_golden_plain_upsampling as P  # noqa: E402

OFF_SCALE_NUM, OFF_SCALE_DENOM = 68, 72
JDCT_ISLOW, JDCT_IFAST = 0, 1
DENOMS = (2, 4, 8)
SETTINGS = (("islow_fancy", False, True), ("islow_plain", False, False), ("ifast_fancy", True, True), ("ifast_plain", True, False))
TINY_SIZES = ((1, 1), (7, 5), (17, 9), (33, 17))
TINY_SUBS = ("gray", "444", "422", "420", "440")


def scaled_size(w, h, denom):
    k = 8 // denom
    return -(-w * k // 8), -(-h * k // 8)


class ScaledDecoder(P.Decoder):
    def decode_scaled(self, data, denom, ifast, fancy, gray=False):
        lib = self.lib
        err = C.create_string_buffer(1024)
        cinfo = C.create_string_buffer(self.size + 64)
        base = C.addressof(cinfo)

        def i32(off):
            return C.cast(base + off, C.POINTER(C.c_int))

        lib.jpeg_std_error(err)  # the default error_exit ends the process: this runs in a worker child
        C.cast(cinfo, C.POINTER(C.c_void_p))[0] = C.addressof(err)
        lib.jpeg_CreateDecompress(cinfo, 62, self.size)
        buf = C.create_string_buffer(bytes(data), len(data))
        lib.jpeg_mem_src(cinfo, buf, len(data))
        assert lib.jpeg_read_header(cinfo, 1) == 1
        width, height, ncomp = i32(P.OFF_IMAGE_WIDTH)[0], i32(P.OFF_IMAGE_HEIGHT)[0], i32(P.OFF_NUM_COMPONENTS)[0]
        assert i32(OFF_SCALE_NUM)[0] == 1 and i32(OFF_SCALE_DENOM)[0] == 1
        assert i32(P.OFF_DCT_METHOD)[0] == JDCT_ISLOW and i32(P.OFF_DO_FANCY)[0] == 1
        i32(OFF_SCALE_DENOM)[0] = denom
        i32(P.OFF_DCT_METHOD)[0] = JDCT_IFAST if ifast else JDCT_ISLOW
        i32(P.OFF_DO_FANCY)[0] = 1 if fancy else 0
        if gray:
            assert ncomp in (1, 3)
            i32(P.OFF_OUT_COLOR_SPACE)[0] = P.JCS_GRAYSCALE
        lib.jpeg_start_decompress(cinfo)
        ow, oh, oc = i32(P.OFF_OUTPUT_WIDTH)[0], i32(P.OFF_OUTPUT_HEIGHT)[0], i32(P.OFF_OUTPUT_COMPONENTS)[0]
        assert (ow, oh) == scaled_size(width, height, denom), (ow, oh, width, height, denom)
        assert oc == (1 if gray else ncomp)
        out = np.zeros((oh, ow * oc), dtype=np.uint8)
        row = (C.c_void_p * 1)()
        while i32(P.OFF_OUTPUT_SCANLINE)[0] < oh:
            row[0] = out.ctypes.data + i32(P.OFF_OUTPUT_SCANLINE)[0] * out.strides[0]
            assert lib.jpeg_read_scanlines(cinfo, row, 1) == 1
        lib.jpeg_finish_decompress(cinfo)
        lib.jpeg_destroy_decompress(cinfo)
        return out.reshape(oh, ow, oc)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------- the files
def tiny_files():
    """name -> bytes of the scaled/ set"""
    from PIL import Image
    import oracle
    from helpers import jpeg_from_coefficients as jc
    from helpers.sampling_goldens import PROG3
    from nvimagecodec_amd.synth import synth_image
    out = {}
    for w, h in TINY_SIZES:
        img = synth_image(w, h, seed=5000 + 100 * w + h)
        for sub in TINY_SUBS:
            for prog in (False, True):
                name = "t%dx%d_%s_%s" % (w, h, sub, "prog" if prog else "base")
                if sub == "440":
                    data = oracle.encode(img, "440", 90)
                    if prog:
                        coefs, qts = oracle.decode_coefficients(data)
                        data = jc.write_progressive(w, h, [(1, 2), (1, 1), (1, 1)], [c.astype(np.int32) for c in coefs],
                                                    [q.astype(np.int32) for q in qts], PROG3)
                else:
                    b = io.BytesIO()
                    if sub == "gray":
                        Image.fromarray(img).convert("L").save(b, "JPEG", quality=90, progressive=prog)
                    else:
                        Image.fromarray(img).save(b, "JPEG", quality=90, subsampling={"444": 0, "422": 1, "420": 2}[sub], progressive=prog)
                    data = b.getvalue()
                out[name] = data
    return out


def file_list():
    """[(set, name, sub or None, bytes)] in manifest order"""
    from helpers import sampling_goldens as G
    files = []
    for c in json.load(open(os.path.join(HERE, "manifest.json")))["decode"]:
        files.append(("decode", c["name"], c["sub"], open(os.path.join(HERE, "decode", c["name"] + ".jpg"), "rb").read()))
    for e in G.ENTRIES + G.REFUSED:
        files.append(("sampling", e["name"], None, G.jpeg(e)))
    for c in json.load(open(os.path.join(HERE, "manifest_gamut.json")))["gamut"]:
        files.append(("gamut", c["name"], None, open(os.path.join(HERE, "gamut", c["name"] + ".jpg"), "rb").read()))
    for name, data in tiny_files().items():
        files.append(("scaled", name, name.split("_")[1], data))
    return files


# ---------------------------------------------------------------------------------------------- worker child
def worker(first):
    """Decodes (file, denominator) pairs from number `first` on, one JSON line each; a refusal of the library ends the process behind
    the "begin" line of the pair."""
    dec = ScaledDecoder()
    k = 0
    for fset, name, sub, data in file_list():
        for denom in DENOMS:
            if k >= first:
                print(json.dumps({"begin": k}), flush=True)
                res = {"index": k}
                first_px = None
                for key, ifast, fancy in SETTINGS:
                    px = dec.decode_scaled(data, denom, ifast, fancy)
                    if key == "islow_fancy":
                        first_px = px
                        res["height"], res["width"], res["components"] = px.shape
                    res[key] = sha(np.repeat(px, 3, axis=2) if px.shape[2] == 1 else px)
                if fset == "scaled":
                    res["y"] = sha(dec.decode_scaled(data, denom, False, True, gray=True)[:, :, 0])
                print(json.dumps(res), flush=True)
            k += 1
    print(json.dumps({"done": k}), flush=True)


def run_workers(total):
    results, first = {}, 0
    while first < total:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(first)], capture_output=True, text=True, timeout=3600)
        begun = None
        done = False
        for line in p.stdout.splitlines():
            rec = json.loads(line)
            if "begin" in rec:
                begun = rec["begin"]
            elif "index" in rec:
                results[rec["index"]] = rec
                begun = None
            elif "done" in rec:
                done = True
        if done:
            break
        assert begun is not None, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
        results[begun] = {"index": begun, "refused": True, "libjpeg": p.stderr.strip().splitlines()[-1] if p.stderr.strip() else ""}
        first = begun + 1
    return results


def main():
    from PIL import Image, features
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    assert features.version_feature("libjpeg_turbo") == manifest["libjpeg_turbo"], "the goldens come from another library version"
    os.makedirs(os.path.join(HERE, "scaled"), exist_ok=True)
    files = file_list()
    for fset, name, sub, data in files:
        if fset == "scaled":
            with open(os.path.join(HERE, "scaled", name + ".jpg"), "wb") as f:
                f.write(data)
    results = run_workers(len(files) * len(DENOMS))
    entries = []
    fancy_422 = {d: 0 for d in DENOMS}
    ifast_420 = 0
    k = 0
    for fset, name, sub, data in files:
        e = {"set": fset, "name": name, "jpeg_sha256": hashlib.sha256(data).hexdigest(), "scales": {}}
        if sub:
            e["sub"] = sub
        for denom in DENOMS:
            r = results[k]
            k += 1
            if r.get("refused"):
                e["scales"][str(denom)] = {"refused": True, "libjpeg": r["libjpeg"]}
                continue
            s = {"width": r["width"], "height": r["height"]}
            if r["components"] == 4:
                e["components"] = 4
                s["cmyk_sha256"] = r["islow_fancy"]
            else:
                s["rgb_sha256"] = r["islow_fancy"]
            for key in ("islow_plain", "ifast_fancy", "ifast_plain"):
                if r[key] != r["islow_fancy"]:
                    s[key + "_sha256"] = r[key]
            if "y" in r:
                s["y_sha256"] = r["y"]
            if sub == "422":
                fancy_422[denom] += int(r["islow_plain"] != r["islow_fancy"])
            if sub == "420" and denom == 2:
                ifast_420 += int(r["ifast_fancy"] != r["islow_fancy"])
            if sub in ("444", "gray"):
                assert len({r[key] for key, _, _ in SETTINGS}) == 1, ("nothing to upsample and no full-size IDCT, yet a switch changed pixels", name, denom)
            e["scales"][str(denom)] = s
        entries.append(e)
    assert fancy_422[2] > 0 and fancy_422[4] > 0 and fancy_422[8] == 0, fancy_422  # the fancy switch reached the library
    assert ifast_420 > 0, ifast_420                                                # so did dct_method
    out = {"generator": "tests/golden/make_golden_scaled.py", "pillow": Image.__version__, "libjpeg_turbo": manifest["libjpeg_turbo"],
           "library": os.path.basename(P.library_path()), "files": entries}
    json.dump(out, open(os.path.join(HERE, "manifest_scaled.json"), "w"), indent=0, separators=(",", ":"))
    refused = sum(1 for e in entries for s in e["scales"].values() if s.get("refused"))
    print("wrote manifest_scaled.json:", len(entries), "files x", len(DENOMS), "denominators,", refused, "refused;", fancy_422, "4:2:2 files differ fancy/plain;",
          ifast_420, "4:2:0 files differ ISLOW/IFAST at 1/2")


if __name__ == "__main__":
    if "--probe" in sys.argv:
        P.probe_struct_size()
    elif "--worker" in sys.argv:
        worker(int(sys.argv[sys.argv.index("--worker") + 1]))
    else:
        main()
