#!/usr/bin/env python3
"""Encode goldens at the edges of the 8-bit range and of the quality scale: the REAL libjpeg-turbo's baseline files (via Pillow, standard
Huffman tables) for the saturated pictures of tests/helpers/extreme_images.py at qualities 1, 75 and 100, and the quantization tables
libjpeg-turbo writes for every quality.

Dev-container only (needs Pillow built against libjpeg-turbo).  Outputs (all data, no code):
  encode_extreme/<pattern>_<w>x<h>.rgb               input pixels, once per input
  encode_extreme/<pattern>_<w>x<h>_<sub>_q<q>.jpg    libjpeg-turbo's baseline encoding (gray: of Pillow's "L" conversion of the input,
                                                     which is jccolor.c's luma)
  manifest_encode_extreme.json                       parameters + sha256
  quant_tables_q1_100.json                           luma / chroma tables of qualities 1..100, natural (row-major) order
Run:  python tests/golden/make_golden_encode_extreme.py     (twice gives the same bytes)
"""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import pil_encode, sha  # noqa: E402
from tests.helpers.extreme_images import PATTERNS, extreme_image  # noqa: E402

SIZES = ((8, 8), (17, 13), (40, 24))
SUBS = ("444", "422", "420", "gray")
QUALITIES = (1, 75, 100)


def seed_of(width, height):
    return 7000 + 100 * width + height


def pil_tables(quality):
    """(luma, chroma) as Pillow reads them back from a file it wrote: lists of 64 in natural order"""
    b = io.BytesIO()
    Image.new("RGB", (8, 8)).save(b, "JPEG", quality=quality)
    q = Image.open(io.BytesIO(b.getvalue())).quantization
    return [int(v) for v in q[0]], [int(v) for v in q[1]]


def main():
    assert features.check_feature("libjpeg_turbo"), "Pillow must be built against libjpeg-turbo"
    out = os.path.join(HERE, "encode_extreme")
    os.makedirs(out, exist_ok=True)
    entries = []
    for (w, h) in SIZES:
        for pattern in PATTERNS:
            img = extreme_image(pattern, w, h, seed_of(w, h))
            stem = f"{pattern}_{w}x{h}"
            with open(os.path.join(out, stem + ".rgb"), "wb") as f:
                f.write(img.tobytes())
            for sub in SUBS:
                for q in QUALITIES:
                    jpeg = pil_encode(img, q, sub)
                    name = f"{stem}_{sub}_q{q}"
                    with open(os.path.join(out, name + ".jpg"), "wb") as f:
                        f.write(jpeg)
                    entries.append(dict(name=name, input=stem + ".rgb", pattern=pattern, width=w, height=h, seed=seed_of(w, h), sub=sub, quality=q,
                                        rgb_sha256=sha(img), jpeg_sha256=hashlib.sha256(jpeg).hexdigest()))
    with open(os.path.join(HERE, "manifest_encode_extreme.json"), "w") as f:
        json.dump(dict(generator="tests/golden/make_golden_encode_extreme.py", pillow=Image.__version__,
                       libjpeg_turbo=features.version_feature("libjpeg_turbo"), encode_extreme=entries), f, indent=1)
    tables = {}
    for q in range(1, 101):
        luma, chroma = pil_tables(q)
        tables[str(q)] = dict(luma=luma, chroma=chroma)
    with open(os.path.join(HERE, "quant_tables_q1_100.json"), "w") as f:
        json.dump(dict(generator="tests/golden/make_golden_encode_extreme.py", pillow=Image.__version__,
                       libjpeg_turbo=features.version_feature("libjpeg_turbo"), order="natural (row-major)", tables=tables), f, separators=(",", ":"))
    total = sum(os.path.getsize(os.path.join(out, fn)) for fn in os.listdir(out))
    print(f"{len(entries)} extreme encode vectors, {total / 1e3:.0f} kB under encode_extreme/")


if __name__ == "__main__":
    main()
