#!/usr/bin/env python3
"""libjpeg-turbo's hashes for the sampling-layout goldens (tests/helpers/sampling_goldens.py), via Pillow.  Dev-container only.

Per file: the sha256 of its bytes, of what libjpeg-turbo gives with fancy upsampling on (RGB H x W x 3, gray H x W, four components
H x W x 4 = 255 - Pillow's inverted CMYK as in make_golden_cmyk.py) and of the same decode with do_fancy_upsampling = FALSE (the ctypes
binding of make_golden_plain_upsampling.py); for the layouts libjpeg refuses, its message.  Output: manifest_sampling.json, one entry
per line."""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
from helpers import sampling_goldens as G  # noqa: E402
from make_golden_plain_upsampling import Decoder  # noqa: E402


def pillow_pixels(jpeg, ncomp):
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    a = np.asarray(im)
    return 255 - a if ncomp == 4 else a


def main():
    assert features.check_feature("libjpeg_turbo")
    plain_decoder = Decoder()
    entries, refused, differ = [], [], 0
    for case in G.CASES:
        jpeg, n = G.build(case), len(case["sampling"])
        pix = pillow_pixels(jpeg, n)
        assert pix.shape[:2] == (case["height"], case["width"]), case["name"]
        fancy = plain_decoder.decode(jpeg, True)
        assert np.array_equal(fancy[:, :, 0] if n == 1 else fancy, pix), ("the binding is not Pillow", case["name"])
        plain = plain_decoder.decode(jpeg, False)
        plain = plain[:, :, 0] if n == 1 else plain
        differ += int(not np.array_equal(plain, pix))
        # the oracle is what the GPU tests compare with: it must be the library here
        ref = oracle.decode_cmyk(jpeg) if n == 4 else oracle.decode(jpeg, oracle.FMT_GRAY if n == 1 else oracle.FMT_RGB)
        assert np.array_equal(ref, pix), case["name"]
        entries.append(dict(name=case["name"], jpeg_sha256=hashlib.sha256(jpeg).hexdigest(), sha256=G.sha(pix), plain_sha256=G.sha(plain)))
    assert differ >= 35, differ  # the switch reached the library
    for case in G.REFUSED_CASES:
        jpeg = G.build(case)
        try:
            pillow_pixels(jpeg, 3)
            raise AssertionError("libjpeg decoded " + case["name"])
        except OSError as e:
            refused.append(dict(name=case["name"], jpeg_sha256=hashlib.sha256(jpeg).hexdigest(), libjpeg=str(e)))
    head = {"generator": "tests/golden/make_golden_sampling.py", "pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"),
            "subsampled_files_that_differ_from_fancy": differ}
    with open(G.MANIFEST_PATH, "w") as f:
        f.write(json.dumps(head)[:-1] + ',\n "sampling": [\n' + ",\n".join("  " + json.dumps(e) for e in entries) + '\n ],\n "refused": [\n'
                + ",\n".join("  " + json.dumps(e) for e in refused) + "\n ]\n}\n")
    print(len(entries), "sampling vectors,", differ, "differ without fancy upsampling;", len(refused), "refused layouts")


if __name__ == "__main__":
    main()
