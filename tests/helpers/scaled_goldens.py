"""The scaled-decode goldens (tests/golden/manifest_scaled.json, made by tests/golden/make_golden_scaled.py from libjpeg-turbo itself): the
files, and which hash a (denominator, dct_method, fancy upsampling) setting must produce.  The manifest stores the hashes of the settings
other than (ISLOW, fancy) only where they differ from that one."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
DENOMS = (2, 4, 8)
SUCCESS, INVALID_ARGUMENT, UNSUPPORTED = 0, 1, 3

with open(os.path.join(GOLDEN, "manifest_scaled.json")) as _f:
    MANIFEST = json.load(_f)
FILES = MANIFEST["files"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def jpeg(entry):
    """the bytes of a manifest entry (the sampling-layout files are rebuilt, the others read); they are the ones the library decoded"""
    if entry["set"] == "sampling":
        from helpers import sampling_goldens as G
        data = G._jpeg(entry["name"])
    else:
        with open(os.path.join(GOLDEN, entry["set"], entry["name"] + ".jpg"), "rb") as f:
            data = f.read()
    assert hashlib.sha256(data).hexdigest() == entry["jpeg_sha256"], entry["name"]
    return data


def expected(entry, denom, ifast=False, fancy=True):
    """-> (status, sha256 of the H x W x 3 RGB pixels or None).  The library's refusals and four-component frames are UNSUPPORTED."""
    s = entry["scales"][str(denom)]
    if s.get("refused") or entry.get("components") == 4:
        return UNSUPPORTED, None
    key = {(False, True): "rgb_sha256", (False, False): "islow_plain_sha256", (True, True): "ifast_fancy_sha256", (True, False): "ifast_plain_sha256"}[
        (bool(ifast), bool(fancy))]
    return SUCCESS, s.get(key, s["rgb_sha256"])


def by_name(name):
    return next(e for e in FILES if e["name"] == name)
