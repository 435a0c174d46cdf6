"""The fast integer IDCT (JDCT_IFAST, decoder option fast_idct) on the CPU: the numpy restatement of tests/helpers/ifast_idct.py against the
hashes tests/golden/make_golden_fast_idct.py took from the real libjpeg-turbo -- the SIMD routine (what the kernels restate) on every gray
decode golden and every gray out-of-gamut vector, the C routine on the JSIMD_FORCENONE=1 hashes, and the CMYK samples."""
import glob
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import ifast_idct

with open(os.path.join(GOLDEN, "manifest_fast_idct.json")) as _f:
    _M = json.load(_f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _read(*parts):
    with open(os.path.join(GOLDEN, *parts), "rb") as f:
        return f.read()


def test_manifest_covers_the_goldens():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        names = [e["name"] for e in json.load(f)["decode"]]
    assert [e["name"] for e in _M["decode"]] == names
    assert len(_M["gamut"]) == 43 and len(_M["cmyk"]) == 54 and len(_M["roi"]) > 100
    # IFAST is not ISLOW: the manifest's pixels differ from the default goldens on every kind of file
    assert all(v > 0 for v in _M["files_that_differ_from_islow"].values())


def test_multiplier_table():
    # jddctmgr.c: aanscales = 16384 * s[row] * s[col], s[k] = cos(k pi / 16) sqrt(2)
    s = np.array([1.0] + [np.cos(k * np.pi / 16) * np.sqrt(2) for k in range(1, 8)])
    assert np.array_equal(ifast_idct.AANSCALES, np.rint(16384 * np.outer(s, s)).astype(np.int64).ravel())
    assert ifast_idct.multiplier_table(np.full(64, 16))[0] == 64
    # a 16-bit table: the library stores the multipliers as int16, the large ones wrap
    assert ifast_idct.multiplier_table(np.full(64, 65535))[9] == ((65535 * 31521 + 2048) >> 12) - 65536 * 8


@pytest.mark.parametrize("entry", [e for e in _M["decode"] if e["sub"] == "gray"], ids=lambda e: e["name"])
def test_simd_restatement_on_gray_goldens(entry):
    plane = ifast_idct.planes(_read("decode", entry["name"] + ".jpg"))[0]
    assert _sha(np.repeat(plane[:, :, None], 3, axis=2)) == entry["rgb_sha256"]


@pytest.mark.parametrize("entry", [e for e in _M["gamut"] if e["mode"] == "L"], ids=lambda e: e["name"])
def test_simd_and_c_restatements_on_gray_gamut_vectors(entry):
    jpeg = _read("gamut", entry["name"] + ".jpg")
    assert _sha(ifast_idct.planes(jpeg)[0]) == entry["simd_sha256"]
    assert _sha(ifast_idct.planes(jpeg, c_routine=True)[0]) == entry["c_sha256"]


def test_the_gamut_vectors_tell_the_routines_apart():
    assert sum(not e["simd_equals_c"] for e in _M["gamut"]) >= 40


@pytest.mark.parametrize("entry", _M["cmyk"], ids=lambda e: e["name"])
def test_cmyk_samples(entry):
    assert _sha(ifast_idct.cmyk_samples(_read("cmyk", entry["name"] + ".jpg"))) == entry["cmyk_sha256"]


def _live_library():
    try:
        from PIL import features
        import PIL
    except ImportError:
        return False
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        version = json.load(f)["libjpeg_turbo"]
    libs = glob.glob(os.path.join(os.path.dirname(PIL.__file__), "..", "pillow.libs", "libjpeg-*.so.62*"))
    return len(libs) == 1 and features.version_feature("libjpeg_turbo") == version


@pytest.mark.skipif(not _live_library(), reason="the libjpeg-turbo the goldens come from is not importable here")
def test_manifest_regenerates_byte_identically(tmp_path):
    out = tmp_path / "manifest_fast_idct.json"
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_fast_idct.py"), "--out", str(out)], check=True, timeout=900,
                   capture_output=True)
    assert out.read_bytes() == open(os.path.join(GOLDEN, "manifest_fast_idct.json"), "rb").read()
