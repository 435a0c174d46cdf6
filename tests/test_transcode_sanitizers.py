"""AddressSanitizer + UBSan over the host side of the lossless transcode (CPU build only, a stand-alone program, never through
Python): hipjpegTranscodeHost -- eligibility rules, relayout, range guard -- between the host entropy decoder and the host coder, fed
with the goldens (the crafted out-of-gamut ones included) and thousands of mutated copies.  The harness
(tests/sanitizers/transcode_fuzz.cpp) also checks that every file that comes out holds the coefficients and tables of its source."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_transcode_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "transcode_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "transcode_fuzz.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "entropy_decode.cpp", "entropy_encode.cpp", "transcode_core.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    seeds = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg"))) if os.path.getsize(p) < 40000]
    seeds += sorted(glob.glob(os.path.join(GOLDEN, "gamut", "*.jpg"))) + sorted(glob.glob(os.path.join(GOLDEN, "cmyk", "*.jpg")))[:4]
    assert len(seeds) > 100
    run = subprocess.run([exe, "3000", "20261018"] + seeds, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert " 0 wrong results" in run.stdout
    files = int(run.stdout.split("calls,")[1].split("files")[0])
    assert files > 1500  # the mutations are not all refused
