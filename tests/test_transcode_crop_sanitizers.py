"""AddressSanitizer + UBSan over the crop, drop-chroma and copy-markers steps of the lossless transcode on the host (CPU build only, a
stand-alone program, never through Python): hipjpegTranscodeHostRegion with random regions and flag sets over the goldens, copies of them
with EXIF / ICC-sized / COM segments spliced in, and mutated copies -- the segment collector and the EXIF patch read lengths and offsets
that the file controls.  The harness (tests/sanitizers/transcode_crop_fuzz.cpp) also checks that every file that comes out parses and
that an unturned one carries the source's blocks from the crop's origin."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_crop_and_markers_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "transcode_crop_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "transcode_crop_fuzz.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "entropy_decode.cpp", "entropy_encode.cpp", "transcode_core.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    seeds = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg"))) if os.path.getsize(p) < 40000]
    seeds += sorted(glob.glob(os.path.join(GOLDEN, "gamut", "*.jpg")))[:6]
    assert len(seeds) > 100
    run = subprocess.run([exe, "1500", "20261018"] + seeds, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert " 0 wrong results" in run.stdout
    files = int(run.stdout.split("calls,")[1].split("files")[0])
    with_markers = int(run.stdout.split("checked (")[1].split("with markers")[0])
    assert files > 800 and with_markers > 500  # the requests are not all refused
