"""ASan / UBSan over the host rules of the coefficient <-> pixel calls (hipjpegGetEncodeCoefficientInfo, the info -> frame builder
coefficient_frame): a stand-alone program (tests/sanitizers/coefficient_pixels_host.cpp), never through Python."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_rules_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "coefficient_pixels_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "coefficient_pixels_host.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "entropy_decode.cpp", "entropy_encode.cpp", "transcode_core.cpp", "coefficients_core.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    files = [os.path.join(GOLDEN, "decode", n + ".jpg") for n in ("s1x1_gray_base_q90", "s3x5_420_base_q90", "s17x13_420_prog_q50", "s33x65_422_base_q90",
                                                                  "h320x200_420_opt_q75", "c1_640x480_444_base_q90")]
    files += sorted(glob.glob(os.path.join(GOLDEN, "cmyk", "*.jpg")))[:1]
    assert all(os.path.exists(f) for f in files) and len(files) == 7
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 13 sizes x 10 subsampling values x 7 qualities; 9 legal sizes x 7 known subsamplings x 7 qualities + 6 files
    assert run.stdout.startswith("910 infos, 447 frames, "), run.stdout
    assert run.stdout.rstrip().endswith(" 0 wrong results"), run.stdout
