"""AddressSanitizer + UBSan over the host side of the lossless decoder (CPU build only, a stand-alone program, never through Python):
the SOF3 path of the parser, the entropy stage, the plain reconstruction and both kernel schedules, fed with the goldens and thousands
of damaged copies.  The harness (tests/sanitizers/lossless_fuzz.cpp) also checks that the three reconstructions agree on every file."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_lossless_decode_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lossless_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "lossless_fuzz.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "lossless_entropy.cpp", "lossless_core.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    seeds = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "lossless", "*.jpg"))) if not os.path.basename(p).startswith("refused")]
    assert len(seeds) > 150
    run = subprocess.run([exe, "4000", "20261020"] + seeds, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert " 0 wrong results" in run.stdout
    decoded = int(run.stdout.split("calls,")[1].split("files")[0])
    reached = int(run.stdout.split("decoded,")[1].split("damaged")[0])
    # the damage is not all caught by the parser: a quarter of the copies get as far as the entropy stage, and some decode to the end
    assert reached > 1000 and decoded > len(seeds) + 100, run.stdout
