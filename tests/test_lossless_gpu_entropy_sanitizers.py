"""AddressSanitizer + UBSan over the host twin of the lossless decoder's GPU entropy stage (CPU build only, a stand-alone program, never
through Python): hipjpegLosslessEntropyAlgorithmHost runs the kernels' schedule and the code they share with it (lossless_gpu_core.h)
over goldens, over the files that sit on the schedule's seams and over the damaged ones.  The driver
(tests/sanitizers/lossless_gpu_entropy_check.cpp) also checks every result against the host stage."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN
from helpers import lossless_entropy_cases as EC
from nvimagecodec_amd import lowlevel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_entropy_twin_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lossless_gpu_entropy_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "lossless_gpu_entropy_check.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "lossless_entropy.cpp", "lossless_core.cpp", "lossless_gpu_host.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    goldens = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "lossless", "*.jpg"))) if not os.path.basename(p).startswith("refused")]
    goldens = goldens[::max(1, len(goldens) // 16)]
    assert len(goldens) >= 12
    shape = lowlevel.lossless_entropy_shape()
    crafted = [f for _, f, _, _ in EC.seam_cases(shape)] + [EC.unsynchronisable(shape)[0]]
    bad = [f for _, f in EC.bad_cases()]
    paths = []
    for k, f in enumerate(crafted + bad):
        p = tmp_path / f"case{k}.jpg"
        p.write_bytes(f)
        paths.append(str(p))
    run = subprocess.run([exe] + goldens + paths, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert " 0 wrong results" in run.stdout, run.stdout
    unconverged = int(run.stdout.split("refused,")[1].split("unconverged")[0])
    assert 1 <= unconverged <= 1 + len(bad), run.stdout  # the file that cannot synchronise; a damaged file's walk need not converge either
    decoded = int(run.stdout.split("files,")[1].split("decoded")[0])
    assert decoded >= len(goldens) + len(crafted), run.stdout  # (some damaged files decode too: the host stage does not miss what they lack)
