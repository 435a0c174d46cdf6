"""AddressSanitizer + UBSan over the host side of the lossless coder (CPU build only, a stand-alone program, never through Python): the
plain host coder and the kernels' schedule run on the host, over the goldens and the seam list, each plane in an allocation of exactly
the bytes the input promises.  The harness (tests/sanitizers/lossless_encode_check.cpp) compares every file with the expected bytes."""
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_encode_model as M
from helpers import lossless_encode_seams as S
from nvimagecodec_amd import lowlevel as LL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nvimagecodec_amd", "csrc")


def _record(samples, want, P, ps, pt, rr, planar, pad, offset):
    s = np.ascontiguousarray(M.as_hwn(samples))
    h, w, n = s.shape
    return struct.pack("<11iI", P, ps, pt, rr, n, w, h, s.itemsize, int(planar), pad, offset, len(want)) + s.tobytes() + want


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_lossless_encode_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lossless_encode_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + SRC, os.path.join(ROOT, "tests", "sanitizers", "lossless_encode_check.cpp")]
    cmd += [os.path.join(SRC, f) for f in ("jpeg_syntax.cpp", "entropy_encode.cpp", "lossless_encode_host.cpp")]
    build = subprocess.run(cmd + ["-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("no sanitizer runtime in this toolchain")
    assert build.returncode == 0, build.stderr[-2000:]
    records = []
    for i, e in enumerate(json.load(open(os.path.join(GOLDEN, "manifest_lossless_encode.json")))["lossless_encode"]):
        s = M.case_samples(e)
        want = M.model_file(s, e["precision"], e["predictor"], e["point_transform"], e["restart_rows"])
        assert hashlib.sha256(want).hexdigest() == e["sha256"], e["name"]
        records.append(_record(s, want, e["precision"], e["predictor"], e["point_transform"], e["restart_rows"], i % 2, i % 16, (5 * i) % 16))
    shape = LL.lossless_encode_shape()
    for c in S.cases(shape) + S.searched_cases(shape):
        want = M.model_file(c["samples"], c["precision"], c["predictor"], c["point_transform"], c["restart_rows"])
        records.append(_record(c["samples"], want, c["precision"], c["predictor"], c["point_transform"], c["restart_rows"], c["planar"], c["pad"],
                               c["offset"]))
    path = str(tmp_path / "cases.bin")
    open(path, "wb").write(b"".join(records))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "%d cases, 0 wrong results" % len(records) in run.stdout
