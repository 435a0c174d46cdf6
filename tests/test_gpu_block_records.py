"""GPU: the position pass copies the block-start records of the synchronisation decodes and walks only the subsequences without a
usable one (csrc/gpu_huffman.hip huff_pos_kernel).  A mixed batch -- photographs, overflowing and periodic pictures, damaged and
restart-interval streams -- must decode bit for bit as through the host entropy stage and the oracle, under the default settings
and under every switch that changes which kernel takes the last decode of a subsequence."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "decode_record_mix.py")


@pytest.mark.parametrize("switches", [{}, {"HIPJPEG_POSITION_PASS": "1"}, {"HIPJPEG_TAIL_AFTER": "1"}, {"HIPJPEG_TAIL_AFTER": "3"},
                                      {"HIPJPEG_TAIL_AFTER": "0"}, {"HIPJPEG_FUSED_DECODE": "1"}, {"HIPJPEG_RIPPLE_IN_SYNC": "1"}],
                         ids=["default", "position_pass", "tail_after_1", "tail_after_3", "no_tail", "fused_decode", "ripple_in_sync"])
def test_mixed_batch_under_switch(switches):
    env = dict(os.environ)
    env.update(switches)
    r = subprocess.run([sys.executable, HELPER], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "records ok" in r.stdout
