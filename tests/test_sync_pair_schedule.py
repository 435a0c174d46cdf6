"""The first sync launch's paired schedule (huff_sync_pair_kernel, csrc/gpu_huffman.hip) on the host twin, WITHOUT a GPU.  The twin
(csrc/gpu_huffman_host.cpp emulate_sync_launch) runs the schedule of the kernel's workgroups -- two sync units each: even rows from
the assumed state, odd rows from their neighbour's end state with records, correction rounds of alternating parity to the
workgroup's fixpoint, then the seams as the tail and ripple launches settle them -- and the one-unit schedule it replaced, and
compares each with the image-wide Jacobi iteration: the same end state and the same block-start record for every subsequence, or
INTERNAL_ERROR.  hipjpegTestSyncScheduleCounts reports what each schedule decodes before the tail kernel and what it leaves to it."""
import io
import json
import os

import pytest

from conftest import GOLDEN, load_decode_case
from helpers import steered_streams as S
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel
from nvimagecodec_amd.synth import synth_image

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _M = json.load(_f)

UNSUPPORTED = 3


def counts(jpeg):
    """both schedules' counts; raises on every status, INTERNAL_ERROR (the schedules disagree with Jacobi) included"""
    c = lowlevel.sync_schedule_counts(jpeg)
    for name in ("single", "paired"):
        assert len(c[name]["phases"]) == 4 and c[name]["phases"][0] + c[name]["phases"][1] >= 1, name   # (one subsequence: phase B alone)
    assert c["single"]["phases"][1] == 0      # (no phase B)
    return c


def test_every_eligible_golden():
    ran = 0
    for entry in _M["decode"]:
        jpeg, _ = load_decode_case(entry)
        try:
            counts(jpeg)
        except N.HipJpegError as e:
            assert e.status == UNSUPPORTED and entry["progressive"], entry["name"]   # the sequential goldens all run
            continue
        ran += 1
    assert ran >= 1 and ran == sum(1 for e in _M["decode"] if not e["progressive"])


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_steered_families(name):
    """Placed bytes on the destuff seams, restart markers (no records), stream ends around a sync unit and two, records at their
    30-slot edge, blocks longer than a subsequence."""
    for k, w in enumerate(S.family(name)):
        c = counts(w.jpeg)
        if w.ri:
            continue
        nsub = -(-w.dbits // 1024)
        # with records round 1 decodes every owned row: all subsequences (one unit), every second one (pairs)
        assert c["single"]["phases"][2] == nsub and c["paired"]["phases"][1] + c["paired"]["phases"][2] == nsub, (name, k)


def test_block_pass_streams():
    """Every stream tests/test_block_pass_streams.py hands to its check_good()."""
    import test_block_pass_streams as T
    got, keep = [], T.check_good
    T.check_good = got.append
    try:
        T.test_eob_behind_short_symbols()
        T.test_zrl_runs()
        for lead in T.test_all_coefficients_present_no_eob.pytestmark[0].args[1]:
            T.test_all_coefficients_present_no_eob(lead)
        T.test_sixteen_bit_code_behind_a_short_one()
        T.test_last_symbols_at_the_end_of_the_stream()
    finally:
        T.check_good = keep
    assert len(got) > 35
    for blocks in got:
        counts(S.gray_file(blocks))


def test_a_1080p_photograph_walks_and_hands_over_less():
    """The arithmetic the paired schedule rests on, with the workgroups' halos counted: at most 0.75 of the one-unit schedule's
    decodes before the tail kernel (the image-wide model reads 0.71: tools/sync_schedule_model.py), at most 0.65 of its tasks for the
    tail kernel's first round (the model: 0.53)."""
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(synth_image(1920, 1080, seed=1234)).save(b, "JPEG", quality=90, subsampling=2)
    c = counts(b.getvalue())
    single, paired = c["single"], c["paired"]
    before_tail = sum(paired["phases"]) / sum(single["phases"])
    handed_over = paired["tail"] / single["tail"]
    print("decodes before the tail: paired %s = %d, one unit %s = %d, ratio %.3f; tasks for the tail: %d against %d, ratio %.3f" % (
        paired["phases"], sum(paired["phases"]), single["phases"], sum(single["phases"]), before_tail, paired["tail"], single["tail"], handed_over))
    # A and B are half of the rows each, round 1 the even rows but the halos
    groups = -(-single["phases"][2] // (2 * 255))     # (round 1 of the one-unit schedule decodes every subsequence once)
    assert abs(paired["phases"][0] - paired["phases"][1]) <= groups and paired["phases"][2] <= paired["phases"][0]
    assert before_tail <= 0.75
    assert handed_over <= 0.65
