"""Progressive (SOF2) files whose scans all have restart intervals, on the algorithm of the interval kernels
(csrc/progressive_interval_core.h: a lane per restart interval finds the block start positions and the DC values, then the replay of
csrc/progressive_gpu_core.h), run on the host by hipjpegEntropyDecodeGpuIntervalAlgorithmHost with the very code the kernels run.
Coefficients must be the oracle's; damaged streams must never be accepted where the host entropy decoder rejects them."""
import json
import os
import random

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_decode_case
from helpers import progressive_restart_files as P
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel

with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    _M = json.load(_f)
_RST = [e for e in _M["decode"] if e["progressive"] and "_rst" in e["name"]]


def _same_as_oracle(jpeg, what):
    ref, _ = oracle.decode_coefficients(jpeg)
    got = lowlevel.entropy_decode_gpu_interval_algorithm_host(jpeg)
    assert len(ref) == len(got)
    for c, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), (what, c)


def test_the_goldens_with_restart_markers():
    assert len(_RST) == 4
    for e in _RST:
        jpeg = load_decode_case(e)[0]
        _same_as_oracle(jpeg, e["name"])
        with pytest.raises(N.HipJpegError) as err:  # the walk's entry point keeps refusing them
            lowlevel.entropy_decode_gpu_algorithm_host(jpeg)
        assert err.value.status == 3  # UNSUPPORTED


def test_libjpeg_turbo_files_with_row_and_block_intervals():
    """Pillow: a marker every MCU row (the DRI then changes from scan to scan), every block, every 5 blocks; a flat picture with one
    textured patch gives end-of-band runs that the markers cut."""
    pytest.importorskip("PIL")
    files = P.pillow_files()
    assert len(files) == 27
    for name, jpeg in files:
        _same_as_oracle(jpeg, name)


def test_files_of_the_projects_own_progressive_coder():
    files = P.transcode_products(GOLDEN)
    assert len(files) == 12
    for name, jpeg in files:
        assert lowlevel.get_image_info(jpeg)["sof_marker"] == 0xC2, name
        _same_as_oracle(jpeg, name)


def test_files_without_restart_intervals_are_not_for_this_entry_point():
    for e in [e for e in _M["decode"] if "_rst" not in e["name"]][::9]:
        with pytest.raises(N.HipJpegError) as err:
            lowlevel.entropy_decode_gpu_interval_algorithm_host(load_decode_case(e)[0])
        assert err.value.status == 3, e["name"]


@pytest.mark.parametrize("name", sorted(P.HELPER_CASES))
def test_chosen_scripts_with_chosen_intervals(name):
    """Each file first pinned: the oracle and the host decoder give back the chosen coefficients.  Then the interval algorithm."""
    jpeg, coefs = P.helper_file(name)
    got, _ = oracle.decode_coefficients(jpeg)
    host, _ = lowlevel.entropy_decode_host(jpeg)
    emu = lowlevel.entropy_decode_gpu_interval_algorithm_host(jpeg)
    for c in range(len(coefs)):
        rows, cols = P.real_blocks(name, c)
        want = np.asarray(coefs[c])[:rows, :cols].astype(np.int16)
        assert np.array_equal(np.asarray(got[c])[:rows, :cols], want), ("oracle", c)
        assert np.array_equal(np.asarray(host[c])[:rows, :cols], want), ("host decoder", c)
        assert np.array_equal(np.asarray(emu[c])[:rows, :cols], want), ("interval algorithm on the host", c)
        assert np.array_equal(emu[c], got[c]), ("blocks of the MCU padding", c)


def test_the_helper_files_hold_end_of_band_runs_cut_by_markers():
    """What the cases are for: the helper's coder lets runs grow, so a marker has to close one somewhere (EOBn symbols in the file's AC
    table are used), and the gray case has more intervals than one workgroup of the kernels serves."""
    info = lowlevel.get_image_info(P.helper_file("gray_500_intervals")[0])
    assert info["blocks_w"][0] * info["blocks_h"][0] == 500 > 256
    jpeg, coefs = P.helper_file("bands_cut_anywhere")
    one_by_one = P.write_progressive_restart(83, 61, P.S444, coefs, [np.full(64, 3 + c, dtype=np.int32) for c in range(3)],
                                             P.HELPER_CASES["bands_cut_anywhere"][3], P.HELPER_CASES["bands_cut_anywhere"][4], max_run=1)
    assert len(jpeg) < len(one_by_one)
    _same_as_oracle(one_by_one, "runs of one block")


def test_ac_scans_of_a_component_with_different_intervals_stay_on_the_host():
    jpeg, coefs = P.helper_file(P.DIFFERENT_INTERVALS)
    with pytest.raises(N.HipJpegError) as err:
        lowlevel.entropy_decode_gpu_interval_algorithm_host(jpeg)
    assert err.value.status == 3  # UNSUPPORTED
    host, _ = lowlevel.entropy_decode_host(jpeg)
    ref, _ = oracle.decode_coefficients(jpeg)
    for c in range(3):
        rows, cols = P.real_blocks(P.DIFFERENT_INTERVALS, c)
        assert np.array_equal(host[c], ref[c])
        assert np.array_equal(np.asarray(host[c])[:rows, :cols], np.asarray(coefs[c])[:rows, :cols].astype(np.int16))


def test_interval_descriptors_have_no_sub_dword_members():
    """The interval kernels index ProgIntervalScan / ProgIntervalImage with wave-uniform run-time indices: like ProgScan / ProgImage
    (tests/test_code_object_hazards.py) they may hold 32- and 64-bit members only (pointers to smaller types are fine)."""
    import re
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "csrc", "progressive_interval_core.h")).read()
    for name in ("ProgIntervalScan", "ProgIntervalImage"):
        m = re.search(r"struct (?:alignas\(16\) )?%s \{(.*?)\n\};" % name, src, re.S)
        assert m, name
        decls = [line.split("//")[0].strip() for line in m.group(1).splitlines()]
        assert sum(1 for d in decls if d) >= 4
        for decl in decls:
            assert not re.match(r"(u?int8_t|u?int16_t|bool|char)\s+[a-z_]", decl), (name, decl)


def test_damaged_streams_get_the_host_verdict():
    """The recipe of test_damaged_progressive_streams_get_the_host_verdict (a bit flip or a random byte somewhere behind the first SOS),
    2000 seeded trials on the four goldens: the interval algorithm must never accept a stream the host decoder rejects, and must agree
    with it on the coefficients where both accept.  At most half of the trials may be lost to damage that hits a header or makes the
    file ineligible (in the rst1 goldens a third of the scan bytes are markers; the rst7 ones have few)."""
    cases = [load_decode_case(e)[0] for e in _RST]
    rng = random.Random(777)
    trials, skipped, both, host_only, neither = 2000, 0, 0, 0, 0
    for _ in range(trials):
        j = bytearray(rng.choice(cases))
        first_sos = j.find(b"\xff\xda")
        k = rng.randrange(first_sos + 14, len(j) - 2)
        if rng.randrange(2):
            j[k] ^= 1 << rng.randrange(8)
        else:
            j[k] = rng.randrange(256)
        j = bytes(j)

        def run(fn):
            try:
                r = fn(j)
                return 0, r[0] if isinstance(r, tuple) else r
            except N.HipJpegError as e:
                return e.status, None
        sg, cg = run(lowlevel.entropy_decode_gpu_interval_algorithm_host)
        if sg in (2, 3):
            skipped += 1
            continue  # the damage hit a marker segment or made the stream ineligible: host entropy stage only
        sh, ch = run(lowlevel.entropy_decode_host)
        if sh == 0 and sg == 0:
            both += 1
            assert all(np.array_equal(a[: b.shape[0]], b) for a, b in zip(cg, ch)), j.hex()
        else:
            # a stream the kernels reject goes to the host decoder, which names the error -- what must never happen is the kernels
            # accepting what the host decoder rejects
            assert not (sg == 0 and sh != 0), (sh, sg, j.hex())
            host_only += sh == 0
            neither += sh != 0
    print("damaged streams: %d trials, %d ineligible or header-level, %d accepted by both, %d by the host decoder alone, %d by neither"
          % (trials, skipped, both, host_only, neither))
    assert skipped <= trials // 2
    assert both >= 1
