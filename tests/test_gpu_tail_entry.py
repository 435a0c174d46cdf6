"""The first tail launch of the GPU entropy stage (huff_tail_kernel<false>, csrc/gpu_huffman.hip) enters a group of 255 subsequences
with the state that lies in front of it when the wave gets there, not with the guess pass 0 made: where the two differ the group's
first subsequence joins the first round as one more chain, and a group whose lists run empty looks in front once more before it
leaves.  What is read depends on timing; incoming[] records what was used and the ripple launch behind compares it with the final
value, so pixels must not.  Every case decodes through gpu_huffman=True as one batch and compares with the oracle bit for bit.

A group is 255 x 128 = 32,640 bytes of destuffed scan, a tail workgroup takes four consecutive groups (units): the inputs are
pictures of one to a few groups.  The crafted one-component files (helpers/steered_streams.py) take about ten seconds to write,
once per process; the switch cases get the finished batch through a file."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)

import oracle
from helpers import sequential_scans as Q
from helpers import steered_streams as S
from nvimagecodec_amd.synth import synth_image

GROUP = S.WG_BYTES          # destuffed bytes of one group
TAIL_WAVES = 4              # groups per tail workgroup (kTailWaves)

# "launch 2: N rounds in total" of resolve()'s HIPJPEG_DEBUG_TIMING line for rounds_batch() (16 x 1080p q90, 240 groups): the rounds
# all groups of the ripple launch spent together.  The parent commit (the tail launch entering with pass 0's guess) printed 235 in
# each of eight runs of this file's child on an MI355X; in the same visit the tree printed 2 in each of seven, and 18 without the
# second look (profiles/tail_entry/README.md).  The bound is half the parent's figure, as the change was specified; it is not taken
# from the tree's own.
PARENT_RIPPLE_ROUNDS = 235
RIPPLE_ROUNDS_BOUND = PARENT_RIPPLE_ROUNDS // 2


def _scan_bytes(jpeg):
    """(raw, destuffed) length of the single scan of a baseline file without restart markers"""
    sos = jpeg.rfind(b"\xff\xda")
    scan = jpeg[sos + 2 + int.from_bytes(jpeg[sos + 2:sos + 4], "big"):-2]
    return len(scan), len(scan) - scan.count(b"\xff\x00")


def _units(raw):
    """sync units the planner lays out for a scan: from its raw length (the destuffed one is known on the device only)"""
    return max(1, -(-(-(-raw * 8 // 1024)) // 255))


def _groups(destuffed):
    return max(1, -(-destuffed // GROUP))


PHOTOS = ((320, 240, "420", 90, 3), (448, 336, "420", 95, 4), (400, 300, "444", 90, 4), (640, 480, "420", 90, 5), (480, 360, "444", 90, 6),
          (472, 354, "444", 95, 8), (640, 480, "420", 95, 7))


@functools.lru_cache(maxsize=None)
def seam_batch():
    """[(file, raw scan bytes, destuffed scan bytes)] in batch order, and the oracle's pixels"""
    crafted = []
    for n in (1, 2, 3, 5):
        for d in (-128, -1, 0, 1, 128):
            w = S.Steered(64, 31000 + 10 * n + d)
            w.ff_at(300 + (n * 7 + d) % 50)
            w.finish(dbytes=n * GROUP + d)
            assert w.dbits == 8 * (n * GROUP + d)
            crafted.append((w.jpeg, len(w.scan), w.dbits // 8))
    photos = []
    for (wd, ht, sub, q, seed) in PHOTOS:
        j = oracle.encode(synth_image(wd, ht, seed=seed), sub, q)
        photos.append((j,) + _scan_bytes(j))
    assert {_groups(d) for _, _, d in photos} >= {1, 2, 3, 5}
    # a photograph after every third crafted file: the unit counts 1, 2, 3, 4, 5 and 6 mix, and so do the first groups' places
    files = []
    for k, c in enumerate(crafted):
        files.append(c)
        if k % 3 == 2:
            files.append(photos[(k // 3) % len(photos)])
    files.append(photos[-1])
    refs = [oracle.decode(j) for j, _, _ in files]
    return files, refs


def first_group_places(files):
    """the wave (unit index mod 4) that gets the first group of every file of the batch"""
    places, unit = [], 0
    for _, raw, _ in files:
        places.append(unit % TAIL_WAVES)
        unit += _units(raw)
    return places


def test_the_batch_puts_first_groups_at_every_wave_and_has_forty_others():
    """(no device needed, but the file is marked gpu as a whole: the batch is what the device cases decode)"""
    files, _ = seam_batch()
    assert set(first_group_places(files)) == {0, 1, 2, 3}
    # groups that are not an image's first: each is entered with a guess that is right two times in three
    assert sum(_groups(d) - 1 for _, _, d in files) >= 40


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


def _decode_exact(dec, jpegs, refs, on_gpu=True):
    import torch
    outs, st = dec.decode(jpegs, fmt="rgb", gpu_huffman=True, check=False)
    torch.cuda.synchronize()
    assert all(s == 0 for s in st), list(st)
    for k, (o, r) in enumerate(zip(outs, refs)):
        got = o.cpu().numpy()
        assert np.array_equal(got, r), "file %d of the batch: first differing pixel %s" % (k, tuple(np.argwhere(got != r)[0]))
    stats = dec.stats()
    if on_gpu:
        assert stats["gpu_entropy_images"] == len(jpegs)
        assert dec.host_fallbacks() == 0
    return stats


def test_group_seams(dec):
    files, refs = seam_batch()
    for _ in range(3):      # (what the tail launch reads depends on timing: the batch more than once)
        _decode_exact(dec, [j for j, _, _ in files], refs)


@functools.lru_cache(maxsize=None)
def noise_batch():
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    jpegs = [oracle.encode(noise, "420", 98), oracle.encode(noise, "444", 98)]
    return jpegs, [oracle.decode(j) for j in jpegs]


# what the parent commit reports for noise_batch() (read once, on an MI355X): the launch queued with the batch and the ripple
# launch behind it, no further one
PARENT_NOISE_SYNC_LAUNCHES = 2


def test_long_chains_stay_on_the_gpu(dec):
    """Noise at q98: about 125 rounds in the tail launch and 40 in the ripple launch, inside the budget of 192 -- also with the
    chains the new entry adds to the first of them."""
    jpegs, refs = noise_batch()
    assert all(_groups(_scan_bytes(j)[1]) >= 12 for j in jpegs)
    stats = _decode_exact(dec, jpegs, refs)
    assert stats["sync_launches"] == PARENT_NOISE_SYNC_LAUNCHES


def test_periodic_streams_still_run_out_of_rounds(dec):
    """The batch of test_gpu_huffman.py's periodic case at a quarter of its size.  A chain on a periodic stream never meets the true
    trajectory; looking in front again must not hand it a fresh budget: the striped picture is given up after 192 subsequences and
    goes to the host decoder, the flat picture and the photograph stay."""
    import torch
    stripes = np.full((1024, 2048, 3), 137, np.uint8)
    stripes[:, ::16] = 30
    flat = np.full((512, 512, 3), 90, np.uint8)
    photo = synth_image(320, 240, seed=12)
    jpegs = [oracle.encode(stripes, "420", 90), oracle.encode(flat, "444", 90), oracle.encode(photo, "420", 90),
             oracle.encode(stripes[:512, :512], "444", 75)]
    refs = [oracle.decode(j) for j in jpegs]
    assert _groups(_scan_bytes(jpegs[0])[1]) >= 3
    stats = _decode_exact(dec, jpegs, refs, on_gpu=False)
    assert stats["gpu_entropy_images"] == 4 and stats["sync_launches"] <= 6
    assert 1 <= dec.host_fallbacks() <= 2              # the striped pictures
    stats = _decode_exact(dec, jpegs[:1], refs[:1], on_gpu=False)
    assert dec.host_fallbacks() == 1 and stats["sync_launches"] <= 6
    _decode_exact(dec, jpegs[1:3], refs[1:3])          # never the flat one or the photograph
    torch.cuda.synchronize()


def test_restart_intervals_and_several_scans(dec):
    photo = synth_image(640, 480, seed=5)
    plain = oracle.encode(photo, "420", 90)
    assert _groups(_scan_bytes(plain)[1]) == 3
    jpegs = [oracle.encode(photo, "420", 90, restart_interval=r) for r in (1, 7, 240)]
    jpegs += [Q.recode(plain, [[0], [1], [2]]), Q.recode(plain, [[0], [1, 2]]), plain]
    _decode_exact(dec, jpegs, [oracle.decode(j) for j in jpegs])


def _child(args, env_extra, timeout):
    env = dict(os.environ, HIPJPEG_ENABLE_TEST_HOOKS="1", **env_extra)   # (the hooks: host_fallbacks() answers)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tail entry ok" in r.stdout, r.stdout[-2000:]
    return r


@pytest.fixture(scope="module")
def batch_file(tmp_path_factory):
    files, refs = seam_batch()
    path = tmp_path_factory.mktemp("tail_entry") / "batch.pickle"
    with open(path, "wb") as f:
        pickle.dump(([j for j, _, _ in files], refs), f)
    return str(path)


@pytest.mark.parametrize("switch", ["HIPJPEG_TAIL_AFTER=0", "HIPJPEG_TAIL_AFTER=1", "HIPJPEG_TAIL_AFTER=3", "HIPJPEG_RIPPLE_IN_SYNC=1",
                                    "HIPJPEG_POSITION_PASS=1"])
def test_group_seams_under_the_switches(batch_file, switch):
    """The switches are read once per process: a child each."""
    name, value = switch.split("=")
    _child(["batch", batch_file], {name: value}, 120)


def rounds_batch():
    return [oracle.encode(synth_image(1920, 1080, seed=400 + k), "420", 90) for k in range(16)]


def test_the_ripple_launch_has_little_left():
    """The groups of the ripple launch spend at most half the rounds they spent when the tail launch entered with pass 0's guess."""
    r = _child(["rounds"], {"HIPJPEG_DEBUG_TIMING": "1"}, 180)
    lines = re.findall(r"launch 2: (\d+) rounds in total", r.stderr)
    assert len(lines) == 1, r.stderr[-2000:]
    rounds = int(lines[0])
    print("ripple launch: %d rounds in total (parent %d, bound %d)" % (rounds, PARENT_RIPPLE_ROUNDS, RIPPLE_ROUNDS_BOUND))
    assert rounds <= RIPPLE_ROUNDS_BOUND


if __name__ == "__main__":
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(device=0, num_threads=4)
    if sys.argv[1] == "batch":
        with open(sys.argv[2], "rb") as f:
            jpegs, refs = pickle.load(f)
        _decode_exact(d, jpegs, refs)
    else:
        jpegs = rounds_batch()
        assert sum(_groups(_scan_bytes(j)[1]) for j in jpegs) == 240
        _decode_exact(d, jpegs, [oracle.decode(j) for j in jpegs])
    print("tail entry ok")
    d.close()
