"""GPU: the verdicts of the GPU entropy stage -- the convergence counters and, per stream, status and gave_up -- reach the
host without a copy command behind the stage: its last kernel stores them into the batch's pinned memory (csrc/gpu_huffman.hip
huff_dc_group_kernel, csrc/decoder_core.cpp resolve()).  Whatever asks for the statuses must still get the host path's answer:
straight behind the entropy stage with no pixel kernel queued, after several entropy stages on one decoder without a resolve in
between (what bench.py does), and with three batches in flight on their own pages."""
import numpy as np
import pytest

import oracle
from nvimagecodec_amd.synth import synth_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    import torch
    assert torch.cuda.is_available()
    from nvimagecodec_amd.lowlevel import BatchDecoder
    d = BatchDecoder(0, num_threads=4)
    yield d
    d.close()


@pytest.fixture(scope="module")
def streams():
    """good: four small photographs; truncated: one of them cut; damaged: a restart-interval stream with four bytes of one interval
    changed; periodic: the smallest striped picture of tests/test_gpu_huffman.py."""
    good = [oracle.encode(synth_image(w, h, seed=20 + k), sub, 90)
            for k, (w, h, sub) in enumerate(((64, 64, "420"), (256, 256, "420"), (200, 136, "422"), (96, 256, "444")))]
    truncated = good[1][: len(good[1]) * 2 // 3] + b"\xff\xd9"
    rst = oracle.encode(synth_image(160, 120, seed=7), "420", 30, restart_interval=1)
    damaged = _damage(rst)
    stripes = np.full((1024, 1024, 3), 137, np.uint8)
    stripes[:, ::16] = 30
    periodic = oracle.encode(stripes, "444", 75)
    refs = {j: oracle.decode(j) for j in good + [periodic, rst]}
    return dict(good=good, truncated=truncated, damaged=damaged, rst=rst, periodic=periodic, refs=refs)


def _damage(rst):
    """Four data bytes in the middle of the scan changed, no FF touched or made (the markers stay where they are, so the stream stays
    eligible for the GPU stage): the first such place at which the host entropy decoder rejects the file."""
    from nvimagecodec_amd import _native as N
    from nvimagecodec_amd import lowlevel
    sos = rst.rfind(b"\xff\xda") + 14
    for at in range(sos + (len(rst) - sos) // 2, len(rst) - 8):
        b = bytearray(rst)
        if 0xFF in b[at - 1:at + 5] or any(x ^ 0x55 == 0xFF for x in b[at:at + 4]):
            continue
        for k in range(4):
            b[at + k] ^= 0x55
        try:
            lowlevel.entropy_decode_host(bytes(b))
        except N.HipJpegError:
            return bytes(b)
    raise AssertionError("no damage found that the host decoder rejects")


def _host_statuses(dec, jpegs):
    import torch
    _, st = dec.decode(jpegs, gpu_huffman=False, check=False)
    torch.cuda.synchronize()
    return list(st)


def _mixed(streams):
    g = streams["good"]
    return [g[0], streams["truncated"], g[1], streams["damaged"], streams["periodic"], g[2], streams["rst"], g[3]]


def test_statuses_straight_behind_the_entropy_stage(dec, streams):
    """device_stage(which=6) and then statuses(): no pixel kernel lies between the stage's last kernel and the host's read."""
    import torch
    jpegs = _mixed(streams)
    want = _host_statuses(dec, jpegs)
    assert want[0] == 0 and want[1] != 0 and want[2] == 0 and want[3] != 0 and want[4] == 0
    outs = dec.allocate_outputs(jpegs)
    dec.host_stage(jpegs, outs, gpu_huffman=True)
    dec.transfer()
    dec.device_stage(which=6)
    got = dec.statuses(len(jpegs))
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(jpegs)
    assert dec.host_fallbacks() >= 2    # the truncated and the damaged stream at least
    assert got == want


def test_statuses_after_three_steps_without_a_resolve(dec, streams):
    """Three times entropy stage, K1, K2 on the same decoder, as bench.py times them, then statuses(): the last step's verdicts."""
    import torch
    jpegs = _mixed(streams)
    want = _host_statuses(dec, jpegs)
    outs = dec.allocate_outputs(jpegs)
    dec.host_stage(jpegs, outs, gpu_huffman=True)
    dec.transfer()
    for _ in range(3):
        dec.device_stage(which=6)
        dec.device_stage(which=0)
        dec.device_stage(which=1)
    got = dec.statuses(len(jpegs))
    torch.cuda.synchronize()
    assert got == want
    for j, o, s in zip(jpegs, outs, got):   # (the pictures the GPU stage kept: single pixel kernels are not repeated behind a hand-over)
        if j in streams["good"] or j == streams["rst"]:
            assert s == 0 and np.array_equal(o.cpu().numpy(), streams["refs"][j])


def test_all_good_batch_stays_on_the_gpu_path(dec, streams):
    import torch
    jpegs = streams["good"] + [streams["rst"]]
    outs = dec.allocate_outputs(jpegs)
    dec.host_stage(jpegs, outs, gpu_huffman=True)
    dec.transfer()
    for _ in range(2):
        dec.device_stage(which=6)
        dec.device_stage(which=0)
        dec.device_stage(which=1)
    assert dec.statuses(len(jpegs)) == [0] * len(jpegs)
    torch.cuda.synchronize()
    assert dec.stats()["gpu_entropy_images"] == len(jpegs) and dec.host_fallbacks() == 0
    for j, o in zip(jpegs, outs):
        assert np.array_equal(o.cpu().numpy(), streams["refs"][j])


def test_three_batches_in_flight_get_their_own_verdicts(dec, streams):
    """Submit / Wait three deep, six batches: all-good ones alternate with ones that hold a truncated and a periodic stream, at
    changing places, so that an all-good batch reuses the page -- and the pinned verdict words -- of a batch with flagged streams.
    Every Wait returns its own batch's statuses, those of the host entropy stage; every intact picture has the oracle's pixels;
    and every batch hands to the host decoder exactly what it hands over when it is decoded alone: nothing, for the all-good ones."""
    import torch
    g, t, p = streams["good"], streams["truncated"], streams["periodic"]
    batches = [g[:3], [t, g[0], p], [g[3], g[1], g[2]], [g[2], p, t, g[3]], g[1:4], [p, t]]
    # one at a time first: the host stage's statuses, and how many streams the GPU stage hands back
    want, handed = [], []
    for b in batches:
        want.append(_host_statuses(dec, b))
        _, st = dec.decode(b, gpu_huffman=True, check=False)
        torch.cuda.synchronize()
        assert list(st) == want[-1]
        handed.append(dec.host_fallbacks())
        flagged = sum(1 for j in b if j == t)
        assert flagged <= handed[-1] <= flagged + sum(1 for j in b if j == p)    # the truncated stream always, the periodic one perhaps
    assert [h for b, h in zip(batches, handed) if t not in b] == [0, 0, 0]
    outs = [dec.allocate_outputs(b) for b in batches]
    results, fallbacks = [], []

    def wait():
        results.append(dec.wait(check=False))
        fallbacks.append(dec.host_fallbacks())      # (of the batch that Wait settled)

    for k, b in enumerate(batches):
        dec.submit(b, outs[k])
        assert dec.stats()["gpu_entropy_images"] == len(b), k      # (of the batch just planned)
        if k >= 2:
            wait()
    wait()
    wait()
    torch.cuda.synchronize()
    assert len(results) == len(batches)
    assert fallbacks == handed
    for k, (b, st) in enumerate(zip(batches, results)):
        assert list(st) == want[k], k
        for i, j in enumerate(b):
            if j == t:
                assert st[i] in (4, 5), (k, i, st)
            else:
                assert st[i] == 0, (k, i, st)
                assert np.array_equal(outs[k][i].cpu().numpy(), streams["refs"][j]), (k, i)
