"""The lossless coder on arenas that are not zero (docs/arena_regions.md, LosslessEncodeBatch): BatchLosslessEncoder on C-ABI allocators
that hand out memory filled with a poison byte, fresh and refilled between two batches of one handle, with the library's own pinned
memory and with the caller's.  Every fill must give the same files, equal to the host twin's."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lossless_encode_model as M
from helpers import lossless_encode_seams as S
from helpers.poisoned_memory import PoisonAllocators
from nvimagecodec_amd import _native as N
from nvimagecodec_amd import lowlevel as LL

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_lossless_encode.json")))["lossless_encode"]


def _run(torch, byte, pinned, cases):
    poison = PoisonAllocators(byte, pinned=pinned)
    enc = LL.BatchLosslessEncoder(device=0, num_threads=2, allocators=poison)
    try:
        raw, keep = [], []
        for c in cases:
            x, n, bufs = M.padded_input(N, c["samples"], c["planar"], c["pad"], c["offset"])
            dev = [torch.from_numpy(b).cuda() for b in bufs]
            for k, d in enumerate(dev):
                x.plane[k] = d.data_ptr() + c["offset"]
            keep.append(dev)
            raw.append((x, n))
        args = ([c["precision"] for c in cases], [c["predictor"] for c in cases], [c["point_transform"] for c in cases],
                [c["restart_rows"] for c in cases])
        # a small batch first, so that the large one grows the arenas and the small one after it works inside what the large one left
        order = [[raw[:3]] + [a[:3] for a in args], [raw] + list(args), [raw[:3]] + [a[:3] for a in args]]
        results = []
        for k, (r, P, ps, pt, rr) in enumerate(order):
            if k:
                torch.cuda.synchronize()
                poison.refill()
            statuses, files = M.encode_raw_batch(enc, r, P, ps, pt, rr)
            assert statuses == [0] * len(r)
            results.append(files)
        assert poison.device_calls >= 2 and (poison.pinned_calls >= 2) == pinned
    finally:
        enc.close()
    assert poison.all_freed(), (poison.live, poison.live_pinned, poison.errors)
    return results


@pytest.mark.parametrize("pinned", [False, True])
def test_two_poison_bytes_give_the_twins_files(pinned):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    shape = LL.lossless_encode_shape()
    cases = S.searched_cases(shape) + S.cases(shape)[::4]
    for e in [e for e in MANIFEST if not e["stored"]]:
        cases.append(dict(name=e["name"], samples=M.case_samples(e), precision=e["precision"], predictor=e["predictor"],
                          point_transform=e["point_transform"], restart_rows=e["restart_rows"], planar=False, pad=3, offset=5))
    want = [LL.encode_lossless_gpu_algorithm_host(np.ascontiguousarray(c["samples"]), c["precision"], c["predictor"], c["point_transform"],
                                                  c["restart_rows"]) for c in cases]
    a = _run(torch, 0x5A, pinned, cases)
    b = _run(torch, 0xFF, pinned, cases)
    assert a == b
    assert a[1] == want and a[0] == want[:3] and a[2] == want[:3]
