"""bench.py's launcher logic, without a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, env=e)


def test_more_gpus_than_visible_is_refused():
    import torch
    if torch.cuda.device_count() >= 2:
        return
    p = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert p.returncode != 0 and "refusing to measure fewer than asked for" in p.stderr


def test_world_size_must_match_gpus():
    p = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], env={"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE=4" in p.stderr


def test_without_a_gpu_the_bench_fails_loudly():
    import torch
    if torch.cuda.is_available():
        return
    p = _run(["--steps", "1", "--warmup", "0"])
    assert p.returncode != 0 and "needs a GPU" in p.stderr


def test_steps_must_be_positive():
    p = _run(["--steps", "0", "--warmup", "0"])
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr


def test_dump_outputs_writes_a_seeded_float_sample(tmp_path):
    """--dump-outputs: float32/float64 arrays only, the same pixel positions on every call, values and sums those of the outputs."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(3)
    outs = [torch.randint(0, 256, (bench.HEIGHT, bench.WIDTH, 3), dtype=torch.uint8, generator=g) for _ in range(3)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, [0, 0, 2])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["rgb_sample.npy", "rgb_sample_yx.npy", "rgb_sum.npy", "status.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    yx = np.load(tmp_path / "a" / "rgb_sample_yx.npy").astype(np.int64)
    sample = np.load(tmp_path / "a" / "rgb_sample.npy")
    assert sample.shape == (3, bench.DUMP_PIXELS, 3) and len(np.unique(yx[:, 0] * bench.WIDTH + yx[:, 1])) == bench.DUMP_PIXELS
    for o, s, total in zip(outs, sample, np.load(tmp_path / "a" / "rgb_sum.npy")):
        o = o.numpy()
        assert np.array_equal(s, o[yx[:, 0], yx[:, 1]]) and np.array_equal(total, o.reshape(-1, 3).sum(0, dtype=np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), [0, 0, 2])
    # a full batch stays inside the 64 MB budget
    per_image = bench.DUMP_PIXELS * 3 * 4 + 3 * 8 + 8
    assert bench.BATCH * per_image + bench.DUMP_PIXELS * 2 * 8 <= bench.DUMP_MAX_BYTES
