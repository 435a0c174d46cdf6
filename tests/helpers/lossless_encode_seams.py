"""Pictures that sit on the seams of the lossless coder's kernels, built from hipjpegLosslessEncodeShape (never hard-coded): the group
of samples a lane codes, the samples of a workgroup (the write kernel's LDS window) and the stuffing chunk.  Shared by the host tests
(plain coder and twin against the numpy model) and the GPU tests (kernels against the twin)."""
import numpy as np

from helpers import lossless_encode_model as M
from helpers import lossless_files as LF

# Seeds found by the searches below (search_* re-derive them; the tests assert the property before they use a seed)
SEED_INTERVAL_ENDS_ON_BYTE = 20
SEED_INTERVAL_ONE_BIT_SHORT = 8
SEED_FF_LAST_OF_CHUNK = 153   # for a chunk of 4096 bytes; another chunk size makes the tests search again
SEED_FF_FIRST_OF_CHUNK = 19
SEED_FF_BEFORE_RST = 1
SEEDS_CHUNK_BYTES = 4096

SEARCH_LIMIT = 4000


def sample_bits(samples, precision, ps, pt, restart_rows):
    """bits of every sample (H x W x N) under the file's pooled table"""
    d = M.differences(samples, precision, ps, pt, restart_rows)
    lut = LF._codes(*M.pooled_table(d))
    ssss, _ = LF.categories(d)
    size = np.array([lut.get(s, (0, 0))[1] for s in range(17)])
    return size[ssss] + np.where(ssss == 16, 0, ssss)


def unstuffed_scan(data, n):
    """the entropy-coded bytes of a file without restart intervals, stuffing removed, EOI dropped"""
    scan = M.scan_bytes(data, n)[:-2]
    return scan.replace(b"\xff\x00", b"\xff")


def interval_picture(seed):
    return LF.random_samples(seed, 4, 19, 1, 12, 0, smooth=False).astype(np.uint16), dict(precision=12, predictor=1, restart_rows=2)


def first_interval_tail_bits(seed):
    s, p = interval_picture(seed)
    return int(sample_bits(s, 12, 1, 0, 2)[:2].sum()) % 8


def chunk_picture(seed, chunk_bytes):
    """noisy 16-bit gray, about 16 bits a sample: just large enough for two chunks"""
    side = int(np.ceil(np.sqrt(chunk_bytes * 8 / 16.0 * 1.4)))
    return LF.random_samples(seed, side, side, 1, 16, 0, smooth=False).astype(np.uint16), dict(precision=16, predictor=1)


def chunk_bytes_at_seam(seed, chunk_bytes):
    s, p = chunk_picture(seed, chunk_bytes)
    raw = unstuffed_scan(M.model_file(s, 16, 1), 1)
    assert chunk_bytes < len(raw) <= 2 * chunk_bytes, len(raw)
    return raw[chunk_bytes - 1], raw[chunk_bytes]


def rst_picture(seed):
    return LF.random_samples(seed, 6, 9, 1, 16, 0, smooth=False).astype(np.uint16), dict(precision=16, predictor=1, restart_rows=1)


def ff_before_rst(seed):
    s, p = rst_picture(seed)
    data = M.model_file(s, 16, 1, 0, 1)
    return any(bytes([0xFF, 0x00, 0xFF, 0xD0 + k]) in data for k in range(8))


def search(predicate):
    """bounded, and loud when nothing is found"""
    for seed in range(SEARCH_LIMIT):
        if predicate(seed):
            return seed
    raise AssertionError("no seed below %d has the property" % SEARCH_LIMIT)


def searched_cases(shape):
    """The seams that take a seed search: each case asserts its property before it is handed out.  Same dicts as cases()."""
    chunk = shape["chunk_bytes"]
    if chunk == SEEDS_CHUNK_BYTES:
        last, first = SEED_FF_LAST_OF_CHUNK, SEED_FF_FIRST_OF_CHUNK
    else:
        last = search(lambda s: chunk_bytes_at_seam(s, chunk)[0] == 0xFF)
        first = search(lambda s: chunk_bytes_at_seam(s, chunk)[1] == 0xFF)
    assert first_interval_tail_bits(SEED_INTERVAL_ENDS_ON_BYTE) == 0 and first_interval_tail_bits(SEED_INTERVAL_ONE_BIT_SHORT) == 7
    assert chunk_bytes_at_seam(last, chunk)[0] == 0xFF and chunk_bytes_at_seam(first, chunk)[1] == 0xFF
    assert ff_before_rst(SEED_FF_BEFORE_RST)
    out = []
    for name, (s, p) in (("interval_ends_on_byte", interval_picture(SEED_INTERVAL_ENDS_ON_BYTE)),
                         ("interval_one_bit_short", interval_picture(SEED_INTERVAL_ONE_BIT_SHORT)),
                         ("ff_last_of_chunk", chunk_picture(last, chunk)), ("ff_first_of_chunk", chunk_picture(first, chunk)),
                         ("ff_before_rst", rst_picture(SEED_FF_BEFORE_RST))):
        out.append(dict(name=name, samples=M.as_hwn(s), precision=p["precision"], predictor=p["predictor"], point_transform=0,
                        restart_rows=p.get("restart_rows", 0), planar=False, pad=len(out) + 1, offset=2 * len(out) + 1))
    return out


def cases(shape):
    """-> list of dicts: name, samples (H x W x N), precision, predictor, point_transform, restart_rows, planar, pad, offset"""
    G, window, chunk = shape["group_samples"], shape["window_samples"], shape["chunk_bytes"]
    out = []
    k = [0]

    def add(name, s, P, ps=1, pt=0, rr=0, planar=None):
        i = k[0]
        k[0] += 1
        s = M.as_hwn(s)
        out.append(dict(name=name, samples=s, precision=P, predictor=ps, point_transform=pt, restart_rows=rr,
                        planar=(i % 2 == 1) if planar is None else planar, pad=1 + (2 * i) % 15, offset=1 + (3 * i) % 15))

    def rnd(seed, h, w, n, P, smooth=True, pt=0):
        return LF.random_samples(seed, h, w, n, P, pt, smooth).astype(np.uint8 if P <= 8 else np.uint16)

    seed = 500
    # a row of G - 1, G, G + 1 and 2 G + 1 samples, for every component count that divides it; heights 1, 2, 3: groups straddle row
    # ends, and with restart_rows = 1 interval ends
    for target in (G - 1, G, G + 1, 2 * G + 1):
        for n in (1, 2, 3, 4):
            if target % n:
                continue
            for h in (1, 2, 3):
                seed += 1
                P = (8, 12, 16, 5)[seed % 4]
                add(f"row{target}_c{n}_h{h}", rnd(seed, h, target // n, n, P, smooth=seed % 3 != 0), P, ps=1 + seed % 7, rr=(0, 1)[seed % 2] if h > 1 else 0)
    # the window's sample count - 1, + 0, + 1 (one more workgroup with a single sample), in one row and in several
    for total in (window - 1, window, window + 1):
        seed += 1
        add(f"window{total}_row", rnd(seed, 1, total, 1, 16, smooth=False), 16)
        for h in range(2, 40):
            if total % h == 0:
                seed += 1
                add(f"window{total}_h{h}", rnd(seed, h, total // h, 1, 8), 8, ps=4, rr=1)
                break
    # every component count, interleaved and planar, uint8 and uint16, every predictor
    for n in (1, 2, 3, 4):
        for planar in (False, True):
            for P in (8, 16):
                seed += 1
                add(f"c{n}_{'planar' if planar else 'interleaved'}_p{P}", rnd(seed, 5, 2 * G + 3, n, P, smooth=seed % 2 == 0), P, ps=1 + seed % 7, pt=seed % 3,
                    planar=planar)
    # restart rows: 1, H, H - 1, and the RSTn wrap
    for name, h, rr in (("rst1", 4, 1), ("rstH", 4, 4), ("rstHm1", 4, 3), ("rst_wrap", 11, 1)):
        seed += 1
        add(name, rnd(seed, h, G + 3, 3, 12), 12, ps=6, rr=rr)
    # a vector of the statistics pass that ends exactly at the row's end, one byte short of it, and one byte beyond
    for w in (16, 15, 17, 32, 33):
        seed += 1
        add(f"stat_u8_w{w}", rnd(seed, 3, w, 1, 8), 8, ps=5)
        add(f"stat_u16_w{w}", rnd(seed, 3, w, 1, 12), 12, ps=7, rr=2)
    add("stat_c3_w16", rnd(seed + 1, 3, 16, 3, 8), 8, ps=4, planar=False)
    add("constant", np.full((5, 13, 2), 200, dtype=np.uint8), 8, ps=2)
    s = rnd(seed + 2, 4, 12, 1, 16, smooth=False)
    s[2, 0::2], s[2, 1::2] = 0, 32768
    add("ssss16", s, 16)
    return out
