"""Lossless JPEG files that put samples on the seams of the GPU entropy stage (subsequences of S bits, G of them per workgroup), files
whose walk cannot synchronise, and damaged files.  Built with tests/helpers/lossless_files.py; used by the host twin's tests and by
the GPU tests alike.

Under LF.FLAT a sample is exactly 5 + SSSS bits (5 for SSSS 16), under LF.long_table 2 bits for SSSS 0, 3 for SSSS 1 and 31 for
SSSS 15 (2 s + 1 for SSSS s = 2 .. 14), so the bit at which any sample starts can be chosen.
"""
import numpy as np

from helpers import lossless_files as LF


def diff_of(ssss):
    """a difference of category ssss whose extra bits are a one and zeros"""
    return 0 if ssss == 0 else 32768 if ssss == 16 else 1 << (ssss - 1)


def flat_categories(bits, seed=1):
    """categories, drawn at random, whose samples take exactly `bits` bits under the flat table (bits = 5 .. 20, or >= 41).  (Not one
    category over and over: a periodic stream lets a parse that started at a wrong bit live for ever, and that is a case of its own.)"""
    if bits <= 20:
        assert bits >= 5
        return [bits - 5]
    assert bits >= 41
    rng = np.random.default_rng(seed)
    out = []
    while bits > 40:
        s = int(rng.integers(0, 17))
        out.append(s)
        bits -= 5 if s == 16 else 5 + s
    return out + [bits // 2 - 5, bits - bits // 2 - 5]


def long_prefix(bits):
    """categories 0 and 1 whose samples take exactly `bits` >= 2 bits under the long table"""
    assert bits >= 2
    return [1] * (bits % 2) + [0] * ((bits - 3 * (bits % 2)) // 2)


def long_categories(bits, seed=1):
    """categories 0 .. 10, drawn at random, whose samples take exactly `bits` bits under the long table"""
    rng = np.random.default_rng(seed)
    out = []
    while bits >= 34:
        s = int(rng.integers(0, 11))
        out.append(s)
        bits -= 2 if s == 0 else 2 * s + 1
    return out + long_prefix(bits)


def one_row(categories, table, **kw):
    """-> (file, differences H x W x 1): one row, or, where the samples are more than a row can hold, rows of 4096 filled up with
    zeros (the samples of a scan without restart intervals are one run whatever the width)"""
    categories = list(categories)
    if len(categories) > 65535:
        categories += [0] * (-len(categories) % 4096)
    d = np.array([diff_of(s) for s in categories], dtype=np.int64).reshape(-1 if len(categories) > 65535 else 1, min(len(categories), 4096)
                                                                           if len(categories) > 65535 else len(categories), 1)
    tables = [LF.flat_table()] if table == LF.FLAT else [LF.long_table()]
    return LF.write_differences(d, 16, 1, tables=tables, **kw), d


def scan_of(data):
    """(first byte of the entropy-coded data, the EOI's position)"""
    sos = data.index(b"\xff\xda")
    begin = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    return begin, data.rindex(b"\xff\xd9")


def seam_cases(shape):
    """-> [(name, file, differences H x W x N, restart_rows)]; every file decodes, under predictor 1 at 16 bits, to
    LF.model_decode(differences, 16, 1, 0, restart_rows)"""
    S, G = shape["subsequence_bits"], shape["subsequences_per_workgroup"]
    cases = []

    def add(name, file, d, rr=0):
        cases.append((name, file, d, rr))

    add("one sample", *one_row([7], LF.FLAT))
    for bits in (S - 1, S, S + 1, G * S - 1, G * S, G * S + 1):
        add(f"{bits} bits", *one_row(flat_categories(bits), LF.FLAT))
    # a 31-bit sample across a border
    for border, what in ((S, "subsequence"), (G * S, "workgroup")):
        for before in (1, 15, 16, 30):
            cats = long_categories(border - before) + [15] + long_categories(S + 7, seed=2)
            add(f"31-bit sample {before} bits before a {what} border", *one_row(cats, LF.LONG))
    # categories without extra bits as the last sample of a subsequence
    for s in (16, 0):
        add(f"SSSS {s} ends a subsequence", *one_row(flat_categories(S - 5) + [s] + flat_categories(S + 3), LF.FLAT))
    # a stuffed FF as the first and as the last byte of a subsequence: 32767 is 0, then nineteen ones
    for name, at in (("first", S - 5), ("last", S - 13)):
        cats = flat_categories(at)
        d = np.array([diff_of(s) for s in cats] + [0] + [diff_of(s) for s in flat_categories(2 * S)], dtype=np.int64).reshape(1, -1, 1)
        d = LF.with_stuffed_byte(d, (0, len(cats), 0))
        f = LF.write_differences(d, 16, 1, table=LF.FLAT)
        begin, end = scan_of(f)
        stuffed = f.index(b"\xff\x00", begin)
        assert (stuffed - begin) * 8 == (S if name == "first" else S - 8), name
        add(f"stuffed FF as the {name} byte of a subsequence", f, d)
    # components, one table for all and one each
    rng = np.random.default_rng(2026)
    others = [LF.flat_table(), LF.long_table(), LF.long_table(list(range(16, -1, -1))), LF.long_table([1, 0] + list(range(2, 17)))]
    for n in (1, 2, 3, 4):
        d = rng.integers(0, 65536, size=(9, 131, n))
        add(f"{n} components, one table", LF.write_differences(d, 16, 1, table=LF.FLAT), d)
        add(f"{n} components, a table each", LF.write_differences(d, 16, 1, tables=others[:n]), d)
    d = rng.integers(0, 65536, size=(3 * G // 8, 131, 3))  # several workgroups
    add("3 components over workgroup borders", LF.write_differences(d, 16, 1, tables=others[:3]), d)
    # a smooth picture under tables made for it (codes of one to a few bits, every code but the ones in use): what natural files
    # look like, over several workgroups
    d = LF.differences_of_states(LF.random_samples(5, 150, 300, 3, 16), 16, 1)
    add("a smooth picture, optimal tables, over workgroup borders", LF.write_differences(d, 16, 1), d)
    # restart intervals
    for w in (1, 65):
        d = rng.integers(0, 65536, size=(11, w, 2))
        add(f"intervals of one row, width {w}", LF.write_differences(d, 16, 1, 0, 1, table=LF.FLAT), d, 1)
    row = [diff_of(s) for s in flat_categories(S)]
    d = np.array([row, row[::-1], row], dtype=np.int64).reshape(3, -1, 1)  # (reversed: as many bits)
    add("intervals that end on a subsequence border", LF.write_differences(d, 16, 1, 0, 1, table=LF.FLAT), d, 1)
    # every pad length: row k has k more bits than a whole number of bytes
    width = S // 8 + 8
    rows = [[diff_of(s) for s in [4] * k + [3] * (width - k)] for k in range(1, 8)]
    d = np.array(rows, dtype=np.int64).reshape(7, width, 1)
    add("intervals with pad lengths 1 to 7", LF.write_differences(d, 16, 1, 0, 1, table=LF.FLAT), d, 1)
    return cases


def unsynchronisable(shape):
    """A constant picture of three components, a different table each: all zeros under the flat table's 00000 and the long tables'
    00, periodic with nine bits.  Every guess parses for ever and none drifts onto the true samples.  -> (file, differences)"""
    S = shape["subsequence_bits"]
    budget = shape["max_rounds"] * (shape["max_ripple_launches"] + 1)  # subsequences a correction can travel: every launch runs max_rounds
    pixels = (2 * budget + 16) * S // 9
    d = np.zeros((pixels // 300 + 1, 300, 3), dtype=np.int64)
    f = LF.write_differences(d, 8, 1, tables=[LF.flat_table(), LF.long_table(), LF.long_table([1, 0] + list(range(2, 17)))])
    begin, end = scan_of(f)
    assert (end - begin) * 8 > (shape["max_rounds"] + shape["max_ripple_launches"]) * S and (end - begin) * 8 > (budget + 8) * S
    return f, d


def _intervals(data):
    """the pieces of a file: header, the intervals' bytes, the markers between them, trailer"""
    begin, end = scan_of(data)
    cuts = [i for i in range(begin, end - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    pieces, at = [], begin
    for c in cuts:
        pieces.append(data[at:c])
        at = c + 2
    pieces.append(data[at:end])
    return data[:begin], pieces, [data[c:c + 2] for c in cuts], data[end:]


def _join(head, pieces, markers, tail):
    out = bytearray(head)
    for k, p in enumerate(pieces):
        if k:
            out += markers[k - 1]
        out += p
    return bytes(out + tail)


def bad_cases():
    """-> [(name, file)]: files whose scan is damaged; the status is whatever hipjpegDecodeLosslessHost says of them"""
    rng = np.random.default_rng(77)
    d = rng.integers(0, 65536, size=(6, 90, 1))
    plain = LF.write_differences(d, 16, 1, table=LF.FLAT)
    rst = LF.write_differences(d, 16, 1, 0, 1, table=LF.FLAT)
    wider = LF.write_differences(rng.integers(0, 65536, size=(6, 91, 1)), 16, 1, 0, 1, table=LF.FLAT)
    narrower = LF.write_differences(rng.integers(0, 65536, size=(6, 89, 1)), 16, 1, 0, 1, table=LF.FLAT)
    begin, end = scan_of(plain)
    cases = [("truncated mid-sample", plain[:begin + (end - begin) // 2 + 1]),
             ("truncated mid-sample, EOI kept", plain[:begin + (end - begin) // 2 + 1] + b"\xff\xd9")]
    no_code = bytearray(plain)
    no_code[begin] = 0x8B  # 10001...: the flat table has codes 00000 to 10000 only
    cases.append(("a code no table holds", bytes(no_code)))
    head, pieces, markers, tail = _intervals(rst)
    assert len(pieces) == 6
    in_turn = [bytes([0xFF, 0xD0 + k]) for k in range(8)]
    cases.append(("a restart marker missing", _join(head, [pieces[0], pieces[1] + pieces[2]] + pieces[3:], in_turn[:4], tail)))
    half = len(pieces[2]) // 2
    early = [pieces[0], pieces[1], pieces[2][:half], pieces[2][half:]] + pieces[3:]
    cases.append(("a restart marker early", _join(head, early, in_turn[:6], tail)))
    turn = list(markers)
    turn[1] = b"\xff\xd5"
    cases.append(("a restart marker out of turn", _join(head, pieces, turn, tail)))
    for name, other in (("one sample too many in an interval", wider), ("one sample too few in an interval", narrower)):
        _, other_pieces, _, _ = _intervals(other)
        mixed = list(pieces)
        mixed[3] = other_pieces[3]
        cases.append((name, _join(head, mixed, markers, tail)))
    return cases
