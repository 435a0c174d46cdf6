"""Dev tool (CPU only): how often a symbol of the bench's sources ends a block or has a code longer than the first-level lookup of
the GPU entropy walks (kHuffFastBits = 10 bits), per symbol and per wave-step of 64 lanes at independent places of the stream
(1 - (1 - p)^64).  A plain Python Huffman walk over every source of bench.make_inputs().
usage: walk_event_shares.py   (profiles/walk_steps/event_shares.txt was made with it)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

FAST_BITS = 10


def segments(data):
    pos, tables, comps, size = 2, {}, [], None
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + n]
        if m == 0xC4:
            q = 0
            while q < len(seg):
                ident, bits = seg[q], list(seg[q + 1:q + 17])
                vals = list(seg[q + 17:q + 17 + sum(bits)])
                tables[ident] = (bits, vals)
                q += 17 + sum(bits)
        elif m in (0xC0, 0xC1):
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15) for i in range(seg[5])]
            size = (int.from_bytes(seg[3:5], "big"), int.from_bytes(seg[1:3], "big"))
        elif m == 0xDA:
            scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            return tables, comps, size, scan, pos + 2 + n
        pos += 2 + n


def decoder(bits, vals):
    """16-bit window -> (code length, symbol)"""
    look, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            look[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    table = [None] * 65536
    for (length, code), sym in look.items():
        lo = code << (16 - length)
        for w in range(lo, lo + (1 << (16 - length))):
            table[w] = (length, sym)
    return table


def count(jpeg):
    tables, comps, (width, height), scan, start = segments(jpeg)
    end = jpeg.rindex(b"\xff\xd9")
    raw = jpeg[start:end].replace(b"\xff\x00", b"\xff") + b"\xff" * 8
    order = []
    for cid, td, ta in scan:
        h, v = next((h, v) for i, h, v in comps if i == cid)
        order += [(decoder(*tables[td]), decoder(*tables[0x10 | ta]))] * (h * v)
    hmax, vmax = max(h for _, h, _ in comps), max(v for _, _, v in comps)
    total_blocks = -(-width // (8 * hmax)) * -(-height // (8 * vmax)) * len(order)
    pos, symbols, long_codes, k = 0, 0, 0, 0
    for _ in range(total_blocks):
        dc, ac = order[k]
        z = 0
        while z < 64:
            b = pos >> 3
            window = (int.from_bytes(raw[b:b + 4], "big") >> (16 - (pos & 7))) & 0xFFFF
            length, sym = (dc if z == 0 else ac)[window]
            symbols += 1
            long_codes += length > FAST_BITS
            size = sym & 15
            pos += length + size
            z += 1 if z == 0 else (sym >> 4) + 1 if size else (16 if sym == 0xF0 else 64)
        k = (k + 1) % len(order)
    blocks = total_blocks
    assert 0 <= 8 * (len(raw) - 8) - pos < 8, "the walk did not end on the scan's last byte"
    return len(raw) - 8, symbols, blocks, long_codes


if __name__ == "__main__":
    sources, what = bench.make_inputs()
    print(what)
    for s, jpeg in enumerate(sources):
        nbytes, symbols, blocks, long_codes = count(jpeg)
        pe, pl = blocks / symbols, long_codes / symbols
        print("source %d: %d scan bytes, %d symbols in %d blocks (%.1f per block); a symbol ends a block %.2f %%, has a long code %.2f %%; "
              "some lane of 64: %.1f %% / %.1f %%" % (s, nbytes, symbols, blocks, symbols / blocks, 100 * pe, 100 * pl,
                                                     100 * (1 - (1 - pe) ** 64), 100 * (1 - (1 - pl) ** 64)))
