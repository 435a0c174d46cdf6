"""Test helper: the outputs of one decode batch placed inside ONE byte arena, every byte around them a sentinel.

A tightly packed output (BatchDecoder.allocate_outputs) ties pointer, pitch and width together -- pitch is W or 3 W -- so some
combinations of a store path's conditions cannot occur, and a store past the end of a row lands at the start of the next row (where
another wave overwrites it) or in the allocator's slack.  Here every output is a torch.as_strided view at a chosen (offset, pitch) of
one uint8 tensor: LEAD sentinel bytes in front of the first frame, TAIL behind the last, at least GAP between two frames and between
two planes, and whatever the pitch leaves behind each row.  check() copies the arena to the host once and asserts that every output
holds its expectation and that EVERY OTHER byte still is the sentinel; a failure names the image, the plane, the row and how far
past that row's end the first stray bytes lie.  A stray byte can equal one sentinel, not both: run every batch with each of SENTINELS.

A Layout holds the placement and knows no tensor; Arena(layout, sentinel, device) allocates.  Works on CPU tensors (tests/test_pixel_seams.py
plants stray bytes there)."""
import collections
import hashlib

import numpy as np

LEAD = 4096
TAIL = 4096
GAP = 128           # least distance between two frames / two planes (a frame starts on the next multiple of ALIGN behind it)
ALIGN = 256         # frame origins are multiples of this, plus the residue a case asks for
SENTINELS = (0xAB, 0x54)

# one plane of an output: `rows` rows of `row_bytes` bytes, row y at offset + y * pitch of the arena
Plane = collections.namedtuple("Plane", "offset pitch rows row_bytes")
Frame = collections.namedtuple("Frame", "name fmt shape planes")
# an expectation given as a hash: sha256 of canon(decoded array) must be `sha256` (the scaled goldens pin hashes, not pixels)
Hashed = collections.namedtuple("Hashed", "sha256 canon")


def _plane_extent(rows, row_bytes, pitch):
    return (rows - 1) * pitch + row_bytes if rows else 0


class Layout:
    """Where the outputs of a batch lie.  add() places one output behind the ones before it and returns its index."""

    def __init__(self, lead=LEAD, tail=TAIL, gap=GAP):
        assert lead >= LEAD and tail >= TAIL and gap >= 16
        self.lead, self.tail, self.gap = lead, tail, gap
        self.frames = []
        self._cursor = lead

    def _origin(self, residue):
        base = -(-self._cursor // ALIGN) * ALIGN
        return base + residue

    def add(self, name, fmt, shape, pitch=None, residue=0, plane_stride=None, planes=None):
        """fmt rgb / bgr: shape (H, W, 3); rgb_planar / bgr_planar: (3, H, W); y: (H, W); yuv_planar: a list of (h, w).
        pitch: bytes between rows (default: tight); residue: the first byte's offset modulo ALIGN.
        planar: plane_stride = bytes between planes (default: the least that keeps the gap; its residue modulo 8 or 16 sets the planes'
        relative alignment).  yuv_planar: planes = per plane (pitch, residue), each plane placed on its own."""
        assert 0 <= residue < ALIGN
        placed = []
        if fmt in ("rgb", "bgr", "y"):
            h, w = shape[0], shape[1]
            row_bytes = w * (1 if fmt == "y" else 3)
            pitch = row_bytes if pitch is None else pitch
            assert pitch >= row_bytes
            off = self._origin(residue)
            placed.append(Plane(off, pitch, h, row_bytes))
            self._cursor = off + _plane_extent(h, row_bytes, pitch) + self.gap
        elif fmt in ("rgb_planar", "bgr_planar"):
            _, h, w = shape
            pitch = w if pitch is None else pitch
            assert pitch >= w
            extent = _plane_extent(h, w, pitch)
            least = extent + self.gap
            plane_stride = least if plane_stride is None else plane_stride
            assert plane_stride >= least, (plane_stride, least)
            off = self._origin(residue)
            placed = [Plane(off + p * plane_stride, pitch, h, w) for p in range(3)]
            self._cursor = off + 2 * plane_stride + extent + self.gap
        elif fmt == "yuv_planar":
            planes = planes or [(None, 0)] * len(shape)
            assert len(planes) == len(shape)
            for (h, w), (ppitch, presidue) in zip(shape, planes):
                ppitch = w if ppitch is None else ppitch
                assert ppitch >= w
                off = self._origin(presidue)
                placed.append(Plane(off, ppitch, h, w))
                self._cursor = off + _plane_extent(h, w, ppitch) + self.gap
        else:
            raise ValueError(fmt)
        self.frames.append(Frame(name, fmt, tuple(shape) if fmt != "yuv_planar" else [tuple(s) for s in shape], placed))
        return len(self.frames) - 1

    @property
    def nbytes(self):
        return self._cursor - self.gap + self.tail if self.frames else self.lead + self.tail

    def rows(self):
        """every row of every plane: arrays (start, end exclusive, frame, plane, row), sorted by start"""
        rec = []
        for f, frame in enumerate(self.frames):
            for p, pl in enumerate(frame.planes):
                for y in range(pl.rows):
                    rec.append((pl.offset + y * pl.pitch, pl.offset + y * pl.pitch + pl.row_bytes, f, p, y))
        rec.sort()
        a = np.array(rec, dtype=np.int64).reshape(-1, 5)
        assert np.all(a[1:, 0] >= a[:-1, 1]), "outputs overlap"
        return a

    def owned(self):
        """bool mask over the arena: True where an output's byte lies"""
        m = np.zeros(self.nbytes, dtype=bool)
        for frame in self.frames:
            for pl in frame.planes:
                idx = pl.offset + np.arange(pl.rows)[:, None] * pl.pitch + np.arange(pl.row_bytes)[None, :]
                assert not m[idx].any(), "outputs overlap"
                m[idx] = True
        assert not m[:self.lead].any() and not m[self.nbytes - self.tail:].any()
        return m


def _plane_of(host, pl):
    return np.lib.stride_tricks.as_strided(host[pl.offset:], (pl.rows, pl.row_bytes), (pl.pitch, 1))


class Arena:
    """The tensor of a Layout, filled with `sentinel`, and the views the decoder writes through (outs: what BatchDecoder.decode takes
    as outs=)."""

    def __init__(self, layout, sentinel, device="cuda", torch=None):
        if torch is None:
            import torch
        self.layout, self.sentinel = layout, int(sentinel)
        # the residues a case chose are residues of the ADDRESS only if the arena starts on a multiple of ALIGN: allocate ALIGN bytes more
        # and start at the first such address (the bytes in front and behind are sentinels too, and checked)
        self._raw = torch.full((layout.nbytes + ALIGN,), self.sentinel, dtype=torch.uint8, device=device)
        self._shift = -self._raw.data_ptr() % ALIGN
        self.buf = self._raw[self._shift: self._shift + layout.nbytes]
        assert self.buf.data_ptr() % ALIGN == 0
        self.outs = []
        for frame in layout.frames:
            pl = frame.planes
            if frame.fmt in ("rgb", "bgr"):
                self.outs.append(self._view(frame.shape, (pl[0].pitch, 3, 1), pl[0].offset))
            elif frame.fmt == "y":
                self.outs.append(self._view(frame.shape, (pl[0].pitch, 1), pl[0].offset))
            elif frame.fmt == "yuv_planar":
                self.outs.append([self._view(s, (q.pitch, 1), q.offset) for s, q in zip(frame.shape, pl)])
            else:
                self.outs.append(self._view(frame.shape, (pl[1].offset - pl[0].offset, pl[0].pitch, 1), pl[0].offset))

    def _view(self, shape, strides, offset):
        return self._raw.as_strided(tuple(shape), strides, self._raw.storage_offset() + self._shift + offset)

    def host(self):
        """the arena's bytes on the host (one copy); the alignment slack around it must be untouched as well"""
        raw = self._raw.cpu().numpy()
        inner = raw[self._shift: self._shift + self.layout.nbytes]
        assert np.all(raw[:self._shift] == self.sentinel) and np.all(raw[self._shift + self.layout.nbytes:] == self.sentinel), "stray bytes outside the arena"
        return inner

    def decoded(self, host, index):
        """output `index` as the decoder's caller sees it: (H, W, 3), (3, H, W), (H, W) or a list of planes"""
        frame = self.layout.frames[index]
        planes = [_plane_of(host, pl).copy() for pl in frame.planes]
        if frame.fmt in ("rgb", "bgr"):
            return planes[0].reshape(frame.shape)
        if frame.fmt == "y":
            return planes[0]
        if frame.fmt == "yuv_planar":
            return planes
        return np.stack(planes)

    def check(self, expected, first=6):
        """expected: per output an array of the output's shape (a list of planes for yuv_planar), a Hashed, or None (not compared:
        an image the batch is known to refuse).  Raises AssertionError that lists wrong pixels and stray bytes."""
        layout = self.layout
        assert len(expected) == len(layout.frames)
        host = self.host()
        problems = []
        for i, (frame, want) in enumerate(zip(layout.frames, expected)):
            if want is None:
                continue
            got = self.decoded(host, i)
            if isinstance(want, Hashed):
                if hashlib.sha256(np.ascontiguousarray(want.canon(got)).tobytes()).hexdigest() != want.sha256:
                    problems.append("image %d (%s, %s): pixels do not hash to the golden value" % (i, frame.name, frame.fmt))
                continue
            gp = got if frame.fmt == "yuv_planar" else (list(got) if frame.fmt.endswith("_planar") else [got])
            wp = want if frame.fmt == "yuv_planar" else (list(want) if frame.fmt.endswith("_planar") else [want])
            assert len(gp) == len(wp), (frame.name, len(gp), len(wp))
            for p, (g, w) in enumerate(zip(gp, wp)):
                w = np.asarray(w)
                assert g.shape == w.shape, (frame.name, p, g.shape, w.shape)
                if not np.array_equal(g, w):
                    bad = np.argwhere(g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1))
                    problems.append("image %d (%s, %s) plane %d: %d wrong bytes, first at row %d byte %d" %
                                    (i, frame.name, frame.fmt, p, len(bad), bad[0][0], bad[0][1]))
        stray = np.flatnonzero((host != self.sentinel) & ~layout.owned())
        if stray.size:
            rows = layout.rows()
            prev = np.searchsorted(rows[:, 1], stray[:first], side="right") - 1  # the last row that ends at or before the byte
            for idx, k in zip(stray[:first], prev):
                if k < 0:
                    f, p, y = rows[0, 2:]
                    where = "in the lead, %d bytes before image %d (%s) plane %d row %d" % (rows[0, 0] - idx, f, layout.frames[f].name, p, y)
                else:
                    _, end, f, p, y = rows[k]
                    where = "image %d (%s) plane %d row %d, +%d bytes past the row's end" % (f, layout.frames[f].name, p, y, idx - end + 1)
                    if k + 1 == len(rows):
                        where += " (the tail)"
                    elif rows[k + 1, 2] != f:
                        where += " (between frames)"
                    elif rows[k + 1, 3] != p:
                        where += " (between planes)"
                problems.append("stray byte 0x%02X at arena offset %d: %s" % (host[idx], idx, where))
            problems.append("%d stray bytes in all (sentinel 0x%02X)" % (stray.size, self.sentinel))
        assert not problems, "\n".join(problems)
