"""Dev tool (CPU only): how much the first synchronisation launch of the GPU entropy stage walks under two schedules, on the bench's
sources -- a plain Python Huffman walk with a state walker, image-wide (the workgroups' halos are ignored: one group per image).

  current  pass 0: every subsequence from the assumed state (a block of MCU position 0 starts at its first bit); round 1: every
           subsequence again from its neighbour's end state (the decode that records); round 2: the successors of those whose end
           state moved in round 1
  paired   phase A: every second subsequence from the assumed state; phase B: the others from A's end state of the subsequence in
           front (subsequence 0 from the exact initial state); round 1: A's subsequences from B's end states; round 2: the successors
           of those whose end state moved in round 1

Per source and schedule: walks per bit (subsequence decodes / subsequences) by phase, the end states that are still wrong when round 2
is over, the tasks round 2 leaves (the tail kernel's first round), and the rounds the tail then needs to the fixpoint.  The fixpoint
is the same for both (checked): the states of the true trajectory.
usage: sync_schedule_model.py [source ...]   (profiles/sync_pairs/model.txt was made with it)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from walk_event_shares import decoder, segments

SUBSEQ_BITS = 1024


class Scan:
    def __init__(self, jpeg):
        tables, comps, _, scan, start = segments(jpeg)
        end = jpeg.rindex(b"\xff\xd9")
        raw = jpeg[start:end].replace(b"\xff\x00", b"\xff")
        self.total_bits = 8 * len(raw)
        self.raw = raw + b"\xff" * 8
        self.order = []
        for cid, td, ta in scan:
            h, v = next((h, v) for i, h, v in comps if i == cid)
            self.order += [(decoder(*tables[td]), decoder(*tables[0x10 | ta]))] * (h * v)
        self.nsub = -(-self.total_bits // SUBSEQ_BITS)
        self.memo = {}

    def walk(self, j, state):
        """Subsequence j from state (bit position, zigzag index, MCU position) -> the state at the first symbol that starts at or
        behind the subsequence's end.  A window that is no code (a walk through garbage) is taken as a 16-bit EOB."""
        key = (j, state)
        got = self.memo.get(key)
        if got is not None:
            return got
        pos, z, k = state
        limit = min((j + 1) * SUBSEQ_BITS, self.total_bits)
        raw, order, n = self.raw, self.order, len(self.order)
        while pos < limit:
            b = pos >> 3
            window = (int.from_bytes(raw[b:b + 4], "big") >> (16 - (pos & 7))) & 0xFFFF
            hit = order[k][0 if z == 0 else 1][window]
            length, sym = hit if hit else (16, 0)
            size = sym & 15
            pos += length + size
            z += 1 if z == 0 else (sym >> 4) + 1 if size else (16 if sym == 0xF0 else 64)
            if z >= 64:
                z = 0
                k = k + 1 if k + 1 < n else 0
        self.memo[key] = (pos, z, k)
        return pos, z, k


def run(scan, paired):
    ns = scan.nsub
    assumed = lambda j: (j * SUBSEQ_BITS, 0, 0)
    front = lambda j, end: end[j - 1] if j else (0, 0, 0)
    truth = [None] * ns
    for j in range(ns):
        truth[j] = scan.walk(j, front(j, truth))
    end, phases = [None] * ns, []
    if paired:
        a = list(range(1, ns, 2))
        for j in a:
            end[j] = scan.walk(j, assumed(j))
        b = list(range(0, ns, 2))
        for j in b:
            end[j] = scan.walk(j, front(j, end))
        phases += [len(a), len(b)]
        tasks = a
    else:
        for j in range(ns):
            end[j] = scan.walk(j, assumed(j) if j else (0, 0, 0))
        phases.append(ns)
        tasks = list(range(1, ns))
    rounds, wrong, tail, tail_rounds = 0, None, None, 0
    while tasks:
        rounds += 1
        if rounds <= 2:
            phases.append(len(tasks))
        else:
            tail_rounds += 1
        starts = [end[j - 1] for j in tasks]   # Jacobi: start states as they were before the round
        moved = []
        for j, s in zip(tasks, starts):
            now = scan.walk(j, s)
            if now != end[j] and j + 1 < ns:
                moved.append(j + 1)
            end[j] = now
        tasks = moved
        if rounds == 2:
            wrong, tail = sum(1 for j in range(ns) if end[j] != truth[j]), len(tasks)
    assert end == truth, "the schedule's fixpoint is not the true trajectory"
    if wrong is None:   # (done before round 2 was over)
        wrong, tail = 0, 0
    return phases, wrong, tail, tail_rounds


if __name__ == "__main__":
    sources, what = bench.make_inputs()
    print(what)
    pick = [int(a) for a in sys.argv[1:]] or range(len(sources))
    for s in pick:
        scan = Scan(sources[s])
        print("source %d: %d subsequences" % (s, scan.nsub))
        for name, paired in (("current", False), ("paired", True)):
            phases, wrong, tail, tail_rounds = run(scan, paired)
            ns = scan.nsub
            print("  %-8s walks per bit %s = %.3f; end states wrong before the tail %.1f %%; tasks for the tail's first round %.1f %% of all "
                  "subsequences; %d tail rounds to the fixpoint" % (name, " + ".join("%.3f" % (p / ns) for p in phases), sum(phases) / ns,
                                                                     100 * wrong / ns, 100 * tail / ns, tail_rounds))
