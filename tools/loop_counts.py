#!/usr/bin/env python3
"""Loops of one kernel of a device-only assembly listing (hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only file.hip -o file.s):
vector, scalar, LDS and global instruction counts between every label and a backward branch to it, and how many labels lie inside
(0 or 1: an innermost loop).  usage: loop_counts.py file.s kernel_name_substring
The walk loops of huff_sync_kernel are the ones with 3 LDS instructions and no global one (profiles/walk_step_diet/README.md)."""
import re, sys
s = open(sys.argv[1]).read()
want = sys.argv[2]
for m in re.finditer(r'^(\S*' + re.escape(want) + r'\S*):[^\n]*\n(.*?)\.Lfunc_end', s, re.S | re.M):
    name, body = m.group(1), m.group(2)
    lines = body.split('\n')
    labels = {}
    for i, l in enumerate(lines):
        lm = re.match(r'^(\.LBB\d+_\d+):', l)
        if lm:
            labels[lm.group(1)] = i
    print(name[:80])
    for i, l in enumerate(lines):
        bm = re.match(r'^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)', l) or re.match(r'^\s+s_branch\s+(\.LBB\d+_\d+)', l)
        if bm and bm.group(1) in labels and labels[bm.group(1)] < i:
            a = labels[bm.group(1)]
            seg = lines[a:i + 1]
            inner = sum(1 for x in seg[1:] if re.match(r'^\.LBB', x))
            v = sum(1 for x in seg if re.match(r'^\s+v_', x))
            sc = sum(1 for x in seg if re.match(r'^\s+s_', x))
            ds = sum(1 for x in seg if re.match(r'^\s+ds_', x))
            gl = sum(1 for x in seg if re.match(r'^\s+(global|flat|buffer)_', x))
            print(f"  loop {bm.group(1):12s} lines {a}-{i} labels_inside {inner} valu {v} salu {sc} lds {ds} global {gl}")
