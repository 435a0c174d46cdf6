"""Dev tool: reads rocprofv3 output directories of tools/prof_gh.py runs under DIR.
DIR/*_1, *_2, *_3 (--kernel-trace --stats of `prof_gh.py 20`): per kernel of the GPU entropy stage mean / min / max over the
dispatches, the trace's LDS and VGPR columns -> summary.txt in each directory.
DIR/*_timeline (--kernel-trace --memory-copy-trace of `prof_gh.py 20 256 steps`): the time from the end of a batch's last entropy kernel to
the start of idct_plane_kernel, and the kernels and copies around the stage's end in the last step -> timeline.txt.
usage: gh_trace_summary.py DIR   (profiles/entropy_residue/ was made with it)"""
import csv, glob, os, sys
root = sys.argv[1]
NAMES = ["destuff_compact_kernel", "huff_sync_kernel", "huff_sync_pair_kernel", "huff_tail_kernel<false>", "huff_tail_kernel<true>", "huff_scan_kernel",
         "huff_copy_records_kernel", "huff_pos_kernel", "huff_blocks_kernel", "huff_dc_group_kernel"]
def short(n):
    n = n.replace('(anonymous namespace)::', '').replace('hipjpeg::', '')
    return n.split('(')[0].replace('void ', '').strip()
def find(d, pat):
    g = glob.glob(os.path.join(d, '**', pat), recursive=True)
    return g[0] if g else None
for d in sorted(glob.glob(os.path.join(root, '*_[123]'))):
    f = find(d, '*kernel_trace.csv')
    if not f: continue
    per = {}
    for r in csv.DictReader(open(f)):
        per.setdefault(short(r['Kernel_Name']), []).append(((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3, r.get('LDS_Block_Size', '?'), r.get('VGPR_Count', '?')))
    lines, tot = [], 0.0
    for n in NAMES:
        if n not in per: continue
        v = [x[0] for x in per[n]]
        tot += sum(v) / len(v)
        lines.append("%-28s n=%3d mean %8.1f us  min %8.1f  max %8.1f  lds %s vgpr %s" % (n, len(v), sum(v) / len(v), min(v), max(v), per[n][0][1], per[n][0][2]))
    lines.append("sum of means %.1f us" % tot)
    open(os.path.join(d, 'summary.txt'), 'w').write("\n".join(lines) + "\n")
    print("==", os.path.basename(d)); print("\n".join(lines))
for d in sorted(glob.glob(os.path.join(root, '*_timeline'))):
    f = find(d, '*kernel_trace.csv')
    if not f: continue
    ev = []
    for r in csv.DictReader(open(f)):
        ev.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])[:26]))
    m = find(d, '*memory_copy_trace.csv')
    if m:
        for r in csv.DictReader(open(m)):
            ev.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), 'COPY ' + r.get('Direction', '')[-14:]))
    ev.sort()
    gaps, last_ent = [], None
    for i, (s, e, n) in enumerate(ev):
        if n.startswith('huff_dc'): last_ent = (i, e)
        if n.startswith('idct_plane') and last_ent:
            gaps.append(((s - last_ent[1]) / 1e3, last_ent[0], i))
            last_ent = None
    g = [x[0] for x in gaps]
    out = ["gap from the end of the last entropy kernel to the start of idct_plane_kernel: n=%d median %.1f us  mean %.1f  min %.1f  max %.1f" % (len(g), sorted(g)[len(g) // 2], sum(g) / len(g), min(g), max(g))] if g else ["no gaps found"]
    if gaps:
        _, a, b = gaps[-1]
        t0 = ev[max(a - 3, 0)][0]
        out.append("last step, around the stage's end (us from the first line's start):")
        for s, e, n in ev[max(a - 3, 0):b + 2]:
            out.append("  %9.1f .. %9.1f  %7.1f  %s" % ((s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, n))
    open(os.path.join(d, 'timeline.txt'), 'w').write("\n".join(out) + "\n")
    print("==", os.path.basename(d)); print("\n".join(out))
