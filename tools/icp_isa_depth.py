#!/usr/bin/env python3
"""Static instruction counts of the ICP loop kernel's ISA by loop depth, as tools/icp_isa.sh writes it (compile only, no
GPU): the compiler annotates every basic block with the loop it belongs to ("in Loop: Header=.. Depth=N", "Loop Header:
Depth=N"); instructions of blocks at depth >= D are counted -- all, vector (v_*), v_readlane_b32 and s_nop -- and, with
a list of spill lanes, the v_readlane_b32 that read them.
usage: tools/icp_isa_depth.py out.s [D = 2] [which icp_sweep_kernel of the file = 0] [vNN:lo-hi ...]"""
import collections
import re
import sys


def main():
    lines = open(sys.argv[1]).read().split('\n')
    dmin = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    which = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    lanes = []
    for a in sys.argv[4:]:
        reg, rng = a.split(':')
        lo, hi = rng.split('-')
        lanes.append((reg, int(lo), int(hi)))
    st = [i for i, l in enumerate(lines) if l.startswith('_Z16icp_sweep_kernel')][which]
    en = [i for i, l in enumerate(lines) if i > st and l.startswith('.Lfunc_end')][0]
    print(lines[st].split(':')[0][:64])
    depth = 0
    pending = False  # inside the comment lines of a block's head
    by_depth = collections.Counter()
    c = collections.Counter()
    for l in lines[st + 1:en]:
        s = l.strip()
        if not s:
            continue
        head = re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:)', s)
        if head:
            depth = 0
            pending = True
        if s.startswith(';') or head:
            if pending:
                m = re.search(r'(?:in Loop: Header=\S+|Loop Header:) Depth=(\d+)', s)
                if m:
                    depth = int(m.group(1))
            continue
        if s.startswith('.') or s.endswith(':'):
            continue
        pending = False
        op = s.split()[0]
        by_depth[depth] += 1
        if depth >= dmin:
            c['all'] += 1
            if op.startswith('v_'):
                c['vector'] += 1
            if op in ('v_readlane_b32', 's_nop'):
                c[op] += 1
            if op == 'v_readlane_b32' and lanes:
                m = re.match(r'v_readlane_b32\s+\S+\s+(v\d+),\s*(\d+)', s)
                if m and any(m.group(1) == r and lo <= int(m.group(2)) <= hi for r, lo, hi in lanes):
                    c['listed lanes'] += 1
    print('by depth:', ' '.join('%d:%d' % kv for kv in sorted(by_depth.items())))
    print('depth >= %d: instructions %d vector %d v_readlane %d s_nop %d%s' % (
        dmin, c['all'], c['vector'], c['v_readlane_b32'], c['s_nop'],
        (' | v_readlane of the listed lanes %d' % c['listed lanes']) if lanes else ''))


if __name__ == '__main__':
    main()
