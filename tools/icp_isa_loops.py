#!/usr/bin/env python3
"""Innermost loops of the ICP loop kernel's ISA that come from a given range of source lines (compile only, no GPU).
Input: a .s of tools/icp_isa.sh built with line tables (tools/icp_isa.sh out.s -gline-tables-only).  The compiler marks
the head of every innermost loop ("This Inner Loop Header: Depth=N") and every other block of it ("in Loop: Header=BBx_y");
every instruction is attributed to the last `.loc` before it, whose comment also carries the chain of calls it was inlined
through ("@[ file:line:col @[ ... ] ]").  For every innermost loop with at least `--min-share` of its instructions in
LO-HI of the source file the tool prints, in the order of the file: its head, depth, instruction and vector-instruction
(v_*) counts, how many of them lie in the range, the call lines it was inlined through (outermost last; the most frequent
chain of the loop's instructions) and, with --mark A-B, how many of its instructions come from lines A-B (e.g. the lines
that maintain the runner-up distance: which of two instances of a body a loop belongs to).
usage: tools/icp_isa_loops.py out.s LO-HI [--kernel K = 0] [--file NAME = sfe_icp_sweep_loop.hip] [--min-share S = 0.5]
                              [--symbol PREFIX = _Z16icp_sweep_kernel]  (another file's kernel: its mangled name's beginning,
                              e.g. --file sfe_icp3.hip --symbol _Z15icp3_job_kernelILi3ELi0E)
                              [--mark A-B] [--max-insts N --max-vector M [--unmarked-only]]
With --max-insts / --max-vector the exit status is 1 if a listed loop (with --unmarked-only: one without marked
instructions) is larger, or if nothing is listed."""
import argparse
import collections
import re
import sys


def span(s):
    lo, hi = s.split('-')
    return int(lo), int(hi)


def loops_of(lines, which, fname, symbol='_Z16icp_sweep_kernel'):
    """-> [dict(head, depth, insts, vector, lines Counter, chains Counter)] of the which-th kernel whose name begins with symbol"""
    st = [i for i, l in enumerate(lines) if l.startswith(symbol)][which]
    en = [i for i, l in enumerate(lines) if i > st and l.startswith('.Lfunc_end')][0]
    files = {}                # (the file table is the translation unit's: its entries stand wherever they were first needed)
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = m.group(2).split('/')[-1]
    loops = collections.OrderedDict()
    cur = None                # the innermost loop the current block belongs to (None: not in one)
    head_label, in_head = None, False
    line, chain = None, ()
    for l in lines[st:en]:
        s = l.strip()
        if not s:
            continue
        m = re.match(r'\.loc\s+(\d+)\s+(\d+)\s+\d+', s)
        if m:
            line = int(m.group(2)) if files.get(int(m.group(1))) == fname else None
            chain = tuple(int(x) for x in re.findall(r'@\[ [^:\s]+:(\d+):\d+', s))
            continue
        m = re.match(r'^\.LBB(\d+_\d+):', s)
        if m or re.match(r'^; %bb\.\d+:', s):
            head_label, in_head, cur = (m.group(1) if m else None), True, None
        if s.startswith(';') or m:
            if in_head:
                h = re.search(r'in Loop: Header=BB(\d+_\d+) Depth=(\d+)', s)
                if h and h.group(1) in loops:
                    cur = h.group(1)
                h = re.search(r'This Inner Loop Header: Depth=(\d+)', s)
                if h and head_label:
                    cur = head_label
                    loops[cur] = dict(head='.LBB' + cur, depth=int(h.group(1)), insts=0, vector=0,
                                      lines=collections.Counter(), chains=collections.Counter())
            continue
        if s.startswith('.') or s.endswith(':'):
            continue
        in_head = False
        if cur is None:
            continue
        lp = loops[cur]
        lp['insts'] += 1
        lp['vector'] += s.split()[0].startswith('v_')
        lp['lines'][line] += 1
        lp['chains'][chain] += 1
    return lines[st].split(':')[0][:64], list(loops.values())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('asm')
    ap.add_argument('range', type=span)
    ap.add_argument('--kernel', type=int, default=0)
    ap.add_argument('--file', default='sfe_icp_sweep_loop.hip')
    ap.add_argument('--symbol', default='_Z16icp_sweep_kernel')
    ap.add_argument('--min-share', type=float, default=0.5)
    ap.add_argument('--mark', type=span)
    ap.add_argument('--max-insts', type=int)
    ap.add_argument('--max-vector', type=int)
    ap.add_argument('--unmarked-only', action='store_true')
    a = ap.parse_args()
    name, loops = loops_of(open(a.asm).read().split('\n'), a.kernel, a.file, a.symbol)
    print(name)
    lo, hi = a.range
    shown, bad = 0, 0
    for lp in loops:
        inr = sum(n for ln, n in lp['lines'].items() if ln is not None and lo <= ln <= hi)
        if lp['insts'] == 0 or inr < a.min_share * lp['insts']:
            continue
        shown += 1
        chain = lp['chains'].most_common(1)[0][0]
        txt = '%-12s depth %d: instructions %4d vector %4d | in %d-%d: %4d | inlined at %s' % (
            lp['head'], lp['depth'], lp['insts'], lp['vector'], lo, hi, inr, ' <- '.join(map(str, chain)) or '-')
        marked = 0
        if a.mark:
            marked = sum(n for ln, n in lp['lines'].items() if ln is not None and a.mark[0] <= ln <= a.mark[1])
            txt += ' | in %d-%d: %d' % (a.mark[0], a.mark[1], marked)
        gated = not (a.unmarked_only and marked)
        if gated and ((a.max_insts is not None and lp['insts'] > a.max_insts) or
                      (a.max_vector is not None and lp['vector'] > a.max_vector)):
            bad += 1
            txt += ' | OVER'
        print(txt)
    print('%d innermost loops of %d listed' % (shown, len(loops)))
    if a.max_insts is not None or a.max_vector is not None:
        sys.exit(1 if bad or not shown else 0)


if __name__ == '__main__':
    main()
