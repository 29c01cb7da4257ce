#!/usr/bin/env python3
"""Static instruction mix of a marked region of the ICP loop kernel's ISA, as tools/icp_isa.sh writes it (compile only, no
GPU): the region between `asm volatile("; NAME_BEGIN")` and `; NAME_END`, whole and split at its first cross-lane move
(v_mov_b32_dpp / v_permlane*): for the SUMS region that is the two per-minimiser loops, and the reduction with the stores
and the cross-wave pass behind them.
usage: tools/icp_isa_region.py out.s [NAME = SUMS] [which icp_sweep_kernel of the file = 0]"""
import collections
import sys


def mix(name, ls):
    c = collections.Counter()
    for l in ls:
        l = l.strip()
        if l and not l.startswith((';', '.')) and not l.endswith(':'):
            c[l.split()[0]] += 1

    def n(pred):
        return sum(v for k, v in c.items() if pred(k))
    print('%s: instructions %d VALU %d fp64 %d v_readlane %d dpp %d v_mov_b32 %d v_cndmask %d v_permlane %d s_nop %d scratch %d ds %d' % (
        name, sum(c.values()), n(lambda k: k.startswith('v_')), n(lambda k: k.endswith('_f64') or '_f64_' in k),
        c['v_readlane_b32'], n(lambda k: 'dpp' in k), c['v_mov_b32_e32'], n(lambda k: 'cndmask' in k),
        n(lambda k: 'permlane' in k), c['s_nop'], n(lambda k: k.startswith('scratch_')), n(lambda k: k.startswith('ds_'))))


def main():
    lines = open(sys.argv[1]).read().split('\n')
    name = sys.argv[2] if len(sys.argv) > 2 else 'SUMS'
    which = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    st = [i for i, l in enumerate(lines) if l.startswith('_Z16icp_sweep_kernel')][which]
    en = [i for i, l in enumerate(lines) if i > st and l.startswith('.Lfunc_end')][0]
    body = lines[st:en]
    print(lines[st].split(':')[0][:64])
    b = [i for i, l in enumerate(body) if name + '_BEGIN' in l][0]
    e = [i for i, l in enumerate(body) if name + '_END' in l][0]
    reg = body[b:e]
    mix('region', reg)
    first = [i for i, l in enumerate(reg) if '_dpp' in l or 'permlane' in l]
    if first:
        mix('before the first cross-lane move', reg[:first[0]])
        mix('from the first cross-lane move', reg[first[0]:])


if __name__ == '__main__':
    main()
