"""Issue-slot census of one kernel's ISA: what the vector issue slots of a step are spent on, by mnemonic class.

    python profiles/tools/slot_census.py kernel.s [--trips 4] [--weight LABEL=N ...] [--blocks]

kernel.s is ONE kernel cut out of hipcc -S output (or a one-kernel unit, profiles/tools/README.md), product or
-DATACOM_MARKS build.  The ISA is cut into regions at labels and branches; a region inside an inner loop (from the label
the compiler annotates "Inner Loop Header" to the backward branch to it) is weighted by --trips (the four physics
sub-steps), every other region by 1; --weight LABEL=N overrides one region (N = 0 for a path the headline run does not
take: the tool cannot know which side of a uniform branch runs).  --blocks lists the regions with their weights so that
the weighted total can be reconciled with SQ_INSTS_VALU per wave.  With MARK comments present the sections are listed too.

Every class is priced with the lone-wave issue costs of profiles/r01_issue_costs.md (clocks per instruction).  The tool
classifies by mnemonic class only -- it names no single instruction beyond the classes of the table.
"""
import argparse
import collections
import re

# class -> clocks per instruction (profiles/r01_issue_costs.md; the row used is named beside each)
PRICE = collections.OrderedDict([
    ('packed fma/mul/add', 5.2),    # v_pk_fma_f32, 2 independent chains (dependent 5.6, 4 independent 5.1)
    ('plain arithmetic', 4.8),      # v_fma_f32: between 4 independent chains (4.1) and a dependent chain (5.5)
    ('transcendental', 8.5),        # v_rcp_f32 dependent
    ('dpp add', 5.1),               # v_add_f32_dpp, 4 independent
    ('dpp move', 5.1),              # priced as the DPP add: the same issue path
    ('moves and selects', 5.3),     # v_cndmask_b32 dependent (4.3 behind its compare)
    ('accvgpr', 4.2),               # v_accvgpr_write_b32 + v_accvgpr_read_b32, each
    ('s_nop 0', 4.7),
    ('s_nop 1', 8.7),
    ('s_nop >1', 12.7),             # not measured: s_nop 1 plus one more issue slot
    ('rest of valu', 4.3),          # compares, conversions, integer and bit operations: v_cmp_*_e64 behind a select
])
NON_ARITH = ('dpp move', 'moves and selects', 'accvgpr', 's_nop 0', 's_nop 1', 's_nop >1')
TRANS = ('v_rcp', 'v_rsq', 'v_sqrt', 'v_sin', 'v_cos', 'v_exp', 'v_log')
ARITH = ('v_fma', 'v_fmac', 'v_mac', 'v_mad', 'v_mul', 'v_add', 'v_sub', 'v_max', 'v_min', 'v_med3', 'v_ldexp', 'v_fract',
         'v_floor', 'v_trunc', 'v_rndne', 'v_ceil')


def classify(line):
    """Class of one ISA line, or None for what is no vector issue slot (scalar, memory, waits, directives)."""
    t = line.strip().split()
    if not t or t[0][0] in '.;/' or t[0].endswith(':'):
        return None
    op = t[0]
    if op == 's_nop':
        n = int(t[1], 0)
        return 's_nop 0' if n == 0 else 's_nop 1' if n == 1 else 's_nop >1'
    if not op.startswith('v_'):
        return None
    dpp = op.endswith('_dpp') or 'quad_perm' in line or ' row_' in line
    if op.startswith('v_accvgpr'):
        return 'accvgpr'
    if dpp:
        return 'dpp move' if op.startswith('v_mov') else 'dpp add'
    if op.startswith(('v_mov', 'v_pk_mov', 'v_cndmask', 'v_readlane', 'v_readfirstlane', 'v_writelane', 'v_swap')):
        return 'moves and selects'
    if op.startswith('v_pk_'):
        return 'packed fma/mul/add'
    if op.startswith(TRANS):
        return 'transcendental'
    if op.startswith(ARITH) and not re.search(r'_[iu](16|32|64)|_co_', op):
        return 'plain arithmetic'
    return 'rest of valu'


def regions(lines):
    """[(name, in_loop, Counter of classes, [(mark, Counter)])] in program order."""
    out, cur, cnt, loop_hdr, in_loop, n = [], 'entry', collections.Counter(), None, False, 0
    mark, marks = '(unmarked)', collections.OrderedDict()

    def close(name):
        nonlocal cnt
        if cnt:
            out.append((name, in_loop, cnt))
        cnt = collections.Counter()

    for l in lines:
        m = re.match(r'^(\.LBB\S+):', l)
        if m:
            close(cur)
            cur = m.group(1)
            if 'Inner Loop Header' in l:
                loop_hdr, in_loop = cur, True
            continue
        mm = re.search(r'; MARK (\S+)', l)
        if mm:
            mark = mm.group(1)
            continue
        t = l.strip().split()
        if t and t[0].startswith(('s_cbranch', 's_branch', 's_endpgm')):
            close(cur)
            n += 1
            if in_loop and len(t) > 1 and t[1] == loop_hdr:
                in_loop = False
            cur = '%s+%d' % (cur.split('+')[0], n)
            continue
        c = classify(l)
        if c:
            cnt[c] += 1
            marks.setdefault(mark, [in_loop, collections.Counter()])[1][c] += 1
    close(cur)
    return out, marks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('isa')
    ap.add_argument('--trips', type=int, default=4, help='executions of an inner loop body per step')
    ap.add_argument('--weight', action='append', default=[], metavar='LABEL=N')
    ap.add_argument('--blocks', action='store_true', help='list the regions and their weights')
    ap.add_argument('--clocks', type=float, default=56.2e3, help='measured clocks per wave per step the classes are set against')
    a = ap.parse_args()
    over = {k: int(v) for k, v in (w.split('=') for w in a.weight)}
    regs, marks = regions(open(a.isa).read().split('\n'))
    static, executed, loop1 = collections.Counter(), collections.Counter(), collections.Counter()
    if a.blocks:
        print('| region | weight | issue slots | s_nop |\n|---|---|---|---|')
    for name, in_loop, cnt in regs:
        w = over.get(name, a.trips if in_loop else 1)
        if a.blocks:
            print('| %s%s | %d | %d | %d |' % (name, ' (loop)' if in_loop else '', w, sum(cnt.values()),
                                              sum(v for k, v in cnt.items() if k.startswith('s_nop'))))
        for k, v in cnt.items():
            static[k] += v
            executed[k] += w * v
            if in_loop:
                loop1[k] += v
    nv = lambda c: sum(v for k, v in c.items() if not k.startswith('s_nop'))
    tot_clk = sum(PRICE[k] * v for k, v in executed.items())
    print('\nvector instructions: static %d, one pass of the loop body %d, executed per step %d (+ %d s_nop)'
          % (nv(static), nv(loop1), nv(executed), sum(executed.values()) - nv(executed)))
    print('priced total %.1f k clocks of %.1f k measured (%.0f %%)\n' % (tot_clk / 1e3, a.clocks / 1e3, 100 * tot_clk / a.clocks))
    print('| class | static | loop body | executed | clk each | clocks | % of measured |\n|---|---|---|---|---|---|---|')
    for k in PRICE:
        if static[k]:
            print('| %s | %d | %d | %d | %.1f | %.0f | %.1f |' % (k, static[k], loop1[k], executed[k], PRICE[k],
                                                                  PRICE[k] * executed[k], 100 * PRICE[k] * executed[k] / a.clocks))
    print('\nnon-arithmetic classes by clocks:')
    for k in sorted(NON_ARITH, key=lambda k: -PRICE[k] * executed[k]):
        if executed[k]:
            print('  %-18s %6d executed  %7.0f clk  %4.1f %%' % (k, executed[k], PRICE[k] * executed[k],
                                                                100 * PRICE[k] * executed[k] / a.clocks))
    if len(marks) > 1:
        print('\n| section | loop | issue slots | dpp add | dpp move | moves and selects | accvgpr | s_nop 0 | s_nop 1 |\n|---|---|---|---|---|---|---|---|---|')
        for name, (in_loop, c) in marks.items():
            print('| %s | %s | %d | %d | %d | %d | %d | %d | %d |' % (name, 'x%d' % a.trips if in_loop else '', sum(c.values()), c['dpp add'],
                                                                    c['dpp move'], c['moves and selects'], c['accvgpr'], c['s_nop 0'], c['s_nop 1']))


if __name__ == '__main__':
    main()
