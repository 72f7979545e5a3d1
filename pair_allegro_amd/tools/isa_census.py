"""Static census of a kernel's ISA between barriers: spill traffic, MFMA, VALU, LDS, waits per barrier interval.
usage: python isa_census.py file.s mangled_kernel_name_substring
       python isa_census.py file.s mangled_kernel_name_substring --by-opcode [--taken LABEL[,LABEL...]] [--top N]

--by-opcode: the VALU instructions of the TILE LOOP (the smallest backward-branch span that holds every MFMA, as in isa_vmcnt.py) by class and by mnemonic,
per barrier interval, twice: for the whole static body of the loop, and for ONE EXECUTED PATH through it.  The path is walked block by block: an unconditional
forward branch is followed, a conditional branch falls through unless its target is named in --taken (a backward branch is never followed: an inner loop counts
once).  Every conditional branch of the loop is listed with its decision and with what lies between it and its target, so that the arms of a wave-uniform switch
(k_fused: the per-edge and the per-centre form of the environment backward) can be told apart and chosen.  A census, not a proof: no values are tracked.
Classes: trans (v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos), cvt (v_cvt_*), mov (v_mov_*, v_accvgpr_*), perm (v_perm*, v_bfi / v_alignbit / v_swap),
mix (v_fma_mix*), pk_f32 (v_pk_*_f32), f32 (unpacked float32 arithmetic), cmp (v_cmp*, v_cndmask), other (integer, logic, 16-bit packed)."""
import re
import sys
from collections import Counter

lines = open(sys.argv[1]).read().split('\n')
key = sys.argv[2]
start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and key in l and l.rstrip().endswith(':') or (l.startswith('_Z') and key in l and '; @' in l))
end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))


def instr(l):
    """the instruction text of an assembly line, or None for labels, directives, comments and blanks"""
    t = l.split(';')[0].strip()
    if not t or t.startswith('.') or t.endswith(':'):
        return None
    return t


def plain():
    body = lines[start:end]
    iv = []
    cur = dict(n=0, mfma=0, valu=0, sst=0, sld=0, ds=0, buf=0, vm0=0, wl=0)
    tot = dict(cur)
    for l in body:
        t = l.strip()
        if not t or t.startswith(';') or t.startswith('.') or t.endswith(':'):
            continue
        op = t.split()[0]
        cur['n'] += 1
        if op.startswith('v_mfma'): cur['mfma'] += 1
        elif op.startswith('v_readlane') or op.startswith('v_writelane'): cur['wl'] += 1
        elif op.startswith('v_'): cur['valu'] += 1
        elif op.startswith('scratch_store'): cur['sst'] += 1
        elif op.startswith('scratch_load'): cur['sld'] += 1
        elif op.startswith('ds_'): cur['ds'] += 1
        elif op.startswith('buffer_'): cur['buf'] += 1
        elif op == 's_waitcnt' and 'vmcnt(0)' in t: cur['vm0'] += 1
        if op == 's_barrier':
            iv.append(cur); cur = dict.fromkeys(cur, 0)
    iv.append(cur)
    print('interval  instr  mfma  valu  lane  sc_st  sc_ld    ds   buf  vmcnt0')
    for i, c in enumerate(iv):
        print(f"{i:7d} {c['n']:6d} {c['mfma']:5d} {c['valu']:5d} {c['wl']:5d} {c['sst']:6d} {c['sld']:6d} {c['ds']:5d} {c['buf']:5d} {c['vm0']:6d}")
        for k in tot: tot[k] += c[k]
    print('total  ', tot)


CLASSES = ('trans', 'cvt', 'mov', 'perm', 'mix', 'pk_f32', 'f32', 'cmp', 'other')
TRANS = re.compile(r'^v_(exp|log|rcp|rsq|sqrt|sin|cos)_')
F32 = re.compile(r'^v_(add|sub|subrev|mul|fma|fmac|mac|mad|max|min|max3|min3|med3|ldexp|fract|floor|ceil|trunc|rndne|frexp_mant|div_scale|div_fmas|div_fixup|mul_legacy)_f32')


def strip_enc(op):
    return re.sub(r'_(e32|e64|sdwa|dpp|e64_dpp)$', '', op)


def classify(op):
    if TRANS.match(op): return 'trans'
    if op.startswith('v_cvt_'): return 'cvt'
    if op.startswith('v_mov_') or op.startswith('v_accvgpr_'): return 'mov'
    if op.startswith(('v_perm', 'v_bfi', 'v_alignbit', 'v_alignbyte', 'v_swap')): return 'perm'
    if op.startswith('v_fma_mix'): return 'mix'
    if op.startswith('v_pk_') and op.endswith('_f32'): return 'pk_f32'
    if F32.match(op): return 'f32'
    if op.startswith(('v_cmp', 'v_cndmask')): return 'cmp'
    return 'other'


def by_opcode(taken, top):
    labels = {}
    for i in range(start, end):
        m = re.match(r'^(\.LBB\d+_\d+):', lines[i])
        if m: labels[m.group(1)] = i
    mf = [i for i in range(start, end) if (instr(lines[i]) or '').startswith('v_mfma')]
    loop = None
    for i in range(start, end):
        t = instr(lines[i]) or ''
        if t.startswith(('s_cbranch', 's_branch')):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] < i and labels[tgt] <= mf[0] and i >= mf[-1]:
                if loop is None or (i - labels[tgt]) < (loop[1] - loop[0]): loop = (labels[tgt], i)
    if loop is None:
        sys.exit('no backward branch around the MFMAs: not a tile loop')

    def span(a, b):
        """(instructions, MFMAs, VALU, buffer operations) of lines a..b-1"""
        n = m = v = bu = 0
        for i in range(a, b):
            t = instr(lines[i])
            if t is None: continue
            op = t.split()[0]
            n += 1
            if op.startswith('v_mfma'): m += 1
            elif op.startswith('v_') and not op.startswith(('v_readlane', 'v_writelane')): v += 1
            elif op.startswith('buffer_'): bu += 1
        return n, m, v, bu

    def walk(follow):
        iv = [dict(n=0, mfma=0, buf=0, cls=Counter(), ops=Counter())]
        decisions = []
        i = loop[0]
        while i <= loop[1]:
            t = instr(lines[i])
            if t is None:
                i += 1
                continue
            op = t.split()[0]
            c = iv[-1]
            c['n'] += 1
            if op.startswith('v_mfma'): c['mfma'] += 1
            elif op.startswith('buffer_'): c['buf'] += 1
            elif op.startswith('v_') and not op.startswith(('v_readlane', 'v_writelane')):
                o = strip_enc(op)
                c['cls'][classify(o)] += 1
                c['ops'][o] += 1
            if op == 's_barrier': iv.append(dict(n=0, mfma=0, buf=0, cls=Counter(), ops=Counter()))
            if follow and op.startswith(('s_cbranch', 's_branch')):
                tgt = t.split()[-1]
                j = labels.get(tgt)
                fwd = j is not None and i < j <= loop[1]
                if op == 's_branch':
                    if fwd:
                        i = j
                        continue
                elif fwd:
                    go = tgt in taken
                    decisions.append((i + 1, op, tgt, go, span(i + 1, j)))
                    if go:
                        i = j
                        continue
            i += 1
        return iv, decisions

    def table(title, iv):
        print(title)
        print('interval  instr  mfma   buf  valu ' + ' '.join(f'{k:>6s}' for k in CLASSES))
        tot = dict(n=0, mfma=0, buf=0, cls=Counter(), ops=Counter())
        for k, c in enumerate(iv):
            print(f"{k:7d} {c['n']:6d} {c['mfma']:5d} {c['buf']:5d} {sum(c['cls'].values()):5d} " + ' '.join(f"{c['cls'][x]:6d}" for x in CLASSES))
            for x in ('n', 'mfma', 'buf'): tot[x] += c[x]
            tot['cls'] += c['cls']; tot['ops'] += c['ops']
        print(f"  total {tot['n']:6d} {tot['mfma']:5d} {tot['buf']:5d} {sum(tot['cls'].values()):5d} " + ' '.join(f"{tot['cls'][x]:6d}" for x in CLASSES))
        return tot

    print(f'{key}: tile loop = lines {loop[0] + 1}..{loop[1] + 1} of {sys.argv[1].split("/")[-1]}')
    st, _ = walk(False)
    table('== static body of the tile loop (every arm of every branch)', st)
    ex, dec = walk(True)
    print('== conditional forward branches met on the executed path: line, branch, target, decision, (instructions, MFMAs, VALU, buffer operations) it jumps over')
    for ln, op, tgt, go, sp in dec:
        print(f"{ln:7d} {op:18s} {tgt:12s} {'TAKEN' if go else 'falls through'}  {sp}")
    tot = table('== executed path' + (' (--taken ' + ','.join(sorted(taken)) + ')' if taken else ' (every conditional branch falls through)'), ex)
    print('== executed path: VALU instructions by mnemonic per barrier interval' + (f' (the {top} most frequent)' if top else ''))
    for k, c in enumerate(ex):
        items = c['ops'].most_common(top or None)
        print(f'{k:7d} ' + '  '.join(f'{o}:{n}' for o, n in items))
    print('== executed path: VALU instructions by mnemonic, whole tile loop')
    for o, n in tot['ops'].most_common():
        print(f'{n:6d}  {classify(o):7s} {o}')


if '--by-opcode' in sys.argv[3:]:
    a = sys.argv[3:]
    tk = set(a[a.index('--taken') + 1].split(',')) if '--taken' in a else set()
    tp = int(a[a.index('--top') + 1]) if '--top' in a else 12
    by_opcode(tk, tp)
else:
    plain()
