"""Static census of the vector-memory waits of a kernel's TILE LOOP (sibling of isa_census.py).
usage: python isa_vmcnt.py file.s mangled_kernel_name_substring [--sites]

The tile loop is the smallest backward-branch span that holds every MFMA of the function.  Printed for it:
  - the number of `s_waitcnt vmcnt(N)` by N (a wait with a small N behind a young load drains the in-order queue);
  - the number of register copies (v_mov_b32 / v_mov_b64) whose source was written by a vector-memory load and has not been read by anything else: the
    load did not land where its value lives, and the copy sits behind a wait for that load;
  - with --sites: every wait with N <= 3, its line in the file, the youngest vector-memory instruction in front of it and the distance in instructions.
The scan is linear (no control flow): a census, not a proof."""
import re
import sys
from collections import Counter

path, key = sys.argv[1], sys.argv[2]
sites = '--sites' in sys.argv[3:]
lines = open(path).read().split('\n')
start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and key in l and (l.rstrip().endswith(':') or '; @' in l))
end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))

labels = {}
for i in range(start, end):
    m = re.match(r'^(\.LBB\d+_\d+):', lines[i])
    if m:
        labels[m.group(1)] = i
mf = [i for i in range(start, end) if lines[i].strip().startswith('v_mfma')]
loop = None
for i in range(start, end):
    t = lines[i].strip()
    if t.startswith('s_cbranch') or t.startswith('s_branch'):
        tgt = t.split()[-1]
        if tgt in labels and labels[tgt] < i and labels[tgt] <= mf[0] and i >= mf[-1]:
            if loop is None or (i - labels[tgt]) < (loop[1] - loop[0]):
                loop = (labels[tgt], i)
if loop is None:
    sys.exit('no backward branch around the MFMAs: not a tile loop')

REG = re.compile(r'\bv\[(\d+):(\d+)\]|\bv(\d+)\b')


def regs(tok):
    out = []
    for m in REG.finditer(tok):
        if m.group(3) is not None:
            out.append(int(m.group(3)))
        else:
            out.extend(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


waits = Counter()
copies = 0
loaded = set()          # registers written by a vector-memory load and not touched since
ninstr = nmfma = nvmem = 0
last_vmem = None        # (instruction index, text)
site_rows = []
for i in range(loop[0], loop[1] + 1):
    t = lines[i].strip()
    if not t or t.startswith(';') or t.startswith('.') or t.endswith(':'):
        continue
    t = t.split(';')[0].strip()
    op = t.split()[0]
    ninstr += 1
    if op.startswith('v_mfma'):
        nmfma += 1
    if op == 's_waitcnt':
        m = re.search(r'vmcnt\((\d+)\)', t)
        if m:
            n = int(m.group(1))
            waits[n] += 1
            if n <= 3:
                site_rows.append((i + 1, n, ninstr - last_vmem[0] if last_vmem else -1, last_vmem[1] if last_vmem else '-'))
        continue
    ops = t[len(op):].split(',')
    is_vload = (op.startswith('buffer_load') or op.startswith('global_load') or op.startswith('flat_load') or
                ((op.startswith('buffer_atomic') or op.startswith('global_atomic')) and ('sc0' in t or 'glc' in t)))
    is_vmem = op.startswith(('buffer_', 'global_', 'flat_', 'scratch_'))
    if is_vmem:
        nvmem += 1
        last_vmem = (ninstr, ' '.join(t.split()))
    if op in ('v_mov_b32', 'v_mov_b64', 'v_mov_b32_e32', 'v_mov_b64_e32') and len(ops) >= 2:
        src = regs(ops[1])
        if src and all(r in loaded for r in src):
            copies += 1
    touched = [r for o in ops for r in regs(o)]
    for r in touched:
        loaded.discard(r)
    if is_vload:
        loaded.update(regs(ops[0]))

print(f'{key}: tile loop = lines {loop[0] + 1}..{loop[1] + 1} of {path.split("/")[-1]}: {ninstr} instructions, {nmfma} MFMAs, {nvmem} vector-memory operations')
print('s_waitcnt vmcnt(N) by N: ' + '  '.join(f'{n}:{c}' for n, c in sorted(waits.items())))
print(f'vmcnt(0..3) waits: {sum(c for n, c in waits.items() if n <= 3)}')
print(f'copies out of load destinations (first read of a loaded register is a v_mov): {copies}')
if sites:
    print('line   N  instructions since the youngest vector-memory operation, which is')
    for ln, n, dist, what in site_rows:
        print(f'{ln:6d} {n:2d} {dist:5d}  {what}')
