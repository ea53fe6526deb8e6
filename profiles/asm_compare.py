"""Per-kernel comparison of the device assembly of two builds (text only).

  hipcc <Makefile flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage x.hip -o x.s 2> x.rpass
  python3 asm_compare.py old1.s,old2.s new1.s,new2.s old1.rpass,old2.rpass new1.rpass,new2.rpass

Per kernel symbol: comments, debug / line directives and the function index inside local labels are dropped, the rest of
the instruction stream is compared line by line; the resource figures come from the remarks.  Prints a markdown table."""
import re, sys, subprocess, collections
def kernels(paths):
    out = {}
    for p in paths:
        cur = None
        for line in open(p):
            m = re.match(r'^(_Z\w+):', line)
            if m and cur is None:
                cur = m.group(1); out[cur] = []; continue
            if cur:
                if line.startswith('.Lfunc_end'):
                    cur = None; continue
                s = line.split(';')[0].rstrip()
                if not s.strip(): continue
                t = s.strip()
                if t.startswith(('.loc', '.file', '.cfi', '.p2align', '.section', '.type', '.globl', '.protected', '.weak')): continue
                s = re.sub(r'\.LBB\d+_', '.LBB_', s)
                s = re.sub(r'\.Ltmp\d+', '.Ltmp', s)
                out[cur].append(s.strip())
    return out
def res(paths):
    r = collections.defaultdict(dict)
    name = None
    for p in paths:
        for line in open(p):
            m = re.search(r'remark: .*Function Name: (\S+)', line)
            if m: name = m.group(1); continue
            m = re.search(r'remark: +(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', line)
            if m and name: r[name][m.group(1).split(' ')[0]] = int(m.group(2))
    return r
def dem(names):
    o = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, o))
old_s, new_s, old_r, new_r = [a.split(',') for a in sys.argv[1:5]]
A, B = kernels(old_s), kernels(new_s)
RA, RB = res(old_r), res(new_r)
d = dem(sorted(set(A) | set(B)))
print('| kernel | instructions | VGPRs | SGPRs | LDS | scratch | occupancy | stream |')
print('|---|---|---|---|---|---|---|---|')
bad = 0
for k in sorted(set(A) | set(B), key=lambda k: d[k]):
    n = d[k].replace('void ', '').split('(')[0]
    if k not in B: print(f'| `{n}` | {len(A[k])} | | | | | | removed |'); continue
    if k not in A: print(f'| `{n}` | {len(B[k])} | | | | | | NEW |'); bad += 1; continue
    same = A[k] == B[k]
    f = lambda key: (str(RA[k].get(key)) if RA[k].get(key) == RB[k].get(key) else f'{RA[k].get(key)} -> {RB[k].get(key)}')
    print(f'| `{n}` | {len(A[k])}' + ('' if same else f' -> {len(B[k])}') + f' | {f("VGPRs")} | {f("TotalSGPRs")} | {f("LDS")} | {f("ScratchSize")} | {f("Occupancy")} | {"identical" if same else "DIFFERS"} |')
    bad += not same
print(f'\n{len(A)} kernels before, {len(B)} after, {bad} differ or are new')
