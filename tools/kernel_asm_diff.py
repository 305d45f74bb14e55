"""Compare two device-assembly files (hipcc --cuda-device-only -S) kernel by kernel: instruction stream from the label to the
last s_endpgm (comments dropped, basic-block labels renumbered), the .amdhsa_kernel block and the compiler's register / scratch /
LDS / occupancy figures; differing instruction lines are printed.

    python tools/kernel_asm_diff.py before.s after.s"""
import difflib
import re
import sys

FIGURES = ('NumVgprs', 'NumAgprs', 'TotalNumSgprs', 'ScratchSize', 'LDSByteSize', 'Occupancy')


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r'^\t\.amdhsa_kernel (\S+)$', text, re.M):
        body = text[text.index('\n%s:' % name):]
        code, rest = body[:body.index('\t.amdhsa_kernel ')], body[body.index('\t.amdhsa_kernel '):]
        ins = [re.sub(r'\.LBB\d+_', '.LBB_', l.split(';')[0].strip()) for l in code[:code.rindex('s_endpgm')].split('\n')[2:]]
        fig = ', '.join('%s %s' % (k, re.search(r'^; %s: (\d+)' % k, rest, re.M).group(1)) for k in FIGURES)
        out[name] = ([l for l in ins if l and not l.startswith('.p2align')], rest[:rest.index('.end_amdhsa_kernel')], fig)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
print('%d kernels before, %d after; only before: %s; only after: %s' % (len(a), len(b), sorted(set(a) - set(b)), sorted(set(b) - set(a))))
differ = 0
for name in sorted(set(a) & set(b)):
    (ia, da, fa), (ib, db, fb) = a[name], b[name]
    differ += ia != ib or da != db or fa != fb
    print('  instr %s  desc %s  figures %s  %6d -> %6d instructions  %s' % ('==' if ia == ib else '!=', '==' if da == db else '!=',
                                                                          '==' if fa == fb else '!=', len(ia), len(ib), name))
    print('      %s' % fa if fa == fb else '      before: %s\n      after:  %s' % (fa, fb))
    for l in difflib.unified_diff(ia, ib, 'before', 'after', n=0, lineterm=''):
        if l[0] in '+-' and l[:3] not in ('+++', '---'):
            print('      ' + l)
print('kernels that are not identical: %d' % differ)
