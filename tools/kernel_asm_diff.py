"""Compare two device-assembly files (hipcc --cuda-device-only -S) kernel by kernel: instruction stream from the label to the
last s_endpgm (comments dropped, basic-block labels renumbered), the .amdhsa_kernel block and the compiler's register / scratch /
LDS / occupancy figures; differing instruction lines are printed.  Every kernel gets a class:
  (a) identical: instruction stream, .amdhsa_kernel block and figures are the same;
  (b) equivalent: block and figures are the same, so is the multiset of mnemonics of the instructions that do not begin with s_,
      and so are the counts of s_waitcnt, s_barrier and s_setprio (register names and the order or polarity of scalar compares,
      branches and s_nop may differ);
  (c) anything else - the mnemonics whose counts differ are listed.

    python tools/kernel_asm_diff.py before.s after.s [--brief]      (--brief: classes, figures and counts only, no line listing)"""
import collections
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


def classify(ia, ib, same_rest):
    """class of one kernel and, for (c), the mnemonics whose counts differ"""
    if ia == ib and same_rest:
        return 'a', ''
    ca, cb = (collections.Counter(l.split()[0] for l in ins if not l.endswith(':')) for ins in (ia, ib))
    held = lambda m: not m.startswith('s_') or m in ('s_waitcnt', 's_barrier', 's_setprio')
    if same_rest and all(ca[m] == cb[m] for m in set(ca) | set(cb) if held(m)):
        return 'b', ''
    return 'c', ', '.join('%s %d -> %d' % (m, ca[m], cb[m]) for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m])


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
print('%d kernels before, %d after; only before: %s; only after: %s' % (len(a), len(b), sorted(set(a) - set(b)), sorted(set(b) - set(a))))
differ = 0
classes = collections.Counter()
for name in sorted(set(a) & set(b)):
    (ia, da, fa), (ib, db, fb) = a[name], b[name]
    differ += ia != ib or da != db or fa != fb
    cls, moved = classify(ia, ib, da == db and fa == fb)
    classes[cls] += 1
    print('  (%s)  instr %s  desc %s  figures %s  %6d -> %6d instructions  %s' % (cls, '==' if ia == ib else '!=', '==' if da == db else '!=',
                                                                                '==' if fa == fb else '!=', len(ia), len(ib), name))
    print('      %s' % fa if fa == fb else '      before: %s\n      after:  %s' % (fa, fb))
    if moved:
        print('      counts that differ: ' + moved)
    if '--brief' in sys.argv[3:]:
        continue
    for l in difflib.unified_diff(ia, ib, 'before', 'after', n=0, lineterm=''):
        if l[0] in '+-' and l[:3] not in ('+++', '---'):
            print('      ' + l)
print('kernels that are not identical: %d; class (a) %d, (b) %d, (c) %d' % (differ, classes['a'], classes['b'], classes['c']))
