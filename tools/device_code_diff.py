#!/usr/bin/env python3
"""Device code of two trees, compared symbol by symbol, on a host without a GPU.

    python tools/device_code_diff.py PARENT_TREE THIS_TREE [--keep DIR] [--only NAME.hip ...] [--jobs N]

Every maggie_amd/csrc/*.hip of both trees (once per value of a `// build-variants:` first line) is compiled with build()'s flags plus
`-S --cuda-device-only`. The assembly is cut into pieces that belong to one symbol each -- the function body with its .amdhsa_kernel block and
resource lines, and the kernel's entry in the metadata -- plus one piece, counted as the symbol '<file>', for what belongs to no function (globals, target, version). Pieces are
compared by symbol name, so the order of the symbols may differ; the compiler's per-function label numbers (.LBB12_3, .Lfunc_end12, BB12_3 in the loop
comments and the padding in front of those comments) are renumbered away for the same reason, and lines that name the per-compile `__hip_cuid_` are dropped. Exit status 0: same symbol set, same text for every symbol,
or symbols only REMOVED (each is printed; DESIGN.md section 21 lists the ones that were allowed to go). Anything added or changed: exit status 1.

--keep DIR leaves the .s files in DIR/parent and DIR/this and reuses one that is newer than every source and header of its tree."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only']
# only the FUNCTION index goes (.LBB12_3 -> .LBB_3, .LCPI12_0 -> .LCPI_0; BB12_3 without .L: the loop comments): the number behind the underscore stays
LABEL = re.compile(r'(?<!\w)((?:\.L)?BB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\.LCPI)\d+(?=_|\b)')
BEGIN = re.compile(r'; -- Begin function (\S+)')


def units(tree, only):
    """(label, source, extra flags) for every compile of a tree."""
    out = []
    for s in sorted(glob.glob(os.path.join(tree, 'maggie_amd', 'csrc', '*.hip'))):
        base = os.path.basename(s)
        if only and base not in only:
            continue
        with open(s) as f:
            first = f.readline()
        if first.startswith('// build-variants:'):
            name, vals = first.split(':', 1)[1].strip().split('=')
            for v in vals.split(','):
                out.append(('%s[%s=%s]' % (base, name.strip(), v.strip()), s, ['-D%s=%s' % (name.strip(), v.strip())]))
        else:
            out.append((base, s, []))
    return out


def compile_unit(tree, keep, unit):
    label, src, extra = unit
    dst = os.path.join(keep, re.sub(r'[^\w.=-]', '_', label) + '.s')
    deps = [src] + glob.glob(os.path.join(tree, 'maggie_amd', 'csrc', '*.h')) + glob.glob(os.path.join(tree, 'include', '*.h'))
    if not (os.path.isfile(dst) and all(os.path.getmtime(d) < os.path.getmtime(dst) for d in deps)):
        tmp = dst + '.tmp'
        r = subprocess.run([HIPCC] + FLAGS + extra + [src, '-o', tmp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            raise RuntimeError('hipcc failed on %s of %s' % (label, tree))
        os.replace(tmp, dst)
    with open(dst) as f:
        return f.read()


def pieces(asm):
    """{symbol: text} of one assembly file; '<file>' holds what belongs to no function."""
    # (the blanks in front of a comment pad it to a column: their number follows the digits of the label that was just renumbered)
    lines = [re.sub(r'[ \t]+;', ' ;', LABEL.sub(lambda m: m.group(1), l)) for l in asm.splitlines() if '__hip_cuid_' not in l]
    out = {'<file>': []}
    cur = out['<file>']
    i = 0
    while i < len(lines) and lines[i].strip() != '.amdgpu_metadata':
        nxt = lines[i + 1] if i + 1 < len(lines) else ''
        m = BEGIN.search(lines[i]) or (lines[i].startswith(('\t.section', '\t.text')) and BEGIN.search(nxt))
        if m:                                           # the .section / .text line in front of a function goes with that function
            assert m.group(1) not in out, m.group(1)
            cur = out[m.group(1)] = []
            if not BEGIN.search(lines[i]):
                cur.append(lines[i])
                i += 1
        elif cur is not out['<file>'] and lines[i].startswith('\t.section\t.AMDGPU.gpr_maximums'):
            cur = out['<file>']                         # after the last function
        cur.append(lines[i])
        i += 1
    entry = None
    for l in lines[i:]:                                 # the metadata: one entry per kernel under amdhsa.kernels, named by its .symbol line
        if l.startswith('  - ') and entry is not False:
            entry = []
            out.setdefault('<meta>', []).append(entry)
        elif l and not l.startswith(' '):
            entry = None if l.startswith('amdhsa.kernels:') else False
        (entry if isinstance(entry, list) else out['<file>']).append(l)
    for e in out.pop('<meta>', []):
        sym = [l.split()[-1] for l in e if l.startswith('    .symbol:')]
        assert len(sym) == 1 and sym[0].endswith('.kd'), e[:3]
        out[sym[0][:-3]] += ['<metadata>'] + e
    return {k: '\n'.join(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent_tree')
    ap.add_argument('this_tree')
    ap.add_argument('--keep')
    ap.add_argument('--only', nargs='*', default=[])
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    if min(a.jobs, 16) < 1:
        ap.error('--jobs')
    keep = a.keep or tempfile.mkdtemp(prefix='device_code_diff.')
    trees = {'parent': os.path.abspath(a.parent_tree), 'this': os.path.abspath(a.this_tree)}
    work = []
    for side, tree in trees.items():
        os.makedirs(os.path.join(keep, side), exist_ok=True)
        work += [(side, u) for u in units(tree, a.only)]
    work.sort(key=lambda w: -os.path.getsize(w[1][1]))             # the conv files take minutes: start them first
    with ThreadPoolExecutor(min(a.jobs, 16)) as ex:
        asm = list(ex.map(lambda w: compile_unit(trees[w[0]], os.path.join(keep, w[0]), w[1]), work))
    got = {'parent': {}, 'this': {}}
    for (side, (label, _, _)), text in zip(work, asm):
        got[side][label] = pieces(text)
    bad = 0
    print('%-34s %8s %10s %8s %6s %8s' % ('unit', 'symbols', 'identical', 'removed', 'added', 'changed'))
    for label in sorted(set(got['parent']) | set(got['this'])):
        p, t = got['parent'].get(label), got['this'].get(label)
        if p is None or t is None:
            print('%-34s only in %s' % (label, 'this' if p is None else 'parent'))
            bad += 1
            continue
        removed = sorted(set(p) - set(t))
        added = sorted(set(t) - set(p))
        changed = sorted(k for k in set(p) & set(t) if p[k] != t[k])
        print('%-34s %8d %10d %8d %6d %8d' % (label, len(p), len(set(p) & set(t)) - len(changed), len(removed), len(added), len(changed)))
        for kind, names in (('removed', removed), ('ADDED', added), ('CHANGED', changed)):
            for n in names:
                print('    %s %s' % (kind, n))
        bad += len(added) + len(changed)
    print('device code: %s' % ('DIFFERS' if bad else 'identical (removed symbols are listed above)'))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
