#!/usr/bin/env python3
"""Compare two gfx950 assembly listings function by function.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only file.hip -o file.s     (the flags of tools/ds_read_check.py)
    tools/isa_diff.py parent.s new.s [--rename OLD=NEW ...]

A refactor that must not change device code is checked by compiling the translation unit before and after and running
this tool: it prints the function symbols only in the first listing, those only in the second, and those whose text
differs.  The text of a symbol is everything from its label to its end label -- the instructions and the kernel
descriptor (registers, LDS, scratch) -- with comments stripped, blank lines dropped, the symbol's own name replaced by a
placeholder and the per-function number taken out of local labels (.LBB12_3 -> .LBB_3), because that number is the
function's position in the file and moves when a neighbour is removed.  Whole texts are compared for equality; nothing
looks for particular instructions.

--rename OLD=NEW replaces OLD by NEW in the demangled names of the FIRST listing before the two are matched: for symbols
whose name changed for a stated reason (a dropped template parameter), e.g.
    --rename 'conv_fwd_dma_kernel<true, false, 0>=conv_fwd_dma_kernel<true, false>'

Exit status: 0 when no symbol differs, 1 otherwise (symbols on one side only do not fail it: they are the report).
"""
import argparse
import re
import shutil
import subprocess
import sys

TYPE_RE = re.compile(r'^\s*\.type\s+([^,\s]+),@function')
END_RE = re.compile(r'^\.Lfunc_end\d+:')
LOCAL_RE = re.compile(r'\.L([A-Za-z_]+?)\d+_(\d+)')


def functions(path):
    """{mangled name: [normalised lines]} of every @function symbol of the listing."""
    names, out, cur, body = set(), {}, None, None
    with open(path, errors='replace') as fh:
        lines = fh.read().split('\n')
    for ln in lines:
        m = TYPE_RE.match(ln)
        if m:
            names.add(m.group(1))
    for ln in lines:
        if cur is None:
            head = ln.split(':', 1)[0]
            if ':' in ln and head in names and head not in out:
                cur, body = head, []
            continue
        if END_RE.match(ln):
            out[cur] = body
            cur = None
            continue
        t = ln.split(';', 1)[0].replace(cur, '@SELF')
        t = LOCAL_RE.sub(r'.L\1_\2', ' '.join(t.split()))
        if t:
            body.append(t)
    return out


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or shutil.which('/opt/rocm/llvm/bin/llvm-cxxfilt')
    names = list(names)
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout.split('\n')
    return {n: d for n, d in zip(names, res)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent')
    ap.add_argument('new')
    ap.add_argument('--rename', action='append', default=[], metavar='OLD=NEW')
    args = ap.parse_args()
    fa, fb = functions(args.parent), functions(args.new)
    da, db = demangle(fa), demangle(fb)
    a = {}
    for n, body in fa.items():
        d = da[n]
        for r in args.rename:
            old, new = r.split('=', 1)
            d = d.replace(old, new)
        a[d] = body
    b = {db[n]: body for n, body in fb.items()}
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    print('%s: %d function symbols    %s: %d function symbols    common and identical: %d' %
          (args.parent, len(a), args.new, len(b), len(set(a) & set(b)) - len(differ)))
    for r in args.rename:
        print('  renamed before matching: %s' % r)
    for title, lst in (('only in %s' % args.parent, only_a), ('only in %s' % args.new, only_b), ('text differs', differ)):
        print('%s: %d' % (title, len(lst)))
        for n in lst:
            print('    ' + n)
            if lst is differ:
                x, y = a[n], b[n]
                k = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                print('        %d / %d lines; first difference at line %d: %r | %r' %
                      (len(x), len(y), k + 1, x[k] if k < len(x) else None, y[k] if k < len(y) else None))
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
