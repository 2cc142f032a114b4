#!/usr/bin/env python3
"""Is the device code of two builds of a kernel file the same, kernel by kernel?

  hipcc $(HIPFLAGS) $(HIPFLAGS_equihash_solver) --cuda-device-only -S csrc/kernels/equihash_solver.hip -o X.s
  python tools/eh_codegen_cmp.py parent.s change.s > profiles/raw/rN/codegen_identity.txt

A change of the host code alone can move the kernels inside the file (they are emitted in the order
of their first use), and the compiler numbers local labels by the function's position, so the two
files then differ byte for byte although no kernel changed. This tool compares per symbol:
  text  each kernel's block of the .s file (code, kernel descriptor, resource comments) with the
        function ordinal in local labels (.LBB<n>_k, 'Header=BB<n>_k', .Lfunc_end<n>) and the comment
        column's padding normalised;
  code  the bytes of each kernel and of its descriptor (.kd) after assembling both files for the
        same target: labels are gone there, so these must be equal byte for byte.
The per-kernel metadata entries are compared as a sorted list. Exit status 0 iff everything is equal.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM', '/opt/rocm'), 'lib', 'llvm', 'bin')


def sha(b):
    return hashlib.sha256(b if isinstance(b, bytes) else b.encode()).hexdigest()


def split(path):
    """-> kernel order, {symbol: text of its block}, preamble, [file-level sections, sorted metadata entries, rest]"""
    lines = open(path).read().split('\n')
    funcs, order, pre, tail, cur = {}, [], [], [], None
    for i, ln in enumerate(lines):
        m = re.match(r'\s*\.section\s+\.text\.([A-Za-z0-9_$.]+),', ln)
        if m and m.group(1) != cur:
            cur = m.group(1)
            funcs[cur] = []
            order.append(cur)
        if re.match(r'\s*\.section\s+\.AMDGPU\.gpr_maximums', ln):
            tail = lines[i:]
            break
        (funcs[cur] if cur else pre).append(ln)
    t = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_#', '\n'.join(tail))  # named after a hash of the source
    a, b = t.index('amdhsa.kernels:'), t.index('amdhsa.target:')
    return order, {k: norm('\n'.join(v)) for k, v in funcs.items()}, pre, [t[:a], sorted(re.split(r'\n(?=  - \.agpr_count)', t[a:b])), t[b:]]


def norm(s):
    s = re.sub(r'BB\d+_', 'BB#_', s)
    s = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1#', s)
    return re.sub(r'[ \t]+;', ' ;', s)


def machine_code(path, tmp):
    """{symbol: sha256 of its bytes} of the kernels and kernel descriptors of the assembled file"""
    co = os.path.join(tmp, os.path.basename(os.path.dirname(os.path.abspath(path))) + '_' + os.path.basename(path) + '.co')
    target = re.search(r'\.amdgcn_target\s+"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)', open(path).read()).group(1)
    subprocess.check_call([os.path.join(LLVM, 'clang'), '-x', 'assembler', '-target', 'amdgcn-amd-amdhsa', '-mcpu=' + target, '-c', path, '-o', co])
    data = open(co, 'rb').read()
    secs = {}
    for ln in subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '-SW', co], capture_output=True, text=True, check=True).stdout.split('\n'):
        m = re.match(r'\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', ln)
        if m:
            secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for ln in subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '-sW', co], capture_output=True, text=True, check=True).stdout.split('\n'):
        p = ln.split()
        if len(p) == 8 and p[3] in ('FUNC', 'OBJECT') and p[6].isdigit() and not p[7].startswith('__hip_cuid_'):
            addr, off = secs[int(p[6])]
            start = off + int(p[1], 16) - addr
            out[p[7]] = '%s %6d B' % (sha(data[start:start + int(p[2])])[:16], int(p[2]))
    return out


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    print('parent  sha256 %s  %s' % (sha(open(pa, 'rb').read()), pa))
    print('change  sha256 %s  %s' % (sha(open(pb, 'rb').read()), pb))
    ao, a, apre, atail = split(pa)
    bo, b, bpre, btail = split(pb)
    with tempfile.TemporaryDirectory() as tmp:
        ma, mb = machine_code(pa, tmp), machine_code(pb, tmp)
    ok = set(a) == set(b) and set(ma) == set(mb) and apre == bpre and atail == btail
    print('kernels: %d and %d, the same set: %s, in the same order: %s' % (len(a), len(b), set(a) == set(b), ao == bo))
    if ao != bo:
        print('position of each parent kernel in the change: %s' % [bo.index(s) if s in b else None for s in ao])
    print('preamble equal: %s; file-level sections and metadata (per-kernel entries sorted) equal: %s' % (apre == bpre, atail == btail))
    print()
    print('text  code  kd    sha256[:16] of the code, size        kernel')
    for s in ao:
        t, c, k = a[s] == b.get(s), ma.get(s) == mb.get(s), ma.get(s + '.kd') == mb.get(s + '.kd')
        ok &= t and c and k
        name = subprocess.run(['c++filt', s], capture_output=True, text=True).stdout.strip() if shutil.which('c++filt') else s
        name = re.sub(r'bcpk::EhCfg<(\d+), (\d+)[^>]*>', r'Cfg\1_\2', name).split('(')[0]
        print('%-5s %-5s %-5s %s  %s' % (*('same' if x else 'DIFF' for x in (t, c, k)), ma.get(s), name))
    print()
    print('VERDICT: %s' % ('every kernel identical, symbol by symbol' if ok else 'DEVICE CODE DIFFERS'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
