"""
Compare the gfx950 code objects of two builds of the library, first as bytes, then symbol by symbol.

    python tools/code_object_diff.py parent/libmi3drt.so er3t_amd/libmi3drt.so

A change of the host code alone should leave the device code what it was.  The whole object can still differ: kernels that are
instantiated by their first use on the host (no explicit instantiation: k_tl_runs, k_tl_scatter, k_tl_wavescan, k_tl_prefix) are emitted
in the order of those uses, and a kernel that moves takes its descriptor's code offset with it.  So: every symbol of either object
(functions, kernel descriptors, data) by name, its bytes compared; what differs is listed, what only moved is counted.
Uses llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm install (ROCM_PATH, /opt/rocm).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')


def code_object(lib, tmp, tag):
    fat, co = os.path.join(tmp, tag + '.fatbin'), os.path.join(tmp, tag + '.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', lib, fat])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                           '--input=' + fat, '--output=' + co])
    return co


def symbols(co):
    data = open(co, 'rb').read()
    secs = {}
    out = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '-S', '-W', co], text=True)
    for m in re.finditer(r'\[\s*(\d+)\]\s+(\S+)\s+(\S+)\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+([0-9a-f]+)', out):
        secs[int(m.group(1))] = (m.group(2), m.group(3), int(m.group(4), 16), int(m.group(5), 16))
    syms, on = {}, False
    for line in subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '-s', '-W', co], text=True).splitlines():
        if line.startswith('Symbol table'):
            on = '.symtab' in line
            continue
        f = line.split()
        if not on or len(f) < 8 or not f[0].endswith(':') or not f[6].isdigit() or f[2] == '0':
            continue
        name, kind, addr, off = secs[int(f[6])]
        if kind != 'NOBITS':
            at = off + int(f[1], 16) - addr
            syms[f[7]] = (name, int(f[1], 16), data[at:at + int(f[2])])
    return data, syms


def main(parent, new):
    with tempfile.TemporaryDirectory() as tmp:
        da, a = symbols(code_object(parent, tmp, 'parent'))
        db, b = symbols(code_object(new, tmp, 'new'))
    print('code objects: %d and %d bytes, sha256 %s and %s: %s' % (len(da), len(db), hashlib.sha256(da).hexdigest()[:16], hashlib.sha256(db).hexdigest()[:16],
                                                                 'identical' if da == db else 'differ'))
    print('%d and %d symbols with bytes; only in the first: %s; only in the second: %s' % (len(a), len(b), sorted(set(a) - set(b)), sorted(set(b) - set(a))))
    differ = [k for k in a if k in b and a[k][2] != b[k][2]]
    moved = [k for k in a if k in b and a[k][1] != b[k][1]]
    for k in differ:
        at = [i for i, (x, y) in enumerate(zip(a[k][2], b[k][2])) if x != y]
        # (a kernel descriptor, `.kd`: bytes 16 ... 23 are the offset from the descriptor to the kernel's code)
        print('DIFF %s (%s, %d bytes; bytes %d ... %d differ)' % (k, a[k][0], len(a[k][2]), at[0], at[-1]))
    text = sum(len(v[2]) for v in a.values() if v[0] == '.text')
    print('%d symbols differ, of them outside .text: %d; %d symbols at another address; .text bytes compared: %d' %
          (len(differ), sum(1 for k in differ if a[k][0] != '.text'), len(moved), text))
    return 1 if set(a) != set(b) or any(a[k][0] == '.text' for k in differ) else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
