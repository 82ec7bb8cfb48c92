"""
Record the fixtures of tests/test_gpu_backward_bits.py: what a library computes for the cases of tests/backward_bits_cases.py.

    python tools/record_backward_golden.py [--lib path/to/libmi3drt.so] [--out tests/golden/backward_bits]

One .npz per case: the debug entries' outputs for 1024 ids as raw bytes, the counters of those ids, and the raw float64 tallies, counters
and names of every production build over 20000 histories (tests/golden/backward_bits/README.md names the arrays).  The fixtures are a
yardstick for a change that must leave every history what it was: point --lib at a build of the commit BEFORE that change (MI3D_LIBRARY
does the same), never at the code under test.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'backward_bits'))
    a = ap.parse_args()
    if a.lib:
        os.environ['MI3D_LIBRARY'] = os.path.abspath(a.lib)
    import numpy as np
    import torch
    torch.cuda.init()                     # (before the library opens the HIP runtime: tests/conftest.py)
    from er3t_amd.solver import Mi3dSolver, library_path
    from tests.backward_bits_cases import CASES, COUNTERS, run_case
    os.makedirs(a.out, exist_ok=True)
    sol = Mi3dSolver(device=0)
    print('library: %s' % library_path())
    for name in CASES:
        r = run_case(sol, name)
        np.savez(os.path.join(a.out, name + '.npz'), **r)
        for k in sorted(r):
            if k.endswith('counters'):
                print('%-10s %-24s %s' % (name, k, dict(zip(COUNTERS, r[k].tolist()))))
            elif k.endswith('kernel') or k.endswith('capped') or k.endswith('staged'):
                print('%-10s %-24s %s' % (name, k, r[k]))
    sol.close()


if __name__ == '__main__':
    main()
