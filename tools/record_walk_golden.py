"""
Record the fixtures of tests/test_gpu_walk_step.py: what a library computes for the cases of tests/walk_step_cases.py.

    python tools/record_walk_golden.py [--lib path/to/libmi3drt.so] [--out tests/golden/walk_step] [--flux]

One .npz per case: the event counters of a counting run as integers (`counters`, in the order of walk_step_cases.COUNTERS), the float32
image (or flux planes) of a plain run (`image`) and the routes' names.  The fixtures are a yardstick for a change that must leave every
history what it was: point --lib at a build of the commit BEFORE that change (MI3D_LIBRARY does the same), never at the code under test.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'walk_step'))
    ap.add_argument('--flux', action='store_true', help='the flux cases as well')
    a = ap.parse_args()
    if a.lib:
        os.environ['MI3D_LIBRARY'] = os.path.abspath(a.lib)
    import numpy as np
    from er3t_amd.solver import Mi3dSolver, library_path
    from tests.walk_step_cases import CASES, FLUX_CASES, COUNTERS, run_case
    os.makedirs(a.out, exist_ok=True)
    sol = Mi3dSolver(device=0)
    print('library: %s' % library_path())
    for name in list(CASES) + (list(FLUX_CASES) if a.flux else []):
        r = run_case(sol, name)
        np.savez(os.path.join(a.out, name + '.npz'), counters=r['counters'], image=r['image'],
                 kernel=np.array(r['kernel']), kernel_counting=np.array(r['kernel_counting']))
        print('%-8s %-44s %s image max %.6g' % (name, r['kernel'], dict(zip(COUNTERS, r['counters'].tolist())), float(np.abs(r['image']).max())))
    sol.close()


if __name__ == '__main__':
    main()
