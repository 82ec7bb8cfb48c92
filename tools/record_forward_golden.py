"""
Record the fixtures of tests/test_gpu_forward_builds.py: what a library computes for the cases of tests/forward_builds_cases.py.

    python tools/record_forward_golden.py [--lib path/to/libmi3drt.so] [--out tests/golden/forward_builds]

One .npz per case: the name of the route, the form of the entry records and the first 14 counters of a counting run, and the name, the
form and the raw float64 tallies of a run of the production build (tests/golden/forward_builds/README.md names the arrays).  Every
production run is made a second time: the largest relative difference between the two, element by element, goes into the table at
the end of that README -- how far the same library is from itself, a record beside the test's bound and not a bound.  The fixtures are
a yardstick for a change that must leave every route with the build it had: point --lib at a build of the commit BEFORE that change
(MI3D_LIBRARY does the same), never at the code under test.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '<!-- run to run: written by tools/record_forward_golden.py -->'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'forward_builds'))
    a = ap.parse_args()
    if a.lib:
        os.environ['MI3D_LIBRARY'] = os.path.abspath(a.lib)
    import numpy as np
    import torch
    torch.cuda.init()                     # (before the library opens the HIP runtime: tests/conftest.py)
    from er3t_amd.solver import Mi3dSolver, library_path
    from tests.forward_builds_cases import CASES, COUNTERS, largest_relative_difference, run_case, run_once, tally_events
    os.makedirs(a.out, exist_ok=True)
    sol = Mi3dSolver(device=0)
    print('library: %s' % library_path())
    rows = ['| case | tally events n | n 2^-53 | largest relative difference between two runs |', '|---|---|---|---|']
    for name in CASES:
        r = run_case(sol, name)
        np.savez_compressed(os.path.join(a.out, name + '.npz'), **r)
        again = {'run0_'+k: v for k, v in run_once(sol, name, False).items()}
        n, d = tally_events(name, r['run1_counters']), largest_relative_difference(again, r)
        rows.append('| `%s` | %d | %.2e | %.2e |' % (name, n, n*2.0**-53, d))
        print('%-18s %-60s form %d/%d  %s' % (name, r['run0_kernel'], int(r['run0_form']), int(r['run1_form']), dict(zip(COUNTERS, r['run1_counters'].tolist()))))
        print('%-18s want %-55s n = %d, run to run %.2e' % ('', CASES[name]['want'] % 0, n, d))
    sol.close()
    readme = os.path.join(a.out, 'README.md')
    head = open(readme).read().split(MARK)[0] if os.path.exists(readme) else ''
    with open(readme, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
