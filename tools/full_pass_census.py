"""census of the lean photon loop's full passes (blocks B0, B2, B5, B6, B4, B7 of mi3d_kernel_lean.hip) from the two measurement builds
   make -C er3t_amd/csrc OUT=/tmp/cen1.so EXTRA=-DMI3D_FULL_CENSUS=1 ; ... OUT=/tmp/cen2.so EXTRA=-DMI3D_FULL_CENSUS=2      (mi3d_diag.h)
   python tools/full_pass_census.py /tmp/cen1.so /tmp/cen2.so [workload] [photons]
each build in a process of its own (MI3D_LIBRARY); the counters `le_steps`, `le_steps3d`, `flux_tally` and the six clock counters carry
the census in these builds (the column-view build leaves them at zero otherwise)."""
import json, os, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = r'''
import json, sys
sys.path.insert(0, %r)
from er3t_amd.solver import Mi3dSolver
from bench import make_scene
sol = Mi3dSolver(0); sol.load_scene(make_scene(%r)); n = int(float(%r))
sol.set_counting(True); sol.reset(); sol.run(n, seed=1234); sol.sync()
c = dict(sol.counters()); c['kernel'] = sol.kernel_name(); c['n'] = n
print('CENSUS ' + json.dumps(c))
'''


def run(lib, work, n):
    r = subprocess.run([sys.executable, '-c', code % (root, work, n)], env=dict(os.environ, MI3D_LIBRARY=os.path.abspath(lib)), capture_output=True, text=True)
    for ln in r.stdout.split('\n'):
        if ln.startswith('CENSUS '):
            return json.loads(ln[7:])
    raise SystemExit('no census from %s: %s' % (lib, r.stderr[-400:]))


if __name__ == '__main__':
    lib1, lib2 = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else 'les480'
    n = sys.argv[4] if len(sys.argv) > 4 else '5e7'
    a, b = run(lib1, work, n), run(lib2, work, n)
    N = float(a['n'])
    print('%s, %s, %g photons; builds %s | %s' % (a['kernel'], work, N, os.path.basename(lib1), os.path.basename(lib2)))
    passes, full = a['sched_b_slots']/64.0, a['le_steps3d']/64.0
    print('passes of phase B per photon %.4f, of which full %.4f (one in %.2f)' % (passes/N, full/N, passes/max(full, 1)))
    print('phase A lane utilisation %.3f, phase B %.3f' % (a['sched_a_lanes']/max(a['sched_a_slots'], 1), a['sched_b_lanes']/max(a['sched_b_slots'], 1)))
    print('lane-passes per photon parked in a rare mode while a pass that is not full runs: %.3f (of %.3f lane-slots of phase B; collisions found by the walk: %.3f)'
          % (a['le_steps']/N, a['sched_b_slots']/N, a['scatter']/N))
    print('photons a later block hands back to an earlier one (B6 -> uniform layers, roulette survivor -> flight), waiting for a second full pass: %.4f per photon '
          '(roulette survivors among them: %.4f)' % (a['flux_tally']/N, (a['roulette']-a['killed'])/N))
    print('lanes served per full pass: B0 %.2f  B2 %.2f  B4 %.2f   (per photon: %.3f, %.3f, %.3f; surface %.3f, roulette %.3f, killed %.3f, escaped %.3f)'
          % (b['le_steps']/full, b['le_steps3d']/full, b['flux_tally']/full, b['le_steps']/N, b['le_steps3d']/N, b['flux_tally']/N,
             a['surface']/N, a['roulette']/N, a['killed']/N, a['escaped']/N))
    names = ('A', 'B0+B5+B6+B7', 'C', 'B4 until its reads are issued', 'B2', 'B4 from there until the records are unpacked')
    tk = [a[k] for k in ('ticks_a', 'ticks_b0', 'ticks_b12', 'ticks_b34', 'ticks_b5', 'ticks_b6')]
    print('share of wave time: ' + '  '.join('%s %.4f' % (nm, t/sum(tk)) for nm, t in zip(names, tk)))
    print('full passes together: %.4f of the wave time; ticks per photon %.1f' % ((tk[1]+tk[3]+tk[4]+tk[5])/sum(tk), sum(tk)/N))
