"""what two waits of a pass of the lean photon loop cost (round 13; mi3d_diag.h: -DMI3D_WAIT_CENSUS)
   make -C er3t_amd/csrc OUT=/tmp/wc_old.so EXTRA="-DMI3D_WAIT_CENSUS -DMI3D_LEAN_C_EARLY=0" ; ... OUT=/tmp/wc_new.so EXTRA=-DMI3D_WAIT_CENSUS
   python tools/wait_census.py [workload] [photons] /tmp/wc_old.so /tmp/wc_new.so ...
each build in a process of its own (MI3D_LIBRARY).  The counting build of the loop is measured (four waves per SIMD, not the plain build's six):
the shares are those of ITS wave time.  A tick reads the clock through the scalar memory path and waits for it, so every interval holds one
tick's cost: the calibration slot (two ticks back to back, once a pass) says how much, and the net figures have it taken off."""
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
work = sys.argv[1] if len(sys.argv) > 1 else 'les480'
n = sys.argv[2] if len(sys.argv) > 2 else '5e7'
for lib in sys.argv[3:]:
    r = subprocess.run([sys.executable, '-c', code % (root, work, n)], env=dict(os.environ, MI3D_LIBRARY=os.path.abspath(lib)), capture_output=True, text=True)
    c = [json.loads(ln[7:]) for ln in r.stdout.split('\n') if ln.startswith('CENSUS ')]
    if r.returncode or not c:
        raise SystemExit('no census from %s (exit %d): %s' % (lib, r.returncode, r.stderr[-400:]))
    c = c[0]
    tk = [c[k] for k in ('ticks_a', 'ticks_b0', 'ticks_b12', 'ticks_b34', 'ticks_b5', 'ticks_b6')]
    tot, passes = float(sum(tk)), c['sched_b_slots']/64.0
    names = ('A', 'pass begin', "C's first wait", 'two ticks', 'BSCHED + C', 'full pass + end')
    print('%s: %s, %s, %s photons; %.3f passes per photon, %.0f wave cycles per pass' % (os.path.basename(lib), c['kernel'], work, n, passes/c['n'], tot/passes))
    print('  share of wave time:  ' + '  '.join('%s %.4f' % (nm, t/tot) for nm, t in zip(names, tk)))
    print('  cycles per pass:     ' + '  '.join('%s %.1f' % (nm, t/passes) for nm, t in zip(names, tk)))
    tick = tk[3]/passes
    net = [max(tk[1]/passes - tick, 0.0), max(tk[2]/passes - tick, 0.0)]
    clean = tot/passes - 6*tick    # (the wave time without the ticks' own cost: six intervals a pass)
    print('  less a tick (%.1f cycles): pass begin %.1f cycles a pass = %.4f of the wave time, C\'s first wait %.1f = %.4f, together %.4f'
          % (tick, net[0], net[0]/clean, net[1], net[1]/clean, (net[0]+net[1])/clean), flush=True)
