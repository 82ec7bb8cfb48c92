"""
Heating-rate jobs, both estimators of the tally (mi3d_set_heating_estimator):

  tools/heating_rate.py rate [--workload les128_flux] [--photons 5e8] [--rounds 3] [--lib other.so ...]
      photons per second of a heating-rate job on the bench grid (the flux workload with Flx_mhrt = 1 and the gas absorption of the parity
      tests), estimator 0 and 1 on this tree's library and estimator 0 on every --lib (an older build: A/B), each run in a process of its
      own, the configurations alternating round by round; the median per configuration and the spread of the rounds.  With the
      instrumented build in between: tally records per photon.
  tools/heating_rate.py fom [--batches 32] [--photons 1e5]
      the figure of merit 1 / (se^2 time) per layer of the 16 x 16 x 68 parity scene, estimator 1 over estimator 0
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def heat_job(workload):
    from bench import make_scene
    from er3t_amd.scene import TARGET_FLUX, TARGET_HEAT
    sc = make_scene(workload)
    sc.target = TARGET_FLUX | TARGET_HEAT
    sc.abs1d = sc.abs1d*30.0 + 2.0e-5
    return sc


def child_rate(workload, nph, est):
    """one configuration in this process: kernel-time and wall-clock photons per second of one run after a warm-up"""
    from er3t_amd.solver import Mi3dSolver
    sol = Mi3dSolver(0)
    sc = heat_job(workload)
    if est:
        sc.heat_estimator = 1      # (a library without the estimator: est 0 only, the call is never made)
        sol.load_scene(sc)
    else:
        sc.heat_estimator = 0
        try:
            sol.load_scene(sc)
        except OSError:            # an older build: no mi3d_set_heating_estimator -- load without it
            sol.set_heating_estimator = lambda e=0: None
            sol.load_scene(sc)
    sol.set_counting(False)
    sol.reset(); sol.run(nph//5, seed=1); sol.sync()
    sol.reset(); sol.sync()
    ms0, _ = sol.timing(); t0 = time.perf_counter()
    sol.run(nph, seed=1234); sol.sync()
    t1 = time.perf_counter(); ms, _ = sol.timing()
    out = {'kernel': nph/((ms-ms0)*1e-3), 'wall': nph/(t1-t0), 'route': sol.kernel_name()}
    if os.environ.get('HEAT_COUNT'):
        n = min(nph, 4000000)
        sol.set_counting(True); sol.reset(); sol.run(n, seed=5); sol.sync()
        c = sol.counters()
        out.update(flux_records_pp=c['flux_tally']/n, heat_records_pp=c['le_steps3d']/n if est else None, scatter_pp=c['scatter']/n)
    print(json.dumps(out))


def rate(args):
    import numpy as np
    configs = [('this est 0', None, 0), ('this est 1', None, 1)] + [(os.path.basename(l)+' est 0', os.path.abspath(l), 0) for l in args.lib]
    res = {c[0]: [] for c in configs}
    for r in range(args.rounds):
        for name, lib, est in configs:
            env = dict(os.environ)
            if lib:
                env['MI3D_LIBRARY'] = lib
            if r == 0 and not lib:
                env['HEAT_COUNT'] = '1'
            p = subprocess.run([sys.executable, os.path.abspath(__file__), 'child', '--workload', args.workload, '--photons', str(args.photons), '--est', str(est)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(name, 'FAILED', p.stderr[-400:]); return 1
            d = json.loads(p.stdout.strip().splitlines()[-1])
            res[name].append(d)
            print('round %d %-24s kernel %.4g wall %.4g photons/s  %s %s' % (r, name, d['kernel'], d['wall'], d['route'],
                  {k: round(v, 2) for k, v in d.items() if k.endswith('_pp') and v is not None}), flush=True)
    for name, rows in res.items():
        k = np.array([d['kernel'] for d in rows]); w = np.array([d['wall'] for d in rows])
        print('%-24s median kernel %.4g (spread %.1f %%), wall %.4g (spread %.1f %%)' % (name, np.median(k), 100*(k.max()-k.min())/np.median(k),
                                                                                      np.median(w), 100*(w.max()-w.min())/np.median(w)))
    return 0


def fom(args):
    import numpy as np
    from er3t_amd.solver import Mi3dSolver
    from er3t_amd.synth import les_scene
    from er3t_amd.scene import TARGET_FLUX, TARGET_HEAT
    sc = les_scene(nx=16, ny=16, nz3=50, target='flux', aerosol=True)
    sc.target = TARGET_FLUX | TARGET_HEAT
    sc.abs1d = sc.abs1d*30.0
    sol = Mi3dSolver(0)
    nb, nper = args.batches, int(args.photons)
    se, tm = [], []
    for est in (0, 1):
        sc.heat_estimator = est
        sol.load_scene(sc); sol.set_counting(False)
        sol.reset(); sol.run(nper, seed=1); sol.sync()
        h = []
        t = 0.0
        for b in range(nb):
            sol.reset(); sol.sync(); t0 = time.perf_counter()
            sol.run(nper, seed=3, offset=b*nper); sol.sync(); t += time.perf_counter()-t0
            h.append(sol.heating(nper).astype(np.float64).mean(axis=(1, 2)))
        se.append(np.std(h, axis=0, ddof=1)/np.sqrt(nb)); tm.append(t)
    f = (se[0]**2*tm[0])/(se[1]**2*tm[1])
    print('time of %d batches of %d photons: estimator 0 %.3f s, estimator 1 %.3f s' % (nb, nper, tm[0], tm[1]))
    print('figure of merit, estimator 1 over 0, per layer:', ' '.join('%d:%.0f' % (k, v) for k, v in enumerate(f)))
    print('min %.1f (layer %d), median %.0f' % (f.min(), int(f.argmin()), np.median(f)))
    return 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['rate', 'fom', 'child'])
    ap.add_argument('--workload', default='les128_flux')
    ap.add_argument('--photons', type=float, default=None, help='per run (rate: 5e8) or per batch (fom: 1e5)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=32)
    ap.add_argument('--est', type=int, default=0)
    ap.add_argument('--lib', action='append', default=[])
    a = ap.parse_args()
    if a.photons is None:
        a.photons = 1.0e5 if a.what == 'fom' else 5.0e8
    if a.what == 'child':
        child_rate(a.workload, int(a.photons), a.est)
    else:
        sys.exit(rate(a) if a.what == 'rate' else fom(a))
