"""
The heating-rate profile of a 3-D cloud field with both estimators of the tally: the default (a collision leaves w kappa_a / beta_t in its
cell) and the path-length estimator (`heating_estimator='path'`, Flx_mhest=1: every flight segment leaves w kappa_a l in the cell it
crosses), their domain-mean profiles and their run-to-run standard deviations side by side.  Same photons, same variable, same units;
the clear layers above and below the cloud are where the second one pays.

    python examples/02_heating_rate.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/02_heating_rate'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(650.0, atm, Ng=4)
    ab.coef['abso_coef']['data'] = ab.coef['abso_coef']['data']*40.0          # an absorption band: heating that shows
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    z = 0.5*(atm.lev['altitude']['data'][1:] + atm.lev['altitude']['data'][:-1])
    res = {}
    for est in ('collision', 'path'):
        sim = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], target='heating rate',
                             heating_estimator=est, surface_albedo=0.1, solar_zenith_angle=40.0, fdir=os.path.join(fdir, est), Nrun=5,
                             photons=4e6, date=datetime.datetime(2017, 8, 13), quiet=True)
        out = mca.mca_out_ng(mca_obj=sim, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
        prof = out['heating_rate']['data'].mean(axis=(0, 1))                  # (nz, Nrun): domain-mean profile of every run
        res[est] = (prof.mean(axis=-1), prof.std(axis=-1, ddof=1), out['heating_rate']['name'])
    print('%s [%s]' % (res['path'][2], out['heating_rate']['units']))
    print('  z [km]   collision: mean    std      path: mean    std      std ratio')
    for k in range(z.size):
        (m0, s0, _), (m1, s1, _) = res['collision'], res['path']
        print('%8.2f   %.4e %.2e   %.4e %.2e   %6.3f' % (z[k], m0[k], s0[k], m1[k], s1[k], s1[k]/s0[k] if s0[k] > 0 else np.nan))
    np.savez(os.path.join(fdir, 'heating_profiles.npz'), z=z, collision=res['collision'][0], collision_std=res['collision'][1],
             path=res['path'][0], path_std=res['path'][1])
    return res


if __name__ == '__main__':
    main(*sys.argv[1:])
