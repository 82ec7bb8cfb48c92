"""
Where a pyrgeometer's reading comes from: `mcarats_ng(source='thermal', target='radiance', sensor_type='irradiance',
camera_method='backward', emission_weights=True)`.  A backward history's path and weight do not depend on any temperature, so the reading
of a sensor is exactly linear in the Planck radiances of the cells it sees: F = pi sum_c K_c B_c (the job files carry
Rad_mwgt = 1).  `mca_out_ng` returns K, combined over g and runs like the reading itself, as `emission_weight` (voxels),
`emission_weight_layers`, `emission_weight_surface`, and the cells' Planck radiances once, as `emission_planck*`.

A ground pyrgeometer under broken cloud: the shares of the surface (by reflection), the clear air and the cloud in its reading; the
Jacobian dF/dT_sfc of an up-looking sensor at 3000 m looking down; and that sensor's reading for a surface 5 K warmer, re-evaluated
from the weights of the first simulation and compared with a second simulation.

    python examples/07_where_the_longwave_comes_from.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402
from er3t_amd.thermal import planck, dplanck_dT, brightness_temperature   # noqa: E402

WL = 11.0       # um


def reading(out, warmer=0.0):
    """pi sum_c K_c B_c per sensor, [W m-2 nm-1].  warmer: the reading for a surface that many K warmer -- <surface_temperature> sets the
    lowest interface temperature, so the surface cells warm by that much and the lowest layer, whose temperature is the mean of its two
    interfaces, by half of it; every other cell keeps its Planck radiance"""
    tot = 0.0
    lowest_is_voxels = out['emission_planck_layers']['data'][0] == 0.0       # (layers inside the 3-D region carry nothing: their voxels do)
    for s in ('', '_layers', '_surface'):
        b = out['emission_planck'+s]['data'].astype(np.float64).copy()
        if warmer and s == '_surface':
            b = planck(WL, brightness_temperature(WL, b)+warmer)
        elif warmer and s == '_layers' and not lowest_is_voxels:
            b[0] = planck(WL, brightness_temperature(WL, b[0])+0.5*warmer)
        elif warmer and s == '' and lowest_is_voxels:
            b[:, :, 0] = planck(WL, brightness_temperature(WL, b[:, :, 0])+0.5*warmer)
        k = out['emission_weight'+s]['data'].astype(np.float64)
        tot = tot+(k*b[..., None]).reshape(-1, k.shape[-1]).sum(axis=0)
    return np.pi*tot


def main(fdir='tmp-data/07_where_the_longwave_comes_from'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(WL*1000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    t_sfc = float(atm.lev['temperature']['data'][0])
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
              date=datetime.datetime(2017, 8, 13), quiet=True, target='radiance', sensor_type='irradiance', Nrun=3, photons=2e5,
              camera_method='backward', sensor_xpos=[0.3, 0.3], sensor_ypos=[0.5, 0.5], sensor_altitude=[1.0, 3000.0],
              sensor_zenith_angle=[0.0, 180.0])
    m = mca.mcarats_ng(fdir=os.path.join(fdir, 'weights'), emission_weights=True, abs_obj=ab, keep_files=False, **kw)
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    f = out['f']['data']
    print('sensors: a pyrgeometer on the ground looking up, a radiometer at 3000 m looking down; %s [%s]: %s' % (out['f']['name'], out['f']['units'], f))
    print('pi sum_c K_c B_c from the weights:                                                              %s' % reading(out))

    # attribution: every cell's share K_c B_c of the reading; a voxel counts as cloud where the field has liquid water
    kv, bv = out['emission_weight']['data'].astype(np.float64), out['emission_planck']['data'].astype(np.float64)
    cloudy = cld.lay['extinction']['data'] > 0.0                  # (nx, ny, nz): the layout of the voxel weights
    share = lambda part: np.pi*part/reading(out)
    vox = kv*bv[..., None]
    lay = (out['emission_weight_layers']['data'].astype(np.float64)*out['emission_planck_layers']['data'].astype(np.float64)[:, None]).sum(axis=0)
    sfc = (out['emission_weight_surface']['data'].astype(np.float64)*out['emission_planck_surface']['data'].astype(np.float64)[..., None]).sum(axis=(0, 1))
    for i, who in enumerate(('ground pyrgeometer', 'radiometer at 3000 m')):
        print('%s: cloud %.1f %%, clear air inside the cloud layers %.1f %%, the 1-D layers above and below %.1f %%, surface %.1f %%'
              % (who, 100.0*share(vox[cloudy].sum(axis=0))[i], 100.0*share(vox[~cloudy].sum(axis=0))[i], 100.0*share(lay)[i], 100.0*share(sfc)[i]))

    # the Jacobian with respect to the surface temperature: dF/dT_sfc = pi K_sfc dB/dT(T_sfc)   [W m-2 nm-1 K-1]
    ksfc = out['emission_weight_surface']['data'].astype(np.float64).sum(axis=(0, 1))
    jac = np.pi*ksfc*float(dplanck_dT(WL, t_sfc))
    print('dF/dT_sfc [W m-2 nm-1 K-1]: %s' % jac)

    # re-evaluation: the same sensors over a surface 5 K warmer, from the weights above and from a second simulation
    warm = reading(out, warmer=5.0)
    m2 = mca.mcarats_ng(fdir=os.path.join(fdir, 'warm'), surface_temperature=t_sfc+5.0, abs_obj=ab, keep_files=False, **kw)
    out2 = mca.mca_out_ng(mca_obj=m2, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    print('surface 5 K warmer: re-evaluated %s, first order %s, a second simulation %s (run-to-run standard deviation %s)'
          % (warm, reading(out)+5.0*jac, out2['f']['data'], out2['f_std']['data']))
    np.savez(os.path.join(fdir, 'where_the_longwave_comes_from.npz'), f=f, f_from_weights=reading(out), jacobian_sfc=jac, f_warm_reevaluated=warm,
             f_warm_second_run=out2['f']['data'])
    return out, out2


if __name__ == '__main__':
    main(*sys.argv[1:])
