"""
Longwave cooling of a 3-D cloud field at 11 um through the drop-in: `mcarats_ng(source='thermal', target='heating rate')` writes
Flx_mhrt=2, the NET heating rate of a thermal job -- absorbed minus emitted power per unit volume, negative where a cell cools --,
and `mca_out_ng` returns it as `heating_rate` beside the fluxes.  Printed: the domain-mean profile (cooling at the cloud top, warming
at the cloud base) with its run-to-run standard deviation, and the map of the layer that holds the cloud tops.  The surface is not part
of the heating grid: its net gain is f_down - f_up at level 0.

    python examples/03_cooling_rate.py [fdir] [collision|path]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/03_cooling_rate', estimator='path'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    sim = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], target='heating rate', source='thermal',
                         heating_estimator=estimator, surface_albedo=0.02, fdir=os.path.join(fdir, estimator), Nrun=5, photons=2e7,
                         date=datetime.datetime(2017, 8, 13), quiet=True)
    out = mca.mca_out_ng(mca_obj=sim, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    hr, sd = out['heating_rate']['data'], out['heating_rate_std']['data']          # (Nx, Ny, Nz layers)
    lev = atm.lev['altitude']['data']
    z, dz = 0.5*(lev[1:]+lev[:-1]), np.diff(lev)*1000.0
    print('%s [%s]' % (out['heating_rate']['name'], out['heating_rate']['units']))
    print('  z [km]   domain mean   mean std of a cell   coldest cell   warmest cell')
    for k in range(z.size):
        print('%8.2f   %+.4e   %.2e   %+.4e   %+.4e' % (z[k], hr[:, :, k].mean(), sd[:, :, k].mean(), hr[:, :, k].min(), hr[:, :, k].max()))
    ktop = int(np.argmin(hr.mean(axis=(0, 1))))                                    # the layer that cools most: the cloud tops
    print('cloud-top layer %d (%.2f km): cooling map, every 8th column [%s]' % (ktop, z[ktop], out['heating_rate']['units']))
    for row in hr[::8, ::8, ktop].T:
        print('  ' + ' '.join('%+.2e' % v for v in row))
    col = (hr*dz[None, None, :]).sum(axis=-1).mean()
    sfc = (out['f_down']['data'][..., 0] - out['f_up']['data'][..., 0]).mean()
    toa = out['f_up']['data'][..., -1].mean()
    print('budget [W/m^2/nm]: atmosphere %+.4e, surface (f_down - f_up at level 0) %+.4e, to space %.4e, sum %+.2e'
          % (col, sfc, toa, col+sfc+toa))
    np.savez(os.path.join(fdir, 'cooling_rate.npz'), z=z, profile=hr.mean(axis=(0, 1)), cloud_top_map=hr[:, :, ktop], std=sd)
    return out


if __name__ == '__main__':
    main(*sys.argv[1:])
