"""
A pyrgeometer network under broken cloud at 11 um through the drop-in: `mcarats_ng(source='thermal', target='radiance',
sensor_type='irradiance')` puts a 4 x 4 grid of up-looking irradiance sensors on the ground under the synthetic cloud field and
`mca_out_ng` returns their readings `f` (W m-2 nm-1; `f_direct` is 0: a thermal job has no sun).  Beside them the column-mean `f_down` at
level 0 of a flux job of the same scene: what a flux job gives is the mean over the domain, not the reading of a sensor at a place --
under a cloud the sky is warm, under a gap it is cold.  Then one thermal all-sky image from the middle of the domain with its
brightness temperature `bt`.  Both sensor jobs carry Rad_nimg (here 2): the periodic images of a sensor in the cyclic domain within two
domain lengths of the nearest one are served, without which the limb-brightened horizon of a window channel is cut off.

    python examples/05_pyrgeometer.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/05_pyrgeometer'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
              date=datetime.datetime(2017, 8, 13), quiet=True)
    g = (np.arange(4)+0.5)/4.0
    xp, yp = [v.ravel() for v in np.meshgrid(g, g)]
    sens = mca.mcarats_ng(target='radiance', sensor_type='irradiance', sensor_xpos=xp, sensor_ypos=yp, sensor_altitude=1.0,
                          sensor_zenith_angle=0.0, camera_images=2, fdir=os.path.join(fdir, 'sensors'), Nrun=5, photons=2e7, **kw)
    out = mca.mca_out_ng(mca_obj=sens, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    f, sd = out['f']['data'].reshape(4, 4), out['f_std']['data'].reshape(4, 4)
    flux = mca.mcarats_ng(target='flux', fdir=os.path.join(fdir, 'flux'), Nrun=5, photons=2e7, **kw)
    fo = mca.mca_out_ng(mca_obj=flux, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    fdn = fo['f_down']['data'][..., 0]                              # (Nx, Ny) at level 0
    print('%s [%s] of the 4 x 4 sensors (rows: y), run-to-run standard deviation in brackets' % (out['f']['name'], out['f']['units']))
    for j in range(4):
        print('  ' + '  '.join('%.4e (%.1e)' % (f[j, i], sd[j, i]) for i in range(4)))
    print('sensors: mean %.4e, min %.4e, max %.4e;  flux job, f_down at level 0: domain mean %.4e, columns %.4e ... %.4e'
          % (f.mean(), f.min(), f.max(), fdn.mean(), fdn.min(), fdn.max()))
    sky = mca.mcarats_ng(target='radiance', sensor_type='all-sky', sensor_altitude=1.0, sensor_zenith_angle=180.0,
                         fdir=os.path.join(fdir, 'allsky'), Nrun=3, photons=5e7, **kw)
    so = mca.mca_out_ng(mca_obj=sky, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    bt = so['bt']['data']
    blocks = np.asarray(so['rad']['data'], dtype=np.float64)[50:450, 50:450].reshape(8, 50, 8, 50).mean(axis=(1, 3))
    from er3t_amd.thermal import brightness_temperature
    print('all-sky image %s: brightness temperature of 50 x 50 pixel blocks [K]' % (bt.shape,))
    for row in brightness_temperature(sky.wlen_um, blocks*1.0e3).T:
        print('  ' + ' '.join('%6.1f' % v for v in row))
    np.savez(os.path.join(fdir, 'pyrgeometer.npz'), f=f, f_std=sd, f_down_level0=fdn, bt=bt)
    return out, fo, so


if __name__ == '__main__':
    main(*sys.argv[1:])
