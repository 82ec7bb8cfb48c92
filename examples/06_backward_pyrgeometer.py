"""
The pyrgeometer network of examples/05_pyrgeometer.py by backward Monte Carlo: `mcarats_ng(source='thermal', target='radiance',
sensor_type='irradiance', camera_method='backward')`.  Every history starts at a sensor and flies backwards along a line of sight; it
collects the emission of the air and the clouds it crosses and of the surface.  The job files carry Rad_mbwd = 1 and no
Rad_nimg: a line of sight wraps through the cyclic domain, all of which is seen.  Three rows of sensors: on the ground, INSIDE the
cloud layer (where the forward route's 1 / r^2 estimates are clamped and heavy-tailed) and above it, looking down.  Beside the ground
row, the same sensors by the forward route with two rings of periodic images, at a hundred times the histories.

    python examples/06_backward_pyrgeometer.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/06_backward_pyrgeometer'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
              date=datetime.datetime(2017, 8, 13), quiet=True, target='radiance', sensor_type='irradiance', Nrun=5)
    g = (np.arange(4)+0.5)/4.0
    rows = (('on the ground, looking up', 1.0, 0.0), ('inside the cloud layer (1000 m), looking up', 1000.0, 0.0), ('above the clouds (3000 m), looking down', 3000.0, 180.0))
    res = {}
    for i, (what, z, vza) in enumerate(rows):
        m = mca.mcarats_ng(sensor_xpos=g, sensor_ypos=0.5, sensor_altitude=z, sensor_zenith_angle=vza, camera_method='backward',
                           fdir=os.path.join(fdir, 'backward%d' % i), photons=2e5, **kw)
        out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
        res[i] = (out['f']['data'], out['f_std']['data'])
        print('%s: %s [%s], run-to-run standard deviation in brackets, 2e5 histories a run' % (what, out['f']['name'], out['f']['units']))
        print('  ' + '  '.join('%.4e (%.1e)' % (a, b) for a, b in zip(*res[i])))
    m = mca.mcarats_ng(sensor_xpos=g, sensor_ypos=0.5, sensor_altitude=1.0, sensor_zenith_angle=0.0, camera_images=2,
                       fdir=os.path.join(fdir, 'forward'), photons=2e7, **kw)
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    print('on the ground, forward route (camera_images=2), 2e7 photons a run:')
    print('  ' + '  '.join('%.4e (%.1e)' % (a, b) for a, b in zip(out['f']['data'], out['f_std']['data'])))
    np.savez(os.path.join(fdir, 'backward_pyrgeometer.npz'), f_ground=res[0][0], f_cloud=res[1][0], f_above=res[2][0], f_ground_forward=out['f']['data'])
    return res, out


if __name__ == '__main__':
    main(*sys.argv[1:])
