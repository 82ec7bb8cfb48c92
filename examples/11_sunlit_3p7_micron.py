"""
A 3.75 um image by backward Monte Carlo.  In the 3-5 um channels reflected sunlight and emission are the same size; the backward route for
satellite views serves such a solar+thermal job with `mcarats_ng(..., source='solar+thermal', view_method='backward', view_sunlight=True)`
(Rad_mvsun = 1): every scattering and every surface reflection of a history also scores the sunlight it turns into the line
of sight.  With `pixel_errors=True` one run gives `rad`, `bt` -- both include the sun -- and their standard errors `rad_se`, `bt_se`.

The path and the weight of a history do not depend on the sun, so the same seeds with the solar irradiance set to 0 walk the same histories
and score their emission alone: the difference of the two images is the solar share, pixel by pixel, with the noise of the paths cancelled.

    python examples/11_sunlit_3p7_micron.py [fdir]
"""

import copy
import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/11_sunlit_3p7_micron'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(3750.0, atm, Ng=4)
    ab.coef['solar']['data'] = np.full(4, 10.0e-3)              # W m-2 nm-1: 10 W m-2 um-1 at the top of the atmosphere
    dark = copy.deepcopy(ab)
    dark.coef['solar']['data'] = np.zeros(4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    n = 256*2*64*64                                             # 256 histories per pixel, shared among the g
    img = {}
    for name, a in (('sunlit', ab), ('dark', dark)):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=a)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
        np.random.seed(11)                                      # (mcarats_ng shuffles the seeds over its jobs: the same for both)
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=a.coef['weight']['data'], source='solar+thermal', surface_albedo=0.1,
                           solar_zenith_angle=40.0, solar_azimuth_angle=30.0, date=datetime.datetime(2017, 8, 13), quiet=True,
                           target='radiance', sensor_type='satellite', view_method='backward', view_sunlight=True, pixel_errors=True,
                           sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0], photons=n, Nrun=1, abs_obj=a, keep_files=False,
                           fdir=os.path.join(fdir, name))
        img[name] = mca.mca_out_ng(mca_obj=m, abs_obj=a, mode='mean', squeeze=True, quiet=True).data
    d, e = img['sunlit'], img['dark']
    share = 1.0-e['rad']['data'].astype(np.float64)/d['rad']['data'].astype(np.float64)
    print('3.75 um, sun 40 degrees from the zenith, %.2g histories:' % n)
    for iv, what in enumerate(('nadir', '40 degrees')):
        rad, se, bt, bse = (d[k]['data'][..., iv] for k in ('rad', 'rad_se', 'bt', 'bt_se'))
        print('  %-10s  rad %.4f (rad_se mean %.4f), bt %.2f K (%.2f ... %.2f; bt_se mean %.3f K), emission alone bt %.2f K; solar share %.2f '
              '(%.2f ... %.2f)' % (what, rad.mean(), se.mean(), bt.mean(), bt.min(), bt.max(), bse.mean(), e['bt']['data'][..., iv].mean(),
                                   share[..., iv].mean(), share[..., iv].min(), share[..., iv].max()))
    np.savez(os.path.join(fdir, 'sunlit_3p7_micron.npz'), rad=d['rad']['data'], rad_se=d['rad_se']['data'], bt=d['bt']['data'],
             bt_se=d['bt_se']['data'], rad_emission=e['rad']['data'], solar_share=share)
    return d, e, share


if __name__ == '__main__':
    main(*sys.argv[1:])
