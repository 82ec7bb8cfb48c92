"""
What do horizontal photon paths do to an 11 um image?  The same cloud twice: under the 3-D solver and under independent columns (IPA), both
served backwards, each with the standard error of every pixel from its ONE run.  `view_columns=True` (Rad_mvcol = 1) lets
`view_method='backward'` serve `solver='ipa'`: a history keeps the column under its start.  The difference of the two brightness
temperatures then has an error bar of its own, sqrt(se_3d^2 + se_ipa^2), pixel by pixel.

    python examples/12_three_d_minus_ipa_brightness_temperature.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/12_three_d_minus_ipa_brightness_temperature'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    n = 256*2*64*64                                             # 256 histories per pixel, shared among the g
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
              date=datetime.datetime(2017, 8, 13), quiet=True, target='radiance', sensor_type='satellite', view_method='backward',
              pixel_errors=True, Nrun=1, sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0], photons=n, abs_obj=ab,
              keep_files=False)
    three = mca.mcarats_ng(fdir=os.path.join(fdir, '3d'), solver='3d', **kw)
    ipa = mca.mcarats_ng(fdir=os.path.join(fdir, 'ipa'), solver='ipa', view_columns=True, **kw)
    d3 = mca.mca_out_ng(mca_obj=three, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    di = mca.mca_out_ng(mca_obj=ipa, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    dbt = d3['bt']['data'].astype(np.float64)-di['bt']['data'].astype(np.float64)
    se = np.sqrt(d3['bt_se']['data'].astype(np.float64)**2+di['bt_se']['data'].astype(np.float64)**2)
    print('BT(3-D) - BT(IPA) at 11 um, %.2g histories a job, one run each; the error bar of a pixel is sqrt(se_3d^2 + se_ipa^2)' % n)
    for iv, what in enumerate(('nadir', '40 degrees')):
        d, s = dbt[..., iv], se[..., iv]
        print('  %-10s  mean %+.3f K, from %+.2f to %+.2f K; error bar %.3f K on average, largest %.3f K; %.0f %% of the pixels differ by more '
              'than 3 error bars; domain mean %+.3f +- %.3f K'
              % (what, d.mean(), d.min(), d.max(), s.mean(), s.max(), 100.0*np.mean(np.abs(d) > 3.0*s), d.mean(), np.sqrt((s**2).sum())/s.size))
    np.savez(os.path.join(fdir, 'three_d_minus_ipa.npz'), bt_3d=d3['bt']['data'], bt_ipa=di['bt']['data'], bt_se_3d=d3['bt_se']['data'],
             bt_se_ipa=di['bt_se']['data'], dbt=dbt, dbt_se=se)
    return dbt, se


if __name__ == '__main__':
    main(*sys.argv[1:])
