"""
A 3.75 um image of the synthetic cloud field, where reflected sunlight and thermal emission are the same size (MODIS 20, VIIRS M12,
ABI 7: the channels of cloud effective-radius retrievals).  Three simulations of the same objects through the drop-in layer:
`source='solar'`, `source='thermal'` and `source='solar+thermal'` (Src_mtype=2: both sources in one job, every photon thermal or solar
in proportion to the two powers, Src_fsol the sunlight of every g).  The mixed radiance is the sum of the other two -- from one set of
photons, in one unit convention --, and its brightness temperature `bt` includes the sun, as the channel measures it.

    python examples/04_solar_plus_thermal.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/04_solar_plus_thermal'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(3750.0, atm, Ng=4)
    ab.coef['solar']['data'] = np.full(4, 10.0e-3)             # the sun at 3.75 um: about 10 W m-2 um-1
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    res = {}
    for source in ('solar', 'thermal', 'solar+thermal'):
        sim = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], target='radiance', source=source,
                             surface_albedo=0.1, surface_temperature=300.0, solar_zenith_angle=40.0, solar_azimuth_angle=30.0,
                             sensor_zenith_angle=0.0, fdir=os.path.join(fdir, source.replace('+', '_')), Nrun=3, photons=1e7,
                             date=datetime.datetime(2017, 8, 13), abs_obj=ab, keep_files=False, quiet=True)
        res[source] = mca.mca_out_ng(mca_obj=sim, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    sol, thm, mix = (res[k]['rad']['data'] for k in ('solar', 'thermal', 'solar+thermal'))
    print('3.75 um radiance [W/m^2/nm/sr], domain means: solar %.4e, thermal %.4e, their sum %.4e; solar+thermal in one job %.4e'
          % (sol.mean(), thm.mean(), sol.mean()+thm.mean(), mix.mean()))
    share = sol/np.maximum(sol+thm, 1e-30)
    print('solar share of the radiance: domain %.3f, per pixel %.3f ... %.3f' % (sol.mean()/(sol.mean()+thm.mean()), share.min(), share.max()))
    bt, bt_th = res['solar+thermal']['bt']['data'], res['thermal']['bt']['data']
    print('brightness temperature: with the sun %.2f ... %.2f K (mean %.2f K); emission alone %.2f ... %.2f K (mean %.2f K)'
          % (bt.min(), bt.max(), bt.mean(), bt_th.min(), bt_th.max(), bt_th.mean()))
    np.savez(os.path.join(fdir, 'image_3p75um.npz'), solar=sol, thermal=thm, mixed=mix, solar_share=share, bt=bt, bt_thermal=bt_th)
    return res


if __name__ == '__main__':
    main(*sys.argv[1:])
