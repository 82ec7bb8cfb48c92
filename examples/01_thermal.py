"""
An 11 um brightness-temperature image of the synthetic cloud field through the drop-in layer: `mcarats_ng(..., source='thermal')`
writes thermal jobs (Src_mtype=3, Src_wlen, the nz+1 interface temperatures), the GPU's general photon loop emits from every cell
in proportion to its power, and `mca_out_ng` sums the g-points and inverts Planck's law (`data['bt']`).

    python examples/01_thermal.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/01_thermal'):
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=16)                  # a water-vapour-like window absorber, 16 g
    cld = synth.cld_synth(atm, nx=128, ny=128, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    sim = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=16, weights=ab.coef['weight']['data'], target='radiance', source='thermal',
                         surface_albedo=0.02, surface_temperature=300.0, sensor_zenith_angle=0.0, fdir=fdir, Nrun=3, photons=2e7,
                         date=datetime.datetime(2017, 8, 13), abs_obj=ab, keep_files=False, quiet=True)
    out = mca.mca_out_ng(mca_obj=sim, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    bt = out['bt']['data']
    print('11 um radiance: mean %.5f W/m^2/nm/sr; brightness temperature %.2f ... %.2f K (mean %.2f K), %d x %d pixels'
          % (out['rad']['data'].mean(), bt.min(), bt.max(), bt.mean(), bt.shape[0], bt.shape[1]))
    np.save(os.path.join(fdir, 'bt_11um.npy'), bt)
    return out


if __name__ == '__main__':
    main(*sys.argv[1:])
