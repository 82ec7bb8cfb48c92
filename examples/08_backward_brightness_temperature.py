"""
An 11 um brightness-temperature image of the synthetic cloud field, a nadir and a slant view (40 degrees) in one simulation, by the forward
route and by backward Monte Carlo: `mcarats_ng(source='thermal', target='radiance', view_method='backward')`.  A backward history starts
on the sensor plane inside its pixel and flies along the view's line of sight; it collects the emission of the air and the clouds it
crosses and of the surface, and every pixel gets the same number of histories.  The job files carry Rad_mvbwd = 1.
Forward beside backward at (about) equal kernel time: a forward thermal photon is cheaper than a backward history, so a
first forward job with the backward job's number of histories measures the ratio, and the forward job shown takes that many times the
photons.  Printed: the image means, and the run-to-run standard deviation of a pixel's radiance, the noise of either image.

    python examples/08_backward_brightness_temperature.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402


def main(fdir='tmp-data/08_backward_brightness_temperature'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
              date=datetime.datetime(2017, 8, 13), quiet=True, target='radiance', sensor_type='satellite', Nrun=5,
              sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
    res = {}
    n = 64*2*64*64                                              # 64 histories per pixel and run
    run = lambda method, photons, name: mca.mcarats_ng(view_method=method, fdir=os.path.join(fdir, name), photons=photons, abs_obj=ab,
                                                       keep_files=False, **kw)
    bwd = run('backward', n, 'backward')
    cal = run('forward', n, 'forward_calibration')
    for method, photons, m in (('backward', n, bwd), ('forward', int(n*bwd.kernel_ms/cal.kernel_ms), None)):
        m = m if m is not None else run(method, photons, 'forward')
        out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
        bt, rad, std = out['bt']['data'], out['rad']['data'], out['rad_std']['data']
        res[method] = (bt, rad, std)
        print('%s route, %.2g histories a run, %.1f ms of transport kernels:' % (method, photons, m.kernel_ms))
        for iv, what in enumerate(('nadir', '40 degrees')):
            print('  %-10s  brightness temperature %.2f K (%.2f ... %.2f), run-to-run standard deviation of a pixel\'s radiance %.2f %%'
                  % (what, bt[..., iv].mean(), bt[..., iv].min(), bt[..., iv].max(), 100.0*(std[..., iv]/rad[..., iv]).mean()))
    np.savez(os.path.join(fdir, 'backward_brightness_temperature.npz'), bt_backward=res['backward'][0], bt_forward=res['forward'][0])
    return res


if __name__ == '__main__':
    main(*sys.argv[1:])
