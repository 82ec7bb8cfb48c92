"""
How noisy is a backward brightness-temperature image?  Every backward history scores in exactly one pixel and the histories of a pixel are
independent, so the standard error of every pixel follows from ONE run: `mcarats_ng(..., view_method='backward', pixel_errors=True)` also
tallies the squared scores (Rad_mserr = 1) and `mca_out_ng` returns `rad_se` and `bt_se` beside `rad` and `bt`.

  1  an 11 um image of the synthetic cloud field, nadir and 40 degrees, Nrun = 1: the brightness temperature and its standard error map;
     beside it the same job with Nrun = 3 and the run-to-run standard deviation er3t would quote, at three times the histories
  2  `Mi3dSolver.run_until`: one job of the simulation (its first g), on a coarser image of 16 x 16 pixels a view, run until no pixel's
     brightness temperature is noisier than 0.1 K

    python examples/10_noise_of_a_brightness_temperature.py [fdir]
"""

import dataclasses
import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402
from er3t_amd.scene import Scene                                # noqa: E402
from er3t_amd.solver import Mi3dSolver                          # noqa: E402
from er3t_amd.thermal import brightness_temperature, dplanck_dT   # noqa: E402


def main(fdir='tmp-data/10_noise_of_a_brightness_temperature'):
    os.makedirs(fdir, exist_ok=True)
    atm = synth.atm_synth(synth.z_levels_config2())
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    n = 256*2*64*64                                             # 256 histories per pixel and run, shared among the g
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
              date=datetime.datetime(2017, 8, 13), quiet=True, target='radiance', sensor_type='satellite', view_method='backward',
              pixel_errors=True, sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0], photons=n, abs_obj=ab, keep_files=False)
    one = mca.mcarats_ng(fdir=os.path.join(fdir, 'nrun1'), Nrun=1, **kw)
    d1 = mca.mca_out_ng(mca_obj=one, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    three = mca.mcarats_ng(fdir=os.path.join(fdir, 'nrun3'), Nrun=3, **kw)
    d3 = mca.mca_out_ng(mca_obj=three, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    slope = dplanck_dT(one.wlen_um, d3['bt']['data'].astype(np.float64))
    bt_std3 = d3['rad_std']['data'].astype(np.float64)*1.0e3/slope/np.sqrt(2.0)       # what three runs say of the error of their mean: std(ddof=1) / sqrt(3)
    print('Nrun = 1, %.2g histories: brightness temperature and its standard error from the histories themselves' % n)
    for iv, what in enumerate(('nadir', '40 degrees')):
        bt, se = d1['bt']['data'][..., iv], d1['bt_se']['data'][..., iv]
        print('  %-10s  bt %.2f K (%.2f ... %.2f), bt_se mean %.3f K, largest %.3f K' % (what, bt.mean(), bt.min(), bt.max(), se.mean(), se.max()))
    print('Nrun = 3, three times the histories: bt_se of the mean, from the histories, %.3f K on average; from the spread of the three runs '
          '%.3f K on average, a figure with two degrees of freedom that scatters from pixel to pixel between %.3f and %.3f K'
          % (d3['bt_se']['data'].mean(), bt_std3.mean(), np.percentile(bt_std3, 5), np.percentile(bt_std3, 95)))
    # ---- run until every pixel is quiet enough: the first g of the job files through the solver itself
    nml = mca.mca_inp_read(one.fnames_inp[0][0])
    scene = dataclasses.replace(Scene.from_nml(nml, os.path.dirname(one.fnames_inp[0][0]), solver=0), nxr=16, nyr=16)
    sol = Mi3dSolver(device=0)
    sol.load_scene(scene)
    npix = scene.nview*scene.nyr*scene.nxr
    sol.reset(); sol.run(1024*npix, seed=1)                       # a pilot image: the slope of the Planck function where it is smallest
    pilot = brightness_temperature(scene.src_wlen, sol.radiance(1024*npix).astype(np.float64))
    se_max = 0.1*float(dplanck_dT(scene.src_wlen, pilot).min())
    N = sol.run_until(se_max, max_histories=(1 << 21)*npix, seed=1, chunk=32768*npix)
    rad, se = sol.radiance(N).astype(np.float64), sol.radiance_se(N).astype(np.float64)
    bt_se = se/dplanck_dT(scene.src_wlen, brightness_temperature(scene.src_wlen, rad))
    print('run_until 0.1 K (g 1 of 4, 16 x 16 pixels a view): stopped after %d histories a pixel on the %s build, largest bt_se %.3f K, mean %.3f K'
          % (N//npix, sol.kernel_name(), bt_se.max(), bt_se.mean()))
    sol.close()
    np.savez(os.path.join(fdir, 'noise_of_a_brightness_temperature.npz'), bt=d1['bt']['data'], bt_se=d1['bt_se']['data'],
             bt_se_three_runs=d3['bt_se']['data'], bt_std_three_runs=bt_std3, histories_per_pixel_until=N//npix)
    return d1, d3, N


if __name__ == '__main__':
    main(*sys.argv[1:])
