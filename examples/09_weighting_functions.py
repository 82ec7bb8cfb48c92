"""
The vertical weighting functions of an 11 um satellite image over the broken-cloud scene of example 08, a nadir and a slant view (40 degrees)
in one simulation: `mcarats_ng(source='thermal', target='radiance', view_method='backward', view_profiles=True)`.  Beside its radiance every
pixel gets two profiles over the layers from the surface up and the surface itself (the job files carry Rad_mvprf = 1):

    view_weight[..., k]        K: the share of the pixel's radiance that comes from layer k per unit Planck radiance there
    view_contribution[..., k]  C: that share itself; rad = view_contribution.sum(-1), whatever the temperatures
    view_layer_planck[..., k]  C / K: the layer's effective Planck radiance as the pixel sees it (NaN where K = 0)

Printed for a cloudy, a clear and a cloud-edge pixel of either view: where the radiance comes from (the peak of the weighting function, the
surface's share), and the layer Jacobian  dR / dT_k = K_k dB/dT(T_eff,k)  with T_eff,k the brightness temperature of C_k / K_k.  That Jacobian
is exact only where the temperature of layer k is horizontally uniform: K_k sums the weights of the layer's voxels, and one dB/dT stands for
all of them.  (The per-voxel Jacobian of a camera or a point radiometer is example 07's, `emission_weights=True`.)

    python examples/09_weighting_functions.py [fdir]
"""

import datetime
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import er3t_amd.rtm.mca as mca                                  # noqa: E402   (same names as er3t.rtm.mca)
from er3t_amd import synth                                      # noqa: E402
from er3t_amd.thermal import brightness_temperature, dplanck_dT  # noqa: E402


def main(fdir='tmp-data/09_weighting_functions'):
    os.makedirs(fdir, exist_ok=True)
    levels = synth.z_levels_config2()
    atm = synth.atm_synth(levels)
    ab = synth.abs_synth(11000.0, atm, Ng=4)
    cld = synth.cld_synth(atm, nx=64, ny=64, nz=50, cot_mean=10.0)
    a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(fdir, 'atm3d.bin'), quiet=True)
    m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=4, weights=ab.coef['weight']['data'], source='thermal', surface_albedo=0.02,
                       date=datetime.datetime(2017, 8, 13), quiet=True, target='radiance', sensor_type='satellite', Nrun=5,
                       sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0], view_method='backward', view_profiles=True,
                       fdir=os.path.join(fdir, 'backward'), photons=256*2*64*64, abs_obj=ab, keep_files=False)
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    rad, bt = out['rad']['data'], out['bt']['data']                                   # (Nxr, Nyr, Nview)
    K, C, B = out['view_weight']['data'], out['view_contribution']['data'], out['view_layer_planck']['data']      # (Nxr, Nyr, Nview, Nz+1)
    nz = K.shape[-1]-1
    z = np.asarray(levels, dtype=np.float64)
    zmid = 0.5*(z[:-1]+z[1:]) if z.size == nz+1 else np.arange(nz, dtype=np.float64)
    print('%.1f ms of transport kernels; largest |sum_k C / rad - 1| over the image: %.1e' % (m.kernel_ms, np.abs(C.sum(axis=-1)/rad-1.0).max()))
    # per nm -> per um; T_eff of every row, and the Jacobian of the radiance (W m-2 sr-1 um-1) to the temperature of a layer
    with np.errstate(invalid='ignore', divide='ignore'):
        teff = brightness_temperature(m.wlen_um, B.astype(np.float64))
        jac = K.astype(np.float64)*1.0e3*np.where(np.isfinite(teff), dplanck_dT(m.wlen_um, np.where(np.isfinite(teff), teff, 250.0)), 0.0)
    for iv, what in enumerate(('nadir', '40 degrees')):
        sfc = K[:, :, iv, nz]/np.maximum(K[:, :, iv].sum(axis=-1), 1.0e-30)          # the surface's share of the pixel's weights
        order = np.argsort(sfc, axis=None)
        picks = (('cloudy', order[0]), ('cloud edge', order[np.searchsorted(sfc.ravel()[order], 0.5*sfc.max())]), ('clear', order[-1]))
        print('%s view:' % what)
        for name, flat in picks:
            i, j = np.unravel_index(flat, sfc.shape)
            k, c = K[i, j, iv], C[i, j, iv]
            top = int(np.argmax(k[:nz]))
            print('  %-10s pixel (%2d, %2d): BT %.2f K; the surface gives %4.1f %% of the radiance, the layers %4.1f %%, most of it layer %d '
                  '(%.2f km, %.1f %%, T_eff %.1f K); dR/dT of that layer %.3f, of the surface %.3f W m-2 sr-1 um-1 K-1'
                  % (name, i, j, bt[i, j, iv], 100.0*c[nz]/c.sum(), 100.0*c[:nz].sum()/c.sum(), top, zmid[top], 100.0*c[top]/c.sum(),
                     teff[i, j, iv, top], jac[i, j, iv, top], jac[i, j, iv, nz]))
    np.savez(os.path.join(fdir, 'weighting_functions.npz'), rad=rad, bt=bt, view_weight=K, view_contribution=C, view_layer_planck=B, jacobian=jac)
    return out


if __name__ == '__main__':
    main(*sys.argv[1:])
