"""
Cameras through the fused g-loop (run statistics on the device) against the file route (one output file per job), the way
tests/test_gpu_dropin.py holds satellite views and fluxes to it: a polar all-sky camera gives the same arrays on both routes -- its run
field holds no direct sun, as its files hold none --, and irradiance sensors give the same f, f_diffuse and f_direct.
"""

import contextlib
import copy
import io
import os

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd.synth import atm_synth, abs_synth, cld_synth
from tests.golden import inputs as gin

pytestmark = pytest.mark.gpu


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _routes(tmp_path, name, **kw):
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(650.0, atm, Ng=3)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    a1 = _quiet(mca.mca_atm_1d, atm_obj=atm, abs_obj=ab)
    a3 = _quiet(mca.mca_atm_3d, atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
    m = _quiet(mca.mcarats_ng, atm_1ds=[a1], atm_3ds=[a3], Ng=3, target='radiance', surface_albedo=0.05, solar_zenith_angle=40.0,
               fdir=str(tmp_path/name), Nrun=3, photons=2e5, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py',
               overwrite=True, date=gin.DATE, quiet=True, abs_obj=ab, keep_files=True, **kw)
    assert m.fused is not None and all(os.path.exists(f) for row in m.fnames_out for f in row)
    files = copy.copy(m); files.fused = None
    return m, files, ab


def test_allsky_camera_fused_equals_files(tmp_path):
    """er3t's all-sky camera (polar map, 178-degree cone: the sun is in it) -- the fused route adds no direct sun to the image"""
    m, files, ab = _routes(tmp_path, 'allsky', sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0)   # looking up
    from er3t_amd.rtm.mca.mca_exe import get_runner
    assert get_runner().sols[0].camera_direct().max() > 0.0          # the sun is in the camera's cone and image
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys())
        for k in ['rad'] + (['rad_std'] if mode == 'mean' else []):
            assert a[k]['data'].shape == b[k]['data'].shape and a[k]['data'].max() > 0.0, (mode, k)
            assert np.array_equal(a[k]['data'], b[k]['data']), (mode, k)     # same float32 operations in the same order
    # and the files are what mi3d_get_radiance gives: one variable, no rdir
    assert len(mca.mca_out_raw(m.fnames_out[0][0]).data) == 1


def test_irradiance_sensors_fused_equal_files(tmp_path):
    m, files, ab = _routes(tmp_path, 'irr', sensor_type='irradiance', sensor_xpos=[0.1, 0.35, 0.6, 0.85], sensor_ypos=0.5,
                           sensor_altitude=10.0, sensor_zenith_angle=[0.0, 0.0, 20.0, 180.0])
    raw = mca.mca_out_raw(m.fnames_out[0][0])
    assert [v['name'].split()[0] for v in raw.data] == ['rad', 'rdir']
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys())
        for k in ('f', 'f_diffuse', 'f_direct'):
            x, y = a[k]['data'], b[k]['data']
            assert x.shape == y.shape and x.shape[0] == 4, (mode, k)
            # the fused field holds diffuse + direct; its reader takes the known direct part off again (float32 rounding apart)
            assert np.allclose(x, y, rtol=2e-5, atol=2e-6*np.abs(b['f']['data']).max()), (mode, k, x, y)
        assert np.array_equal(a['f_direct']['data'], b['f_direct']['data'])
        fd = b['f_direct']['data'] if mode == 'mean' else b['f_direct']['data'][:, 0]
        assert fd[3] == 0.0 and fd[:3].max() > 0.0            # a down-looking sensor does not see the sun
