"""
Per-pixel standard errors of the backward routes (mi3d_set_pixel_errors 1, Rad_mserr = 1): what the host layers do without a
GPU -- the namelist key and its round trip, the refusals of mcarats_ng, Scene and mca_exe, the .err.bin file with the g / run combination of
its reader against a numpy restatement, and the header against the binding.
"""

import contextlib
import inspect
import io
import os
import re

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca import mca_exe
from er3t_amd.rtm.mca.mca_exe import _check_supported
from er3t_amd.rtm.mca.mca_out import g_factors, pixel_error_runs, read_pixel_errors
from er3t_amd.scene import Scene
from er3t_amd.synth import atm_synth, abs_synth
from er3t_amd.thermal import dplanck_dT
from tests.golden import inputs as gin

U24 = 2.0**-24


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 2, 'Rad_mvbwd': 1, 'Rad_mserr': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3,
           'Src_wlen': 11.0, 'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1, 'Atm_ext1d': np.zeros(nz), 'Atm_omg1d': np.ones(nz),
           'Atm_apf1d': np.full(nz, -1.0), 'Atm_abs1d': np.full(nz, 1.0e-5), 'Atm_nx': 1, 'Atm_ny': 1, 'Atm_dx': 1000.0, 'Atm_dy': 1000.0,
           'Rad_the': 180.0, 'Rad_phi': 0.0, 'Rad_zloc': 1.0e6}
    nml.update(kw)
    return {k: v for k, v in nml.items() if v is not None}


def _objects(wvl):
    atm = atm_synth(np.arange(17)*1.0)
    ab = abs_synth(wvl, atm, Ng=2)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    return atm, ab, a1


def _write(a1, ab, fdir, target='radiance', Nrun=1, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=2, target=target, surface_albedo=0.03, fdir=fdir, Nrun=Nrun, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


_text = lambda m: [l for l in open(m.fnames_inp[0][0]).read().splitlines() if 'Wld_jseed' not in l]
IRRADIANCE = dict(sensor_type='irradiance', sensor_xpos=[0.2, 0.7], sensor_ypos=0.5, sensor_altitude=10.0, sensor_zenith_angle=[0.0, 180.0])


def test_the_key_is_written_only_when_on_and_every_other_file_is_unchanged(tmp_path):
    _, ab, a1 = _objects(11000.0)
    _, abs_sol, a1s = _objects(650.0)
    jobs = [(a1, ab, dict(source='thermal')), (a1, ab, dict(source='thermal', view_method='backward')),
            (a1, ab, dict(source='thermal', view_method='backward', view_profiles=True)),
            (a1, ab, dict(source='thermal', target='flux')), (a1, ab, dict(source='thermal', camera_method='backward', **IRRADIANCE)),
            (a1, ab, dict(source='thermal', camera_method='backward', emission_weights=True, **IRRADIANCE)),
            (a1s, abs_sol, dict()), (a1s, abs_sol, dict(target='flux'))]
    for i, (a, b, kw) in enumerate(jobs):
        x = _text(_write(a, b, str(tmp_path/('a%d' % i)), **kw))
        y = _text(_write(a, b, str(tmp_path/('b%d' % i)), pixel_errors=False, **kw))
        assert x == y and not any('Rad_mserr' in l for l in x), kw
    for i, kw in enumerate((dict(view_method='backward'), dict(view_method='backward', sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0]),
                            dict(camera_method='backward', **IRRADIANCE))):
        off = _write(a1, ab, str(tmp_path/('f%d' % i)), source='thermal', **kw)
        on = _write(a1, ab, str(tmp_path/('v%d' % i)), source='thermal', pixel_errors=True, **kw)
        tf, tb = _text(off), _text(on)
        # one line more, in the radiance group, behind every other key of the group (the catalogue's order)
        assert sum('Rad_mserr' in l for l in tb) == 1 and [l for l in tb if 'Rad_mserr' not in l] == tf
        rad = tb[tb.index('&mcarRad_nml_job'):]
        group = rad[1:rad.index('/')]
        keys = [l.split('=')[0].strip() for l in group if '=' in l]
        assert keys[-1] == 'Rad_mserr', keys
        assert on.pixel_errors is True and off.pixel_errors is False
    from er3t_amd.rtm.mca.mca_inp import mca_inp_groups
    assert mca_inp_groups()['mcarRad_nml_job'][-1] == 'Rad_mserr'


def test_round_trip_into_a_scene(tmp_path):
    _, ab, a1 = _objects(11000.0)
    on = _write(a1, ab, str(tmp_path/'v'), source='thermal', view_method='backward', pixel_errors=True, sensor_zenith_angle=[0.0, 40.0])
    off = _write(a1, ab, str(tmp_path/'f'), source='thermal', view_method='backward', sensor_zenith_angle=[0.0, 40.0])
    nml = mca.mca_inp_read(on.fnames_inp[0][0])
    assert nml['Rad_mserr'] == 1 and nml['Rad_mvbwd'] == 1
    _check_supported(nml, str(tmp_path/'v'), solver=0)
    sc = Scene.from_nml(nml, str(tmp_path/'v'), solver=0)
    assert sc.pixel_errors == 1 and sc.view_method == 1 and sc.nview == 2
    nmf = mca.mca_inp_read(off.fnames_inp[0][0])
    assert 'Rad_mserr' not in nmf and Scene.from_nml(nmf, str(tmp_path/'f'), solver=0).pixel_errors == 0
    cam = _write(a1, ab, str(tmp_path/'c'), source='thermal', camera_method='backward', pixel_errors=True, **IRRADIANCE)
    nmc = mca.mca_inp_read(cam.fnames_inp[0][0])
    _check_supported(nmc, str(tmp_path/'c'), solver=0)
    sc = Scene.from_nml(nmc, str(tmp_path/'c'), solver=0)
    assert sc.pixel_errors == 1 and sc.cam_method == 1 and sc.rad_kind == 1


def test_refusals_of_mcarats_ng_scene_and_mca_exe(tmp_path):
    _, ab, a1 = _objects(11000.0)
    _, abs_sol, a1s = _objects(650.0)
    # mcarats_ng: solar sources, forward methods, and the two builds that are not served
    for a, b, kw in ((a1s, abs_sol, dict(pixel_errors=True)), (a1s, abs_sol, dict(source='solar+thermal', wavelength=3900.0, pixel_errors=True)),
                     (a1, ab, dict(source='thermal', pixel_errors=True)), (a1, ab, dict(source='thermal', view_method='forward', pixel_errors=True)),
                     (a1, ab, dict(source='thermal', camera_method='forward', pixel_errors=True, **IRRADIANCE)),
                     (a1, ab, dict(source='thermal', target='flux', pixel_errors=True)),
                     (a1, ab, dict(source='thermal', view_method='backward', view_profiles=True, pixel_errors=True)),
                     (a1, ab, dict(source='thermal', camera_method='backward', emission_weights=True, pixel_errors=True, **IRRADIANCE))):
        with pytest.raises(OSError) as err:
            _write(a, b, str(tmp_path/'bad'), **kw)
        assert 'pixel_errors' in str(err.value), (kw, str(err.value))
    # the namelist: the key without a backward route, with the weights or the profiles, and values other than 0 and 1
    cam = dict(Rad_mrkind=1, Rad_mvbwd=None, Rad_mbwd=1)
    for kw in (dict(Rad_mvbwd=None), dict(Rad_mvbwd=0), dict(Rad_mvprf=1), dict(Rad_mwgt=1, **cam), dict(Rad_mbwd=0, Rad_mrkind=1, Rad_mvbwd=None, Rad_nimg=2),
               dict(Rad_mserr=2), dict(Rad_mserr=-1), dict(Rad_mserr=0.5)):
        for check in (lambda n: _check_supported(n, None, solver=0), lambda n: Scene.from_nml(n, str(tmp_path), solver=0)):
            with pytest.raises(OSError) as err:
                check(_nml(**kw))
            assert 'Rad_mserr' in str(err.value), (kw, str(err.value))
    _check_supported(_nml(), None, solver=0); _check_supported(_nml(**cam), None, solver=0)
    _check_supported(_nml(Rad_mserr=0), None, solver=0); _check_supported(_nml(Rad_mserr=0, Rad_mvbwd=0), None, solver=0)
    assert Scene.from_nml(_nml(), str(tmp_path), solver=0).pixel_errors == 1 and Scene.from_nml(_nml(Rad_mserr=0), str(tmp_path), solver=0).pixel_errors == 0
    assert Scene.from_nml(_nml(**cam), str(tmp_path), solver=0).pixel_errors == 1
    base = dict(zgrd=[0.0, 1000.0], ext1d=[0.0], omg1d=[1.0], apf1d=[-1.0], abs1d=[1e-4], nx=1, ny=1, dx=1000.0, dy=1000.0, target=2,
                view_the=[180.0], view_phi=[0.0], view_zloc=[1e6], src_mtype=3, src_wlen=11.0, tmp1d=[290.0, 280.0])
    assert Scene(rad_kind=2, view_method=1, pixel_errors=1, **base).pixel_errors == 1 and Scene(rad_kind=2, view_method=1, **base).pixel_errors == 0
    assert Scene(rad_kind=1, cam_method=1, pixel_errors=1, cam_images=0, **base).pixel_errors == 1
    for kw in (dict(rad_kind=2, view_method=0, pixel_errors=1), dict(rad_kind=1, cam_method=0, pixel_errors=1, cam_images=0),
               dict(rad_kind=2, view_method=1, view_profiles=1, pixel_errors=1), dict(rad_kind=1, cam_method=1, cam_weights=1, pixel_errors=1, cam_images=0),
               dict(rad_kind=2, view_method=1, pixel_errors=2), dict(rad_kind=2, view_method=1, pixel_errors=-1),
               dict(rad_kind=2, view_method=1, pixel_errors=0.5)):
        with pytest.raises(ValueError) as err:
            Scene(**dict(base, **kw))
        assert 'Rad_mserr' in str(err.value), kw


def test_header_declares_what_the_binding_lists():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'mi3d.h')).read()
    declared = set(re.findall(r'^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(mi3d_\w+)\s*\(', text, flags=re.M))
    listed = {s[0]: s for s in solver_mod._SIGNATURES}
    for name in ('mi3d_set_pixel_errors', 'mi3d_bind_pixel_errors_buffer', 'mi3d_get_radiance_se'):
        assert name in declared and name in listed, name
    assert len(listed['mi3d_get_radiance_se'][2]) == 3 and len(listed['mi3d_set_pixel_errors'][2]) == 2
    for method in ('set_pixel_errors', 'radiance_se', 'run_until'):
        assert callable(getattr(solver_mod.Mi3dSolver, method))
    assert 'err_ptr' in inspect.signature(solver_mod.Mi3dSolver.bind).parameters
    assert list(inspect.signature(solver_mod.Mi3dSolver.run_until).parameters)[1:] == ['se_max', 'relative', 'max_histories', 'seed', 'chunk']
    # the contract text: the estimator, the clamp and the cancellation floor
    block = text[text.index('Per-pixel standard errors'):text.index('int mi3d_set_pixel_errors(')]
    for word in ('rad2', 'max(', 'n (n - 1)', '1e-6', 'MI3D_ESTATE', 'mi3d_reset', 'k_backward<C,S> [thermal]', 'k_backward<C,V,S> [thermal]'):
        assert word in block, word


@pytest.mark.parametrize('kind', ['views', 'radiometers'])
@pytest.mark.parametrize('nrun', [1, 3])
def test_err_bin_and_the_g_run_combination(tmp_path, kind, nrun):
    """synthetic standard errors through the .err.bin files and back through read_pixel_errors and mca_out_ng's readers, against a numpy
    restatement: per run rad_se_r^2 = sum_g f_g^2 se_g^2 with the float32 factors of g_factors, over runs sqrt(sum_r rad_se_r^2) / Nrun;
    float64 throughout and rounded to float32 once, so 2 x 2^-24 covers the reader's order of operations"""
    _, ab, a1 = _objects(11000.0)
    kw = dict(view_method='backward', sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0]) if kind == 'views' \
        else dict(camera_method='backward', **IRRADIANCE)
    m = _write(a1, ab, str(tmp_path/'v'), Nrun=nrun, source='thermal', pixel_errors=True, **kw)
    nml = mca.mca_inp_read(m.fnames_inp[0][0])
    nview, nyr, nxr = int(nml['Rad_nrad']), int(nml.get('Rad_nyr', 1)), int(nml.get('Rad_nxr', 1))
    assert nview == 2
    rng = np.random.default_rng(11)
    se = rng.uniform(0.01, 0.05, size=(nrun, m.Ng, nview, nyr, nxr)).astype(np.float32)
    rad = rng.uniform(5.0, 9.0, size=se.shape).astype(np.float32)
    for ir in range(nrun):
        for ig in range(m.Ng):
            fname = mca_exe.errors_fname(m.fnames_out[ir][ig])
            assert fname.endswith('.err.bin') and not fname.endswith('.out.bin.err.bin')
            r = mca_exe.JobRunner.__new__(mca_exe.JobRunner); r.rank = 0
            result = {'rad': rad[ir, ig], 'se': se[ir, ig]}
            if kind == 'radiometers':
                result['rdir'] = np.zeros_like(rad[ir, ig])
            r.write(m.fnames_out[ir][ig], result)
            assert os.path.getsize(fname) == 4*nview*nyr*nxr
            assert np.array_equal(mca_exe.read_errors(fname, nview, nyr, nxr), se[ir, ig])
    with pytest.raises(OSError):
        mca_exe.read_errors(fname, nview+1, nyr, nxr)
    # a job without the key writes no such file and the same out.bin and .ctl, byte for byte
    last = m.fnames_out[nrun-1][m.Ng-1]
    plain = str(tmp_path/'plain'/os.path.basename(last))
    r.write(plain, {k: v for k, v in result.items() if k != 'se'})
    assert sorted(os.listdir(str(tmp_path/'plain'))) == sorted(f for f in os.listdir(os.path.dirname(last))
                                                               if f.startswith(os.path.basename(last)[:-len('out.bin')]) and 'out.bin' in f)
    for f in os.listdir(str(tmp_path/'plain')):
        assert open(str(tmp_path/'plain'/f), 'rb').read() == open(os.path.join(os.path.dirname(last), f), 'rb').read(), f
    factors, _ = g_factors(m, ab, 1)
    f = factors[0].astype(np.float64)
    assert factors.dtype == np.float32 and np.array_equal(factors[0], np.float32(ab.coef['weight']['data']*1.0e-3))
    var = np.zeros((nrun, nview, nyr, nxr))
    for ir in range(nrun):
        for ig in range(m.Ng):
            var[ir] += (f[ig]*se[ir, ig].astype(np.float64))**2
    assert np.allclose(pixel_error_runs(se, np.repeat(factors, nview, axis=0)), var, rtol=1.0e-15, atol=0.0)
    lay = lambda a: np.transpose(a, (2, 1, 0)+tuple(range(3, a.ndim)))
    want = {'all': lay(np.moveaxis(np.sqrt(var), 0, -1)), 'mean': lay(np.sqrt(var.sum(axis=0))/nrun)}
    for mode in ('mean', 'all'):
        got, info = read_pixel_errors(m, ab, mode=mode, squeeze=False)
        assert got.dtype == np.float32 and got.shape == (nxr, nyr, nview, 1)+((nrun,) if mode == 'all' else ())
        assert info == ['Nx', 'Ny', 'Nz', 'Nt']+(['Nr'] if mode == 'all' else [])
        assert np.allclose(got[:, :, :, 0], want[mode], rtol=2.0*U24, atol=0.0), mode
        data = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        w = np.squeeze(want[mode]) if mode == 'mean' or nrun > 1 else np.squeeze(want[mode])[..., None]
        assert data['rad_se']['data'].shape == w.shape and np.allclose(data['rad_se']['data'], w, rtol=2.0*U24, atol=0.0), mode
        if kind == 'views':
            assert data['rad_se']['dims_info'] == data['rad']['dims_info'] and data['bt_se']['data'].shape == data['bt']['data'].shape
            d = dplanck_dT(m.wlen_um, data['bt']['data'].astype(np.float64))
            # bt_se dB/dT = rad_se (per um as bt takes it): bt_se rounded once, the product in float64
            assert np.allclose(data['bt_se']['data'].astype(np.float64)*d, data['rad_se']['data'].astype(np.float64)*1.0e3, rtol=2.0*U24, atol=0.0)
            assert 'f_se' not in data and data['bt_se']['data'].min() > 0.0
        else:
            assert np.array_equal(data['f_se']['data'], data['rad_se']['data']*np.float32(np.pi)) and data['f_se']['data'].shape == data['f']['data'].shape
            assert 'bt_se' not in data
        if mode == 'mean':
            assert 'rad_std' in data or 'f_std' in data        # (the spread over runs stays what it is)
    # without the switch the reader adds no key
    m.pixel_errors = False
    assert not any(k.endswith('_se') for k in mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data)
