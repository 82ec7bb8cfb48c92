"""
Backward Monte Carlo for the satellite views of thermal jobs without a GPU: the namelist key Rad_mvbwd through mcarats_ng,
mca_exe's checks and Scene.from_nml; that every other job file stays byte for byte what it was; that the header declares what the ctypes
binding lists; and that the float64 reference of the GPU tests (tests/backward_views_ref.py) converges in its own quadrature.
"""

import contextlib
import io
import re

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca.mca_exe import _check_supported, thermal_heating
from er3t_amd.scene import Scene
from er3t_amd.synth import atm_synth, abs_synth
from tests import backward_views_ref as vref
from tests.golden import inputs as gin


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 2, 'Rad_mvbwd': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3, 'Src_wlen': 11.0,
           'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1, 'Atm_ext1d': np.zeros(nz), 'Atm_omg1d': np.ones(nz),
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


def _write(a1, ab, fdir, target='radiance', **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=2, target=target, surface_albedo=0.03, fdir=fdir, Nrun=1, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


_text = lambda m: [l for l in open(m.fnames_inp[0][0]).read().splitlines() if 'Wld_jseed' not in l]
IRRADIANCE = dict(sensor_type='irradiance', sensor_xpos=[0.2, 0.7], sensor_ypos=0.5, sensor_altitude=10.0, sensor_zenith_angle=[0.0, 180.0])


def test_forward_job_files_are_unchanged_and_backward_adds_one_line(tmp_path):
    """view_method='forward', and the argument omitted, write the same text: thermal satellite, flux, sensor and solar jobs; 'backward' adds
    exactly one line, Rad_mvbwd, in the Rad group"""
    _, ab, a1 = _objects(11000.0)
    _, abs_sol, a1s = _objects(650.0)
    jobs = [(a1, ab, dict(source='thermal')), (a1, ab, dict(source='thermal', sensor_zenith_angle=[0.0, 40.0])),
            (a1, ab, dict(source='thermal', target='flux')), (a1, ab, dict(source='thermal', **IRRADIANCE)),
            (a1, ab, dict(source='thermal', camera_method='backward', **IRRADIANCE)), (a1s, abs_sol, dict()), (a1s, abs_sol, dict(target='flux')),
            (a1s, abs_sol, dict(**IRRADIANCE))]
    for i, (a, b, kw) in enumerate(jobs):
        x = _text(_write(a, b, str(tmp_path/('a%d' % i)), **kw))
        y = _text(_write(a, b, str(tmp_path/('b%d' % i)), view_method='forward', **kw))
        assert x == y and not any('Rad_mvbwd' in l for l in x), kw
    for i, kw in enumerate((dict(), dict(sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0]))):
        fwd = _write(a1, ab, str(tmp_path/('f%d' % i)), source='thermal', **kw)
        bwd = _write(a1, ab, str(tmp_path/('v%d' % i)), source='thermal', view_method='backward', **kw)
        tf, tb = _text(fwd), _text(bwd)
        assert sum('Rad_mvbwd' in l for l in tb) == 1 and [l for l in tb if 'Rad_mvbwd' not in l] == tf
        rad = tb[tb.index('&mcarRad_nml_job'):]
        assert any('Rad_mvbwd' in l for l in rad[1:rad.index('/')])
        assert bwd.view_method == 'backward' and fwd.view_method == 'forward'


def test_round_trip_into_a_backward_scene(tmp_path):
    _, ab, a1 = _objects(11000.0)
    bwd = _write(a1, ab, str(tmp_path/'v'), source='thermal', view_method='backward', sensor_zenith_angle=[0.0, 40.0])
    fwd = _write(a1, ab, str(tmp_path/'f'), source='thermal', sensor_zenith_angle=[0.0, 40.0])
    nml = mca.mca_inp_read(bwd.fnames_inp[0][0])
    assert nml['Rad_mvbwd'] == 1 and nml['Src_mtype'] == 3 and nml['Rad_mrkind'] == 2 and 'Rad_mbwd' not in nml
    _check_supported(nml, str(tmp_path/'v'), solver=0)
    sc = Scene.from_nml(nml, str(tmp_path/'v'), solver=0)
    assert sc.view_method == 1 and sc.cam_method == 0 and sc.rad_kind == 2 and sc.nview == 2 and sc.src_mtype == 3
    assert thermal_heating(nml)                                   # (job by job: every pixel is divided by its own count of histories)
    nmf = mca.mca_inp_read(fwd.fnames_inp[0][0])
    assert Scene.from_nml(nmf, str(tmp_path/'f'), solver=0).view_method == 0 and not thermal_heating(nmf)


def test_mcarats_ng_refuses_what_the_route_does_not_serve(tmp_path):
    _, ab, a1 = _objects(11000.0)
    cases = [(dict(view_method='backward'), 'thermal'),                                                       # a solar source
             (dict(view_method='backward', source='solar+thermal'), 'thermal'),
             (dict(view_method='backward', source='thermal', target='flux'), 'radiance'),                     # a flux target
             (dict(view_method='backward', source='thermal', sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0), 'satellite'),
             (dict(view_method='backward', source='thermal', solver='ipa'), 'solver'),
             (dict(view_method='sideways', source='thermal'), 'view_method'),                                 # a misspelt method
             (dict(view_method='backward', source='thermal', emission_weights=True), 'emission_weights')]
    for kw, word in cases:
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), **kw)
        assert word in str(err.value) and 'view_method' in str(err.value), (kw, str(err.value))


def test_host_layers_refuse_in_words_that_name_the_key(tmp_path):
    bad = [dict(Rad_mrkind=1, Rad_nimg=2), dict(Src_mtype=1, Src_wlen=None), dict(Src_mtype=2, Src_fsol=5.0), dict(Wld_mtarget=1, Flx_mflx=1),
           dict(Rad_mvbwd=2), dict(Rad_mvbwd=-1), dict(Rad_mvbwd=0.5)]
    for kw in bad:
        for check in (lambda n: _check_supported(n, None, solver=0), lambda n: Scene.from_nml(n, str(tmp_path), solver=0)):
            with pytest.raises(OSError) as err:
                check(_nml(**kw))
            assert 'Rad_mvbwd' in str(err.value), (kw, str(err.value))
    for s in (1, 2):                                               # independent columns and partial 3-D
        for check in (lambda n: _check_supported(n, None, solver=s), lambda n: Scene.from_nml(n, str(tmp_path), solver=s)):
            with pytest.raises(OSError) as err:
                check(_nml())
            assert 'Rad_mvbwd' in str(err.value)
    _check_supported(_nml(), None, solver=0); _check_supported(_nml(Rad_mvbwd=0), None, solver=2)
    assert Scene.from_nml(_nml(), str(tmp_path), solver=0).view_method == 1
    base = dict(zgrd=[0.0, 1000.0], ext1d=[0.0], omg1d=[1.0], apf1d=[-1.0], abs1d=[1e-4], nx=1, ny=1, dx=1000.0, dy=1000.0, target=2,
                view_the=[180.0], view_phi=[0.0], view_zloc=[1e6], src_mtype=3, src_wlen=11.0, tmp1d=[290.0, 280.0])
    assert Scene(rad_kind=2, view_method=1, **base).view_method == 1 and Scene(rad_kind=2, **base).view_method == 0
    for kw in (dict(rad_kind=1, view_method=1), dict(rad_kind=2, view_method=2), dict(rad_kind=2, view_method=-1), dict(rad_kind=2, view_method=0.5)):
        with pytest.raises(ValueError) as err:
            Scene(**dict(base, **kw))
        assert 'Rad_mvbwd' in str(err.value)


def test_header_declares_what_the_binding_lists():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'mi3d.h')).read()
    declared = set(re.findall(r'^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(mi3d_\w+)\s*\(', text, flags=re.M))
    listed = {s[0] for s in solver_mod._SIGNATURES}
    assert 'mi3d_set_view_method' in declared and 'mi3d_debug_backward_views' in declared
    for name in ('mi3d_set_view_method', 'mi3d_debug_backward_views'):
        assert name in listed


def test_the_reference_converges_in_its_own_quadrature():
    """the pixel means of the non-scattering scene by 4 x 4 and by 8 x 8 Gauss-Legendre points per pixel differ by less than 1e-4 relative,
    in every pixel of every view"""
    sc = vref.absorbing_scene()
    for iv in range(sc.nview):
        a, b = vref.view_image(sc, iv, 4), vref.view_image(sc, iv, 8)
        gap = np.abs(a/b-1.0).max()
        print('view %d: 4 x 4 against 8 x 8 points, largest relative gap %.3e' % (iv, gap))
        assert b.min() > 0.0 and gap < 1.0e-4, (iv, gap)
