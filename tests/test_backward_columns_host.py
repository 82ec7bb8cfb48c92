"""
The backward satellite views under independent columns and partial 3-D (mi3d_set_view_columns 1, Rad_mvcol = 1), host side:
job files, the round trip into a Scene, the refusals of every host layer, header against binding, and the float64 reference of
tests/backward_columns_ref.py against tests/thermal_camera_ref.py's march and against itself.  No GPU.
"""

import contextlib
import dataclasses
import io
import os
import re

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca.mca_exe import _check_supported, thermal_heating
from er3t_amd.rtm.mca.mca_inp import mca_inp_groups
from er3t_amd.scene import Scene
from er3t_amd.synth import atm_synth, abs_synth
from tests import backward_columns_ref as cref
from tests import backward_sun_ref as sref
from tests import backward_views_ref as vref
from tests import thermal_camera_ref as ref
from tests.golden import inputs as gin


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 2, 'Rad_mvbwd': 1, 'Rad_mvcol': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3,
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


def _write(a1, ab, fdir, target='radiance', **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=2, target=target, surface_albedo=0.03, fdir=fdir, Nrun=1, photons=1e4, abs_obj=ab,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


_text = lambda m: [l for l in open(m.fnames_inp[0][0]).read().splitlines() if 'Wld_jseed' not in l]
_bytes = lambda m: [l for l in open(m.fnames_inp[0][0], 'rb').read().split(b'\n') if b'Wld_jseed' not in l]
THE = dict(source='thermal')
MIX = dict(source='solar+thermal', solar_zenith_angle=40.0, solar_azimuth_angle=30.0)


def test_job_files_without_the_switch_are_byte_identical_and_the_switch_adds_one_line(tmp_path):
    """view_columns=False, and the argument omitted, write the same bytes -- thermal, mixed and solar jobs, forward and backward, every
    solver --, none with the key; the switch adds exactly one line, Rad_mvcol, in the Rad group"""
    _, ab, a1 = _objects(11000.0)
    jobs = [dict(THE), dict(THE, solver='ipa'), dict(THE, solver='p3d'), dict(THE, view_method='backward'),
            dict(THE, view_method='backward', pixel_errors=True), dict(THE, view_method='backward', view_profiles=True),
            dict(MIX), dict(MIX, view_method='backward', view_sunlight=True), dict(), dict(target='flux', solver='ipa')]
    for i, kw in enumerate(jobs):
        x = _bytes(_write(a1, ab, str(tmp_path/('a%d' % i)), **kw))
        y = _bytes(_write(a1, ab, str(tmp_path/('b%d' % i)), view_columns=False, **kw))
        assert x == y and not any(b'Rad_mvcol' in l for l in x), kw
    for i, kw in enumerate((dict(THE, solver='ipa'), dict(THE, solver='p3d', sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0]),
                            dict(THE, solver='ipa', pixel_errors=True), dict(THE, solver='ipa', view_profiles=True),
                            dict(MIX, solver='p3d', view_sunlight=True), dict(MIX, solver='ipa', view_sunlight=True, pixel_errors=True))):
        plain = {k: v for k, v in kw.items() if k not in ('pixel_errors', 'view_profiles', 'view_sunlight')}
        fwd = _write(a1, ab, str(tmp_path/('f%d' % i)), **plain)
        col = _write(a1, ab, str(tmp_path/('c%d' % i)), view_method='backward', view_columns=True, **kw)
        tf, tc = _text(fwd), _text(col)
        assert sum('Rad_mvcol' in l for l in tc) == 1 and sum('Rad_mvbwd' in l for l in tc) == 1
        assert [l for l in tc if not any(k in l for k in ('Rad_mvcol', 'Rad_mvbwd', 'Rad_mserr', 'Rad_mvprf', 'Rad_mvsun'))] == tf
        rad = tc[tc.index('&mcarRad_nml_job'):]
        assert any('Rad_mvcol' in l for l in rad[1:rad.index('/')])
        assert col.view_columns is True and fwd.view_columns is False
    groups = mca_inp_groups()
    assert [g for g, keys in groups.items() if 'Rad_mvcol' in keys] == [g for g, keys in groups.items() if 'Rad_mvbwd' in keys] != []


def test_round_trip_into_a_scene(tmp_path):
    _, ab, a1 = _objects(11000.0)
    for name, s in (('ipa', 2), ('p3d', 1)):
        col = _write(a1, ab, str(tmp_path/name), view_method='backward', view_columns=True, solver=name, pixel_errors=True,
                     sensor_zenith_angle=[0.0, 40.0], **THE)
        nml = mca.mca_inp_read(col.fnames_inp[0][0])
        assert nml['Rad_mvcol'] == 1 and nml['Rad_mvbwd'] == 1 and nml['Src_mtype'] == 3 and nml['Rad_mrkind'] == 2 and nml['Rad_mserr'] == 1
        _check_supported(nml, str(tmp_path/name), solver=s)
        sc = Scene.from_nml(nml, str(tmp_path/name), solver=s)
        assert sc.view_columns == 1 and sc.view_method == 1 and sc.rad_kind == 2 and sc.nview == 2 and sc.solver == s and sc.pixel_errors == 1
        assert thermal_heating(nml)                                # (job by job: every pixel is divided by its own count of histories)
        for check in (lambda: _check_supported(nml, str(tmp_path/name), solver=0), lambda: Scene.from_nml(nml, str(tmp_path/name), solver=0)):
            with pytest.raises(OSError) as err:                    # the same file handed to the 3-D solver
                check()
            assert 'Rad_mvcol' in str(err.value) and '3-D solver' in str(err.value)
    fwd = _write(a1, ab, str(tmp_path/'f'), solver='ipa', **THE)
    assert Scene.from_nml(mca.mca_inp_read(fwd.fnames_inp[0][0]), str(tmp_path/'f'), solver=2).view_columns == 0
    mix = _write(a1, ab, str(tmp_path/'m'), view_method='backward', view_columns=True, view_sunlight=True, solver='p3d', **MIX)
    nml = mca.mca_inp_read(mix.fnames_inp[0][0])
    _check_supported(nml, str(tmp_path/'m'), solver=1)
    sc = Scene.from_nml(nml, str(tmp_path/'m'), solver=1)
    assert sc.view_columns == 1 and sc.view_sunlight == 1 and sc.src_mtype == 2 and sc.solver == 1


def test_mcarats_ng_refuses_what_the_switch_does_not_serve(tmp_path):
    _, ab, a1 = _objects(11000.0)
    on = dict(view_method='backward', view_columns=True)
    cases = [(dict(THE, **on), '3d'), (dict(THE, **on, solver='3d'), '3d'),                                  # the switch belongs to IPA / P3D
             (dict(THE, view_columns=True, solver='ipa'), 'view_method'),                                    # ... and to the backward route
             (dict(THE, **on, solver='ipa', sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0), 'satellite'),
             (dict(THE, **on, solver='ipa', emission_weights=True), 'emission_weights')]
    for kw, word in cases:
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), **kw)
        assert ('Rad_mvcol' in str(err.value) or 'view_columns' in str(err.value)) and word in str(err.value), (kw, str(err.value))
    # without the switch independent columns and partial 3-D stay refused on the backward route, in the words they always met
    for s in ('ipa', 'p3d'):
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), view_method='backward', solver=s, **THE)
        assert str(err.value) == 'Error [mcarats_ng]: <view_method=\'backward\'> needs <solver=\'3d\'>: a line of sight crosses columns.'
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), view_method='backward', view_sunlight=True, solver=s, **MIX)
        assert 'view_sunlight' in str(err.value) and 'solver' in str(err.value)
    for kw in (dict(), dict(pixel_errors=True), dict(view_profiles=True)):
        assert _write(a1, ab, str(tmp_path/'ok'), solver='ipa', **on, **THE, **kw).view_columns is True
    assert _write(a1, ab, str(tmp_path/'ok'), solver='p3d', view_sunlight=True, pixel_errors=True, **on, **MIX).view_sunlight is True


def test_host_layers_refuse_in_words_that_name_the_key(tmp_path):
    checks = lambda s: (lambda n: _check_supported(n, None, solver=s), lambda n: Scene.from_nml(n, str(tmp_path), solver=s))
    for kw, word in ((dict(Rad_mvbwd=None), 'Rad_mvbwd'), (dict(Rad_mvbwd=0), 'Rad_mvbwd'), (dict(Rad_mvcol=2), 'not supported'),
                     (dict(Rad_mvcol=-1), 'not supported'), (dict(Rad_mvcol=0.5), 'not supported'),
                     (dict(Rad_mrkind=1, Rad_nimg=2), 'Rad_mrkind'), (dict(Rad_mwgt=1), 'Rad_mwgt')):
        for s in (1, 2):
            for check in checks(s):
                with pytest.raises(OSError) as err:
                    check(_nml(**kw))
                assert 'Rad_mvcol' in str(err.value) and word in str(err.value), (kw, str(err.value))
    for check in checks(0):                                        # the 3-D solver
        with pytest.raises(OSError) as err:
            check(_nml())
        assert 'Rad_mvcol' in str(err.value) and '3-D solver' in str(err.value)
    for s in (1, 2):
        for check in checks(s):
            with pytest.raises(OSError) as err:                    # the switch off: the refusal the solvers always met, in its words
                check(_nml(Rad_mvcol=None))
            assert 'Rad_mvbwd' in str(err.value) and 'Rad_mvcol' not in str(err.value)
            with pytest.raises(OSError) as err:
                check(_nml(Rad_mvcol=0))
            assert 'Rad_mvbwd' in str(err.value)
        _check_supported(_nml(), None, solver=s)
        sc = Scene.from_nml(_nml(), str(tmp_path), solver=s)
        assert sc.view_columns == 1 and sc.view_method == 1 and sc.solver == s
        for kw in (dict(Rad_mserr=1), dict(Rad_mvprf=1)):
            _check_supported(_nml(**kw), None, solver=s)
            assert Scene.from_nml(_nml(**kw), str(tmp_path), solver=s).view_columns == 1
    assert thermal_heating(_nml())
    base = dict(zgrd=[0.0, 1000.0], ext1d=[0.0], omg1d=[1.0], apf1d=[-1.0], abs1d=[1e-4], nx=1, ny=1, dx=1000.0, dy=1000.0, target=2,
                view_the=[180.0], view_phi=[0.0], view_zloc=[1e6], src_wlen=11.0, tmp1d=[290.0, 280.0], rad_kind=2, view_method=1, src_mtype=3)
    assert Scene(view_columns=1, solver=2, **base).view_columns == 1 and Scene(view_columns=1, solver=1, **base).view_columns == 1
    assert Scene(solver=2, **base).view_columns == 0              # (the library refuses it when it runs, as before)
    for kw, word in ((dict(view_columns=2, solver=2), 'must be'), (dict(view_columns=-1, solver=2), 'must be'), (dict(view_columns=0.5, solver=2), 'must be'),
                     (dict(view_columns=1, solver=0), '3-D solver'), (dict(view_columns=1), '3-D solver'),
                     (dict(view_columns=1, solver=2, view_method=0), 'view_method')):
        with pytest.raises(ValueError) as err:
            Scene(**dict(base, **kw))
        assert 'Rad_mvcol' in str(err.value) and word in str(err.value), kw


def test_header_declares_what_the_binding_lists():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'mi3d.h')).read()
    declared = set(re.findall(r'^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(mi3d_\w+)\s*\(', text, flags=re.M))
    listed = {s[0]: s for s in solver_mod._SIGNATURES}
    assert 'mi3d_set_view_columns' in declared and 'mi3d_set_view_columns' in listed
    assert len(listed['mi3d_set_view_columns'][2]) == 2
    assert re.search(r'int\s+mi3d_set_view_columns\s*\(\s*mi3d_solver\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;', text)
    assert hasattr(solver_mod.Mi3dSolver, 'set_view_columns')
    for word in ('k_backward<C,V,I> [thermal]', 'k_backward<C,V,I,S> [thermal]', 'k_backward<C,V,I,P> [thermal]', 'k_backward<C,V,I,N> [solar+thermal]',
                 'k_backward<C,V,I,N,S> [solar+thermal]', 'Rad_mvcol', 'parallax'):
        assert word in text, word


def test_the_reference_agrees_with_the_line_integral_and_with_itself():
    """a vertical line never leaves its column: there the column sum IS the 3-D line integral of tests/thermal_camera_ref.py; in a scene
    whose columns are all alike a slant line's is too; the float32 restatement lies within float32 of the float64 sum; a pixel that is a
    column has the column's value, and the 20 x 9 image averaged over whole columns gives the 6 x 5 image back"""
    sc = cref.columns(vref.absorbing_scene(albedo=0.0))
    rng = np.random.default_rng(5)
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    x, y = rng.uniform(0.0, Lx, 40), rng.uniform(0.0, Ly, 40)
    s = cref.line_scores(sc, 0, x, y)
    v, zs, zreg = vref.view_geometry(sc, 0)
    org = np.stack([x, y, np.full(40, min(zs, float(sc.zgrd[-1])))], axis=-1)
    want = ref.march(sc, org, np.broadcast_to(-v, org.shape))
    assert want.min() > 0.0 and np.abs(s/want-1.0).max() < 1.0e-13
    flat = dataclasses.replace(sc, extp=np.full_like(sc.extp, 0.0007), tmpa3d=np.full_like(sc.tmpa3d, -1.5))
    for iv in (1, 2):
        v, zs, zreg = vref.view_geometry(flat, iv)
        org = np.stack([x, y, np.full(40, zs)], axis=-1)
        want = ref.march(flat, org, np.broadcast_to(-v, org.shape))
        assert np.abs(cref.line_scores(flat, iv, x, y)/want-1.0).max() < 1.0e-12, iv
        rows, wts, _ = cref.line_terms(flat, iv, x, y)
        assert np.all(wts >= 0.0) and np.all(wts.sum(axis=1) <= 1.0+1.0e-12) and np.allclose(rows.sum(axis=1), want, rtol=1.0e-12)
    for iv in range(3):
        s64, s32 = cref.line_scores(sc, iv, x, y), cref.line_scores32(sc, iv, x, y)
        assert s64.min() > 0.0 and np.abs(s32/s64-1.0).max() < 2.0e-6, (iv, np.abs(s32/s64-1.0).max())
    # the slant view sees another image than the 3-D line integral through the same points: the switch has something to do
    v, zs, zreg = vref.view_geometry(sc, 1)
    org = np.stack([x, y, np.full(40, zs)], axis=-1)
    assert np.abs(cref.line_scores(sc, 1, x, y)/ref.march(sc, org, np.broadcast_to(-v, org.shape))-1.0).max() > 0.01
    small = cref.columns(vref.absorbing_scene(albedo=0.0, nxr=vref.NX, nyr=vref.NY))
    for iv in range(3):
        img = cref.column_image(small, iv)
        X, Y = np.meshgrid((np.arange(vref.NX)+0.3)*vref.DX, (np.arange(vref.NY)+0.8)*vref.DY)
        assert np.allclose(img, cref.line_scores(small, iv, X.ravel(), Y.ravel()).reshape(vref.NY, vref.NX), rtol=1.0e-13)
        big = cref.column_image(sc, iv)
        assert abs(big.mean()/img.mean()-1.0) < 1.0e-12           # (both are the mean over the domain)
    # a grey surface cut by the middle row of columns: the image depends on the folded position there, and the quadrature converges
    grey = cref.columns(vref.absorbing_scene(views=vref.VIEWS[:2], albedo=0.3, sfc2d=True))
    a, b = cref.column_image(grey, 1, nmu=16), cref.column_image(grey, 1, nmu=8)
    assert np.abs(a/b-1.0).max() < 1.0e-3 and a.min() > 0.0
    # the sun: a vertical sun's ray keeps its column whatever the solver
    sun = cref.columns(sref.absorbing_sunlit(180.0, 0.0), solver=1)
    a, b = cref.sun_surface_scores(sun, 1, x, y, True), cref.sun_surface_scores(sun, 1, x, y, False)
    assert a.min() > 0.0 and np.allclose(a, b, rtol=1.0e-12)
    slant = cref.columns(sref.absorbing_sunlit(120.0, 40.0), solver=1)
    a, b = cref.sun_surface_scores(slant, 1, x, y, True), cref.sun_surface_scores(slant, 1, x, y, False)
    assert np.abs(a/b-1.0).max() > 0.01
