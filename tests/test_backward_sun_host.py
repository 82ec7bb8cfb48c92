"""
The sunlight term of the backward satellite views (mi3d_set_view_sunlight 1, Rad_mvsun = 1), host side: job files, the round
trip into a Scene, the refusals of every host layer, header against binding, and the float64 reference of tests/backward_sun_ref.py against
itself.  No GPU.
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
from tests import backward_sun_ref as sref
from tests import backward_views_ref as vref
from tests.golden import inputs as gin


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 2, 'Rad_mvbwd': 1, 'Rad_mvsun': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 2,
           'Src_wlen': 3.75, 'Src_fsol': 10.0, 'Src_the': 140.0, 'Src_phi': 30.0, 'Src_qmax': 0.533, 'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1),
           'Sfc_mtype': 1, 'Atm_ext1d': np.zeros(nz), 'Atm_omg1d': np.ones(nz), 'Atm_apf1d': np.full(nz, -1.0), 'Atm_abs1d': np.full(nz, 1.0e-5),
           'Atm_nx': 1, 'Atm_ny': 1, 'Atm_dx': 1000.0, 'Atm_dy': 1000.0, 'Rad_the': 180.0, 'Rad_phi': 0.0, 'Rad_zloc': 1.0e6}
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
MIX = dict(source='solar+thermal', solar_zenith_angle=40.0, solar_azimuth_angle=30.0)


def test_job_files_without_the_switch_are_unchanged_and_the_switch_adds_one_line(tmp_path):
    """view_sunlight=False, and the argument omitted, write the same text -- mixed, thermal (forward and backward) and solar jobs --, none
    with the key; the switch adds exactly one line, Rad_mvsun, in the Rad group, beside the one of Rad_mvbwd"""
    _, ab, a1 = _objects(3750.0)
    jobs = [dict(MIX), dict(MIX, target='flux'), dict(source='thermal'), dict(source='thermal', view_method='backward'),
            dict(source='thermal', view_method='backward', pixel_errors=True), dict(), dict(target='flux')]
    for i, kw in enumerate(jobs):
        x = _text(_write(a1, ab, str(tmp_path/('a%d' % i)), **kw))
        y = _text(_write(a1, ab, str(tmp_path/('b%d' % i)), view_sunlight=False, **kw))
        assert x == y and not any('Rad_mvsun' in l for l in x), kw
    for i, kw in enumerate((dict(), dict(sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0]), dict(pixel_errors=True))):
        fwd = _write(a1, ab, str(tmp_path/('f%d' % i)), **MIX, **{k: v for k, v in kw.items() if k != 'pixel_errors'})
        sun = _write(a1, ab, str(tmp_path/('s%d' % i)), view_method='backward', view_sunlight=True, **MIX, **kw)
        tf, ts = _text(fwd), _text(sun)
        assert sum('Rad_mvsun' in l for l in ts) == 1 and sum('Rad_mvbwd' in l for l in ts) == 1
        assert [l for l in ts if not any(k in l for k in ('Rad_mvsun', 'Rad_mvbwd', 'Rad_mserr'))] == tf
        rad = ts[ts.index('&mcarRad_nml_job'):]
        assert any('Rad_mvsun' in l for l in rad[1:rad.index('/')])
        assert sun.view_sunlight is True and fwd.view_sunlight is False
    groups = mca_inp_groups()
    assert [g for g, keys in groups.items() if 'Rad_mvsun' in keys] == [g for g, keys in groups.items() if 'Rad_mvbwd' in keys] != []


def test_round_trip_into_a_sunlit_scene(tmp_path):
    _, ab, a1 = _objects(3750.0)
    sun = _write(a1, ab, str(tmp_path/'s'), view_method='backward', view_sunlight=True, sensor_zenith_angle=[0.0, 40.0], **MIX)
    nml = mca.mca_inp_read(sun.fnames_inp[0][0])
    assert nml['Rad_mvsun'] == 1 and nml['Rad_mvbwd'] == 1 and nml['Src_mtype'] == 2 and nml['Rad_mrkind'] == 2 and nml['Src_fsol'] > 0.0
    _check_supported(nml, str(tmp_path/'s'), solver=0)
    sc = Scene.from_nml(nml, str(tmp_path/'s'), solver=0)
    assert sc.view_sunlight == 1 and sc.view_method == 1 and sc.rad_kind == 2 and sc.nview == 2 and sc.src_mtype == 2
    assert sc.src_the == 140.0 and sc.src_qmax == nml['Src_qmax'] and 0.5 < sc.src_qmax < 0.6 and sc.src_fsol == nml['Src_fsol']
    assert thermal_heating(nml)                                   # (job by job: every pixel is divided by its own count of histories)
    fwd = _write(a1, ab, str(tmp_path/'f'), sensor_zenith_angle=[0.0, 40.0], **MIX)
    assert Scene.from_nml(mca.mca_inp_read(fwd.fnames_inp[0][0]), str(tmp_path/'f'), solver=0).view_sunlight == 0


def test_mcarats_ng_refuses_what_the_switch_does_not_serve(tmp_path):
    _, ab, a1 = _objects(3750.0)
    on = dict(view_method='backward', view_sunlight=True)
    cases = [dict(on, source='solar'), dict(on, source='thermal'),                                            # the switch belongs to the mixed source
             dict(MIX, view_sunlight=True),                                                                    # ... and to the backward route
             dict(MIX, **on, view_profiles=True), dict(MIX, view_method='backward', view_sunlight=True, emission_weights=True),
             dict(on, source='solar+thermal', solar_zenith_angle=90.0),
             dict(MIX, **on, sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0), dict(MIX, **on, solver='ipa'),
             dict(MIX, **on, target='flux')]
    for kw in cases:
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), **kw)
        assert 'Rad_mvsun' in str(err.value) or 'view_sunlight' in str(err.value), (kw, str(err.value))
    # without the switch the mixed source stays refused on the backward route, in the words it always had
    with pytest.raises(OSError) as err:
        _write(a1, ab, str(tmp_path/'bad'), view_method='backward', **MIX)
    assert 'thermal' in str(err.value) and 'view_method' in str(err.value)
    with pytest.raises(OSError) as err:
        _write(a1, ab, str(tmp_path/'bad'), view_method='backward', pixel_errors=True, **MIX)
    assert 'thermal' in str(err.value)
    assert _write(a1, ab, str(tmp_path/'ok'), pixel_errors=True, **on, **MIX).pixel_errors is True


def test_host_layers_refuse_in_words_that_name_the_key(tmp_path):
    bad = [dict(Src_mtype=1, Src_wlen=None, Src_fsol=None), dict(Src_mtype=3, Src_fsol=None), dict(Rad_mvbwd=None), dict(Rad_mvbwd=0),
           dict(Rad_mvprf=1), dict(Rad_mvsun=2), dict(Rad_mvsun=-1), dict(Rad_mvsun=0.5)]
    for kw in bad:
        for check in (lambda n: _check_supported(n, None, solver=0), lambda n: Scene.from_nml(n, str(tmp_path), solver=0)):
            with pytest.raises(OSError) as err:
                check(_nml(**kw))
            assert 'Rad_mvsun' in str(err.value), (kw, str(err.value))
    for kw in (dict(Src_the=90.0), dict(Src_the=60.0), dict(Src_the=90.2)):     # on the horizon, from below, the cone reaches the horizon
        with pytest.raises(OSError) as err:
            _check_supported(_nml(**kw), None, solver=0)
        assert 'Rad_mvsun' in str(err.value)
        with pytest.raises((OSError, ValueError)) as err:
            Scene.from_nml(_nml(**kw), str(tmp_path), solver=0)
        assert 'Rad_mvsun' in str(err.value)
    for check in (lambda n: _check_supported(n, None, solver=0), lambda n: Scene.from_nml(n, str(tmp_path), solver=0)):
        for kw in (dict(Rad_mrkind=1, Rad_nimg=2), dict(Rad_mwgt=1)):   # cameras and point radiometers; emission weights
            with pytest.raises(OSError) as err:
                check(_nml(**kw))
            assert 'Rad_mvsun' in str(err.value), (kw, str(err.value))
        with pytest.raises(OSError) as err:                        # the switch off: the refusal the mixed source always met, in its words
            check(_nml(Rad_mvsun=None))
        assert 'Rad_mvbwd' in str(err.value)
    for s in (1, 2):                                               # independent columns and partial 3-D
        for check in (lambda n: _check_supported(n, None, solver=s), lambda n: Scene.from_nml(n, str(tmp_path), solver=s)):
            with pytest.raises(OSError):
                check(_nml())
    _check_supported(_nml(), None, solver=0)
    sc = Scene.from_nml(_nml(), str(tmp_path), solver=0)
    assert sc.view_sunlight == 1 and sc.view_method == 1 and sc.src_mtype == 2
    assert thermal_heating(_nml())
    base = dict(zgrd=[0.0, 1000.0], ext1d=[0.0], omg1d=[1.0], apf1d=[-1.0], abs1d=[1e-4], nx=1, ny=1, dx=1000.0, dy=1000.0, target=2,
                view_the=[180.0], view_phi=[0.0], view_zloc=[1e6], src_wlen=3.75, tmp1d=[290.0, 280.0], rad_kind=2, view_method=1,
                src_mtype=2, src_fsol=10.0, src_the=150.0)
    assert Scene(view_sunlight=1, **base).view_sunlight == 1 and Scene(**base).view_sunlight == 0
    for kw in (dict(view_sunlight=2), dict(view_sunlight=-1), dict(view_sunlight=0.5), dict(view_sunlight=1, src_mtype=3, src_fsol=None),
               dict(view_sunlight=1, src_mtype=1), dict(view_sunlight=1, view_method=0), dict(view_sunlight=1, view_profiles=1),
               dict(view_sunlight=1, src_the=90.0), dict(view_sunlight=1, src_the=30.0), dict(view_sunlight=1, src_the=90.2, src_qmax=0.533)):
        with pytest.raises(ValueError) as err:
            Scene(**dict(base, **kw))
        assert 'Rad_mvsun' in str(err.value), kw


def test_header_declares_what_the_binding_lists():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'mi3d.h')).read()
    declared = set(re.findall(r'^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(mi3d_\w+)\s*\(', text, flags=re.M))
    listed = {s[0]: s for s in solver_mod._SIGNATURES}
    assert 'mi3d_set_view_sunlight' in declared and 'mi3d_set_view_sunlight' in listed
    assert len(listed['mi3d_set_view_sunlight'][2]) == 2
    assert re.search(r'int\s+mi3d_set_view_sunlight\s*\(\s*mi3d_solver\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;', text)
    assert hasattr(solver_mod.Mi3dSolver, 'set_view_sunlight')


def test_the_reference_agrees_with_itself():
    """a vertical ray through a column is the column's sum; a slant ray of more than one domain length is the sum of its folded pieces, each
    started where the last one left its own copy of the domain"""
    sc = sref.scattering_sunlit(120.0, 40.0, 10.0)
    ke = sref.extinction(sc)
    dz = np.diff(np.asarray(sc.zgrd, dtype=np.float64))
    for ix, iy in ((0, 0), (3, 2), (5, 4)):
        p = np.array([(ix+0.37)*sc.dx, (iy+0.61)*sc.dy, 0.0])
        tau, xy = sref.tau_line(sc, p, [0.0, 0.0, 1.0])
        assert abs(tau[0]-(ke[:, iy, ix]*dz).sum()) <= 1.0e-14*tau[0] and np.allclose(xy[0], p[:2])
        down, _ = sref.tau_line(sc, p+[0.0, 0.0, float(sc.zgrd[-1])], [0.0, 0.0, -1.0])
        assert abs(down[0]-tau[0]) <= 1.0e-14*tau[0]
    up = -sref.sun_direction(120.0, 40.0)
    Lx, Ly, ztop = sc.nx*sc.dx, sc.ny*sc.dy, float(sc.zgrd[-1])
    p = np.array([1700.0, 1100.0, 0.0])
    whole, end = sref.tau_line(sc, p, up)
    assert abs(end[0, 0]-p[0]) > Lx and abs(end[0, 1]-p[1]) > Ly            # 2.6 km horizontally: the ray wraps in x and in y
    # the pieces: cut the ray at the heights where it leaves a copy of the domain in x or y, fold the cut points, and march each piece in a
    # scene that ends at the cut (a top lowered to it)
    ts = sorted({t for L, u, x0 in ((Lx, up[0], p[0]), (Ly, up[1], p[1])) for m in range(-3, 4) if u != 0.0
                 for t in [((m*L)-x0)/u] if 0.0 < t < ztop/up[2]})
    assert len(ts) >= 2
    total, t0 = 0.0, 0.0
    for t1 in ts+[ztop/up[2]]:
        a = p+up*t0
        a = np.array([np.mod(a[0], Lx), np.mod(a[1], Ly), a[2]])
        b = p+up*0.5*(t0+t1)
        a[0] = np.mod(b[0], Lx)-up[0]*0.5*(t1-t0); a[1] = np.mod(b[1], Ly)-up[1]*0.5*(t1-t0)      # (the start inside the copy the piece lies in)
        zt = min(p[2]+up[2]*t1, ztop)
        k1 = int(np.searchsorted(np.asarray(sc.zgrd), zt, side='left'))
        zg = np.concatenate([np.asarray(sc.zgrd, dtype=np.float64)[:k1], [zt]])
        nzp = zg.size-1
        cut = dataclasses.replace(sc, zgrd=zg, ext1d=sc.ext1d[:, :nzp], omg1d=sc.omg1d[:, :nzp], apf1d=sc.apf1d[:, :nzp], abs1d=sc.abs1d[:nzp],
                                  tmp1d=np.asarray(sc.tmp1d)[:nzp+1], nz3=min(sc.nz3, nzp), extp=sc.extp[:, :min(sc.nz3, nzp)],
                                  omgp=sc.omgp[:, :min(sc.nz3, nzp)], apfp=sc.apfp[:, :min(sc.nz3, nzp)])
        piece, _ = sref.tau_line(cut, a, up)
        total += piece[0]
        t0 = t1
    assert abs(total-whole[0]) <= 1.0e-12*whole[0], (total, whole[0])
    # the closed-form scene of the GPU test: nothing emits at 20 K in float32, and its references are positive
    from er3t_amd.thermal import planck
    assert np.float32(planck(sref.WL, sref.COLD+6.0)) == 0.0
    ab = sref.absorbing_sunlit(120.0, 40.0)
    st = np.array([[100.0, 200.0, 1500.0], [900.0, 700.0, 1500.0]])
    s, hit = sref.surface_scores(ab, st, np.broadcast_to([0.0, 0.0, -1.0], st.shape))
    assert np.all(s > 0.0) and np.allclose(hit, st[:, :2])
    assert vref.NX*vref.DX < 1500.0*np.tan(np.radians(60.0))
