"""
Backward Monte Carlo for the cameras and point radiometers of thermal jobs without a GPU: the namelist key Rad_mbwd
through mcarats_ng, mca_exe's checks and Scene.from_nml; that every other job file stays byte for byte what it was; and that the header
declares what the ctypes binding lists.
"""

import contextlib
import io
import os
import re

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca.mca_exe import _check_supported, thermal_heating
from er3t_amd.scene import Scene, TARGET_RADIANCE
from er3t_amd.synth import atm_synth, abs_synth
from tests.golden import inputs as gin


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 1, 'Rad_mbwd': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3, 'Src_wlen': 11.0,
           'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1}
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


SENSORS = {'all-sky': dict(sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0),
           'irradiance': dict(sensor_type='irradiance', sensor_xpos=[0.2, 0.7], sensor_ypos=0.5, sensor_altitude=10.0, sensor_zenith_angle=[0.0, 180.0]),
           'actinic': dict(sensor_type='actinic', sensor_altitude=500.0, sensor_zenith_angle=0.0)}

_text = lambda m: [l for l in open(m.fnames_inp[0][0]).read().splitlines() if 'Wld_jseed' not in l]


def test_mca_exe_accepts_rad_mbwd_for_thermal_cameras_only():
    _check_supported(_nml())                                   # without Rad_nimg: the backward route needs none
    _check_supported(_nml(Rad_nimg=2))                         # (either key opens the job)
    _check_supported(_nml(Rad_mbwd=0, Rad_nimg=1))
    with pytest.raises(OSError) as err:
        _check_supported(_nml(Rad_mbwd=None))                  # neither key: refused as before
    assert 'Rad_nimg' in str(err.value)
    with pytest.raises(OSError) as err:
        _check_supported(_nml(Rad_mbwd=0))
    assert 'Rad_nimg' in str(err.value)
    for bad in (2, -1, 0.5):
        with pytest.raises(OSError) as err:
            _check_supported(_nml(Rad_mbwd=bad))
        assert 'Rad_mbwd' in str(err.value)
    solar = dict(Src_mtype=1, Src_wlen=None, Atm_tmp1d=np.linspace(290.0, 230.0, 4))
    others = (solar,                                                           # a solar camera
              dict(Src_mtype=2, Src_fsol=10.0),                                # a solar+thermal camera
              dict(Rad_mrkind=2),                                              # a thermal satellite view
              dict(Wld_mtarget=1, Rad_mrkind=None, Flx_mflx=1, Flx_mhrt=0))    # a thermal flux job
    for kw in others:
        with pytest.raises(OSError) as err:
            _check_supported(_nml(**kw))
        assert 'Rad_mbwd=1' in str(err.value) and 'thermal' in str(err.value), kw
        _check_supported(_nml(Rad_mbwd=0, **kw)) if kw is solar else None
    assert thermal_heating(_nml())                             # several ranks take these jobs one by one


def test_scene_refuses_rad_mbwd_elsewhere():
    base = dict(zgrd=np.arange(5)*1000.0, ext1d=np.zeros(4), omg1d=np.ones(4), apf1d=np.full(4, -1.0), abs1d=np.full(4, 1e-4),
                target=TARGET_RADIANCE, view_the=[0.0], view_phi=[0.0], view_zloc=[10.0], src_mtype=3, src_wlen=11.0,
                tmp1d=np.linspace(290.0, 230.0, 5))
    assert Scene(rad_kind=1, cam_method=1, **base).cam_method == 1 and Scene(rad_kind=1, **base).cam_method == 0
    with pytest.raises(ValueError) as err:
        Scene(rad_kind=2, cam_method=1, **base)
    assert 'Rad_mbwd' in str(err.value)
    with pytest.raises(ValueError):
        Scene(rad_kind=1, cam_method=2, **base)
    for kw in (dict(Src_mtype=1, Src_wlen=None), dict(Rad_mrkind=2), dict(Rad_mbwd=3)):
        with pytest.raises(OSError) as err:
            Scene.from_nml(_nml(**kw), '.', solver=0)
        assert 'Rad_mbwd' in str(err.value)


@pytest.mark.parametrize('kind', sorted(SENSORS))
def test_backward_job_files_and_round_trip(tmp_path, kind):
    """Rad_mbwd = 1 in the Rad group and no Rad_nimg; the rest of the file is the forward job's; the file parses back into a backward Scene"""
    atm, ab, a1 = _objects(11000.0)
    fwd = _write(a1, ab, str(tmp_path/'fwd'), source='thermal', **SENSORS[kind])
    bwd = _write(a1, ab, str(tmp_path/'bwd'), source='thermal', camera_method='backward', **SENSORS[kind])
    tf, tb = _text(fwd), _text(bwd)
    assert sum('Rad_mbwd' in l for l in tb) == 1 and not any('Rad_nimg' in l for l in tb)
    assert sum('Rad_nimg' in l for l in tf) == 1 and not any('Rad_mbwd' in l for l in tf)
    assert [l for l in tb if 'Rad_mbwd' not in l] == [l for l in tf if 'Rad_nimg' not in l]
    rad = tb[tb.index('&mcarRad_nml_job'):]
    assert any('Rad_mbwd' in l for l in rad[1:rad.index('/')])
    nml = mca.mca_inp_read(bwd.fnames_inp[0][0])
    assert nml['Rad_mbwd'] == 1 and 'Rad_nimg' not in nml and nml['Src_mtype'] == 3 and nml['Rad_mrkind'] == 1
    _check_supported(nml)
    sc = Scene.from_nml(nml, str(tmp_path), solver=0)
    assert sc.cam_method == 1 and sc.cam_images == -1 and sc.src_mtype == 3 and sc.rad_kind == 1
    assert sc.cam_mpmap == (1 if kind == 'all-sky' else 2) and sc.cam_mrproj == (1 if kind == 'irradiance' else 0)
    assert Scene.from_nml(mca.mca_inp_read(fwd.fnames_inp[0][0]), str(tmp_path), solver=0).cam_method == 0
    assert bwd.camera_method == 'backward' and fwd.camera_method == 'forward'


def test_every_other_job_file_is_what_it_was(tmp_path):
    """camera_method='forward' (the default) writes no new key: thermal and solar sensor jobs, satellite and flux jobs carry the text
    they carried (tests/test_thermal_camera_host.py holds what that text is)"""
    atm, ab, a1 = _objects(11000.0)
    jobs = [dict(source='thermal', **SENSORS['irradiance']), dict(source='thermal', camera_images=1, **SENSORS['all-sky']),
            dict(source='thermal'), dict(source='thermal', target='flux'), dict(source='thermal', target='heating rate'),
            dict(**SENSORS['all-sky']), dict(camera_images=3, **SENSORS['actinic']), dict(), dict(target='flux')]
    for i, kw in enumerate(jobs):
        a = _text(_write(a1, ab, str(tmp_path/('a%d' % i)), **kw))
        b = _text(_write(a1, ab, str(tmp_path/('b%d' % i)), camera_method='forward', **kw))
        assert a == b and not any('Rad_mbwd' in l for l in a), kw


def test_mcarats_ng_refusals(tmp_path):
    atm, ab, a1 = _objects(11000.0)
    cases = [(dict(camera_method='backward', **SENSORS['irradiance']), 'thermal'),                              # a solar job
             (dict(camera_method='backward', source='thermal'), 'sensor_type'),                                   # a satellite view
             (dict(camera_method='backward', source='thermal', target='flux'), 'sensor_type'),                    # a flux job
             (dict(camera_method='backward', source='thermal', camera_images=2, **SENSORS['irradiance']), 'camera_images'),
             (dict(camera_method='sideways', source='thermal', **SENSORS['irradiance']), 'camera_method')]
    for kw, word in cases:
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), **kw)
        assert word in str(err.value), (kw, str(err.value))
    with pytest.raises(OSError):
        _write(a1, ab, str(tmp_path/'bad'), camera_method='backward', source='solar+thermal', **SENSORS['irradiance'])


def test_header_declares_what_the_binding_lists():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'mi3d.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(mi3d_[a-z0-9_]+)\s*\(', text))
    listed = [name for name, _, _ in solver_mod._SIGNATURES]
    assert set(listed) == declared, (set(listed) ^ declared)
    assert 'mi3d_set_camera_method' in declared and 'mi3d_debug_backward' in declared
    # the argument counts of the two new entry points
    sig = dict((n, a) for n, _, a in solver_mod._SIGNATURES)
    for name in ('mi3d_set_camera_method', 'mi3d_debug_backward'):
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert m and len(m.group(1).split(',')) == len(sig[name]), name
