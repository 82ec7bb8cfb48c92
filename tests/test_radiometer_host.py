"""
Point radiometers without a GPU: Scene.from_nml takes the rectangular pixel map (Rad_mpmap = 2) and the cosine weighting
(Rad_mrproj = 1) and refuses other values, mcarats_ng writes the documented namelist for sensor_type 'irradiance' / 'actinic'
while satellite and all-sky job files stay byte for byte what they were, and the rectangular map's pixel solid angles tile the
hemisphere.
"""

import contextlib
import io
import os

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd.scene import Scene
from er3t_amd.synth import atm_synth, abs_synth
from tests.golden import inputs as gin

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _camera_nml(**extra):
    nml = {'Wld_mtarget': 2, 'Atm_nz': 2, 'Atm_zgrd0': np.array([0.0, 1000.0, 2000.0]), 'Atm_np1d': 1,
           'Atm_ext1d(1:, 1)': np.array([1.0e-5, 1.0e-5]), 'Atm_omg1d(1:, 1)': np.array([1.0, 1.0]),
           'Atm_apf1d(1:, 1)': np.array([-1.0, -1.0]), 'Atm_abs1d(1:, 1)': np.array([0.0, 0.0]),
           'Src_flx': 1.0, 'Src_the': 150.0, 'Src_phi': 0.0, 'Src_qmax': 0.5,
           'Rad_mrkind': 1, 'Rad_nrad': 1, 'Rad_the': 0.0, 'Rad_phi': 0.0, 'Rad_zloc': 10.0, 'Rad_nxr': 1, 'Rad_nyr': 1,
           'Rad_umax': 90.0, 'Rad_vmax': 180.0}
    nml.update(extra)
    return nml


def test_scene_accepts_rectangular_map_and_cosine_weighting():
    sc = Scene.from_nml(_camera_nml(Rad_mpmap=2, Rad_mrproj=1))
    assert sc.rad_kind == 1 and sc.cam_mpmap == 2 and sc.cam_mrproj == 1
    assert sc.cam_umax == [90.0] and sc.cam_vmax == [180.0]
    sc0 = Scene.from_nml(_camera_nml(Rad_mpmap=2, Rad_mrproj=0))
    assert (sc0.cam_mpmap, sc0.cam_mrproj) == (2, 0)
    # a camera job without the keys: today's polar map and plain mean radiance
    sc1 = Scene.from_nml(_camera_nml())
    assert (sc1.cam_mpmap, sc1.cam_mrproj) == (1, 0)


@pytest.mark.parametrize('extra', [dict(Rad_mpmap=3), dict(Rad_mpmap=0), dict(Rad_mpmap=2, Rad_mrproj=2), dict(Rad_mrproj=-1)])
def test_scene_refuses_bad_map_or_weighting(extra):
    with pytest.raises(OSError):
        Scene.from_nml(_camera_nml(**extra))


def _objects():
    atm = atm_synth(np.arange(11)*1.0)                  # 10 layers of 1 km
    ab = abs_synth(650.0, atm, Ng=2)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    return ab, a1


def _sensors(fdir, **kw):
    ab, a1 = _objects()
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=2, target='radiance', surface_albedo=0.2, fdir=fdir, Nrun=1, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


@pytest.mark.parametrize('kind,mrproj', [('irradiance', 1), ('actinic', 0)])
def test_sensor_job_file(tmp_path, kind, mrproj):
    m = _sensors(str(tmp_path/kind), sensor_type=kind, sensor_zenith_angle=0.0, sensor_altitude=1500.0, sensor_xpos=0.25,
                 sensor_ypos=0.75)
    nml = mca.mca_inp_read(m.fnames_inp[0][0])
    assert nml['Wld_mtarget'] == 2 and nml['Rad_mrkind'] == 1 and nml['Rad_mpmap'] == 2 and nml['Rad_mrproj'] == mrproj
    assert nml['Rad_nxr'] == 1 and nml['Rad_nyr'] == 1 and nml['Rad_umax'] == 90.0 and nml['Rad_vmax'] == 180.0
    assert nml['Rad_nrad'] == 1 and nml['Rad_the'] == 0.0 and nml['Rad_zloc'] == 1500.0
    assert nml['Rad_xpos'] == 0.25 and nml['Rad_ypos'] == 0.75 and nml['Rad_apsize'] == 0.05
    assert 'Rad_qmax' not in nml                         # the full hemisphere around the axis (Rad_qmax defaults to 180)
    sc = Scene.from_nml(nml, os.path.dirname(m.fnames_inp[0][0]))
    assert sc.rad_kind == 1 and (sc.cam_mpmap, sc.cam_mrproj) == (2, mrproj) and sc.cam_qmax == [180.0]


def test_several_sensors_write_arrays(tmp_path):
    m = _sensors(str(tmp_path/'row'), sensor_type='irradiance', sensor_xpos=[0.1, 0.3, 0.5, 0.7], sensor_ypos=0.5,
                 sensor_altitude=[10.0, 10.0, 2000.0, 2000.0], sensor_zenith_angle=[0.0, 0.0, 180.0, 30.0], sensor_azimuth_angle=90.0)
    assert m.Nview == 4
    nml = mca.mca_inp_read(m.fnames_inp[0][1])
    assert nml['Rad_nrad'] == 4
    assert np.allclose(nml['Rad_xpos'], [0.1, 0.3, 0.5, 0.7]) and np.allclose(nml['Rad_ypos'], 0.5)
    assert np.allclose(nml['Rad_zloc'], [10.0, 10.0, 2000.0, 2000.0]) and np.allclose(nml['Rad_the'], [0.0, 0.0, 180.0, 30.0])
    assert np.allclose(nml['Rad_phi'], 0.0)              # an axis tilted towards the east: counter-clockwise from east, 0
    sc = Scene.from_nml(nml, os.path.dirname(m.fnames_inp[0][1]))
    assert sc.nview == 4 and sc.cam_xpos == [0.1, 0.3, 0.5, 0.7]


def test_sensor_errors(tmp_path):
    with pytest.raises(OSError):
        _sensors(str(tmp_path/'a'), sensor_type='irradiance', sensor_xpos=list(np.linspace(0.0, 1.0, 17)))
    with pytest.raises(OSError):
        _sensors(str(tmp_path/'b'), sensor_type='actinic', sensor_xpos=[0.1, 0.2], sensor_ypos=[0.1, 0.2, 0.3])
    ab, a1 = _objects()
    with pytest.raises(OSError), contextlib.redirect_stdout(io.StringIO()):
        mca.mcarats_ng(atm_1ds=[a1], Ng=2, target='flux', fdir=str(tmp_path/'c'), Nrun=1, photons=1e4, weights=ab.coef['weight']['data'],
                       mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, sensor_type='irradiance')


def _mask(text, tmp):
    lines = [' Wld_jseed       = <masked>' if l.startswith(' Wld_jseed') else l for l in text.split('\n')]
    return '\n'.join(lines).replace(tmp, '<fdir>')


@pytest.mark.parametrize('name', ['rad_allsky', 'rad_3d_hg'])
def test_satellite_and_allsky_job_files_unchanged(tmp_path, name):
    tmp = str(tmp_path)
    inp = gin.make_inputs()
    ad = gin.build_adapters(mca, inp, tmp)
    kw = gin.simulation_cases(ad['a1'], ad['a1b'], ad['a3'], ad['a3b'], ad['sca'], ad['s_l'], ad['s_b'], inp['abs'].coef['weight']['data'])[name]
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            m = mca.mcarats_ng(fdir='%s/%s' % (tmp, name), Nrun=2, Ncpu=2, mp_mode='sh', overwrite=True, date=gin.DATE, quiet=True, **kw)
    finally:
        os.chdir(cwd)
    for ig in (0, 15):
        got = _mask(open(m.fnames_inp[1][ig]).read(), tmp)
        assert got == open(os.path.join(GOLD, 'nml_%s_g%02d.txt' % (name, ig))).read(), (name, ig)
        assert 'Rad_mrproj' not in got


def rect_weights(n, m, umax=90.0, vmax=180.0, mrproj=0):
    """host restatement of the rectangular map's exact weighted pixel solid angles W[i, j] (include/mi3d.h: mi3d_set_camera_map)"""
    t = np.radians(umax)*np.arange(n+1)/n
    dphi = 2.0*np.radians(vmax)/m
    w = (np.cos(t[:-1])-np.cos(t[1:]))*dphi if mrproj == 0 else 0.5*(np.sin(t[1:])**2-np.sin(t[:-1])**2)*dphi
    return np.repeat(w[:, None], m, axis=1)


@pytest.mark.parametrize('n,m', [(1, 1), (9, 36), (90, 7)])
def test_rectangular_weights_tile_the_hemisphere(n, m):
    assert abs(rect_weights(n, m, mrproj=0).sum() - 2.0*np.pi) < 1e-12
    assert abs(rect_weights(n, m, mrproj=1).sum() - np.pi) < 1e-12
    assert np.all(rect_weights(n, m, mrproj=1) > 0.0)
    # the full sphere with umax = 180, unweighted
    assert abs(rect_weights(n, m, umax=180.0).sum() - 4.0*np.pi) < 1e-12
