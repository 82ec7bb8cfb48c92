"""
Solar+thermal source (Src_mtype = 2) without a GPU: the job files mcarats_ng(source='solar+thermal') writes -- and that solar and
thermal job files carry no Src_fsol --, the round trip through mca_inp_read and Scene.from_nml, mca_exe's refusals, Scene's own
validation, and mca_out_ng's g-combination of mixed outputs (the thermal g-sum, the solar route's toa, a brightness temperature).
"""

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd.rtm.mca.mca_exe import _check_supported, thermal_heating
from er3t_amd.rtm.mca.mca_out import mca_out_write
from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_HEAT
from er3t_amd.synth import atm_synth, abs_synth
from er3t_amd.thermal import planck, brightness_temperature
from er3t_amd.util import cal_sol_fac
from tests.golden import inputs as gin
from tests.test_thermal_host import _objects, _write, _thermal_nml, _Files

WVL = 3750.0      # nm


def test_mixed_job_files(tmp_path):
    atm, ab, a1 = _objects(tmp_path, WVL)
    assert a1.abs is ab
    ab.coef['solar']['data'] = np.array([8.0, 9.5, 10.0, 11.25])*1.0e-3     # W m-2 nm-1, one value per g: the formula is checked per g
    m = _write(a1, ab, str(tmp_path/'mix'), source='solar+thermal', solar_zenith_angle=40.0, solar_azimuth_angle=30.0,
               surface_temperature=301.5)
    text = open(m.fnames_inp[0][0]).read()
    src = text[text.index('&mcarSrc_nml_job'):]
    src = src[:src.index('/')]
    assert [l.split('=')[0].strip() for l in src.splitlines()[1:]] == \
        ['Src_mtype', 'Src_dwlen', 'Src_wlen', 'Src_fsol', 'Src_mphi', 'Src_flx', 'Src_qmax', 'Src_the', 'Src_phi']
    solar = ab.coef['solar']['data']
    for ig in range(m.Ng):
        nml = mca.mca_inp_read(m.fnames_inp[0][ig])
        assert nml['Src_mtype'] == 2 and abs(nml['Src_wlen'] - 3.75) < 1e-12 and nml['Src_flx'] == 1.0
        want = 1000.0*cal_sol_fac(gin.DATE)*solar[ig]
        assert want > 0.0 and abs(nml['Src_fsol']/want - 1.0) < 1.0e-5, (ig, nml['Src_fsol'], want)     # ('%g'-style text: six digits)
        assert abs(nml['Src_the'] - 140.0) < 1e-9 and abs(nml['Src_phi'] - 240.0) < 1e-9
        t = np.atleast_1d(nml['Atm_tmp1d'])
        assert t.size == 17 and abs(t[0] - 301.5) < 1e-9 and np.allclose(t[1:], atm.lev['temperature']['data'][1:], rtol=1e-5)
        _check_supported(nml)
        assert thermal_heating(nml)                                # several ranks take every mixed job one by one
    # a heating-rate target carries the net rate
    mh = mca.mcarats_ng(atm_1ds=[a1], Ng=4, target='heating rate', surface_albedo=0.03, fdir=str(tmp_path/'mixh'), Nrun=1, photons=1e4,
                        weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, source='solar+thermal')
    assert mca.mca_inp_read(mh.fnames_inp[0][0])['Flx_mhrt'] == 2


def test_solar_and_thermal_job_files_carry_no_src_fsol(tmp_path):
    atm, ab, a1 = _objects(tmp_path, WVL)
    for source in ('solar', 'thermal'):
        m = _write(a1, ab, str(tmp_path/source), source=source)
        for f in sum(m.fnames_inp, []):
            assert 'Src_fsol' not in open(f).read(), (source, f)
    with pytest.raises(OSError):
        _write(a1, ab, str(tmp_path/'x'), source='thermal+solar')


def test_round_trip_through_mca_inp_read_and_scene(tmp_path):
    atm, ab, a1 = _objects(tmp_path, WVL)
    m = _write(a1, ab, str(tmp_path/'mix'), source='solar+thermal', solar_zenith_angle=40.0)
    for ig in range(m.Ng):
        nml = mca.mca_inp_read(m.fnames_inp[0][ig])
        s = Scene.from_nml(nml, str(tmp_path/'mix'))
        assert s.src_mtype == 2 and abs(s.src_wlen - 3.75) < 1e-12 and s.tmp1d.size == s.nz + 1
        assert s.src_fsol == float(nml['Src_fsol']) and abs(s.src_the - 140.0) < 1e-9 and abs(s.mu0 - np.cos(np.deg2rad(40.0))) < 1e-9
        assert s.target == TARGET_FLUX
    nml = dict(nml, Flx_mhrt=2)
    assert Scene.from_nml(nml, str(tmp_path/'mix')).target == TARGET_FLUX | TARGET_HEAT
    del nml['Src_fsol']
    with pytest.raises(OSError) as err:
        Scene.from_nml(nml, str(tmp_path/'mix'))
    assert 'Src_mtype=2' in str(err.value) and 'Src_fsol' in str(err.value)


def test_scene_validates_src_fsol():
    nz = 4
    kw = dict(zgrd=np.arange(nz+1)*1000.0, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=np.full(nz, 1e-4),
              src_mtype=2, src_wlen=3.75, tmp1d=np.linspace(290.0, 230.0, nz+1))
    assert Scene(src_fsol=0.0, **kw).src_fsol == 0.0 and Scene(src_fsol=10, **kw).src_fsol == 10.0
    for bad in (None, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError) as err:
            Scene(src_fsol=bad, **kw)
        assert 'Src_fsol' in str(err.value)
    # the thermal source's own demands hold for the mixed one
    with pytest.raises(ValueError):
        Scene(src_fsol=1.0, **dict(kw, src_wlen=None))
    with pytest.raises(ValueError):
        Scene(src_fsol=1.0, **dict(kw, tmp1d=np.linspace(290.0, 230.0, nz)))


@pytest.mark.parametrize('case, kw, words', [
    ('no Src_fsol', dict(Src_fsol=None), 'Src_mtype=2'),
    ('negative Src_fsol', dict(Src_fsol=-1.0), 'Src_fsol'),
    ('all-sky camera', dict(Rad_mrkind=1), 'all-sky'),
    ('brdf surface', dict(Sfc_mtype=4), 'Lambertian'),
    ('heating rate', dict(Wld_mtarget=1, Flx_mhrt=1), 'heating rate'),
    ('no Src_wlen', dict(Src_wlen=None), 'Src_wlen'),
    ('layer temperatures', dict(Atm_tmp1d=np.linspace(290.0, 230.0, 4)), 'ambiguous'),
])
def test_mca_exe_refuses_what_the_mixed_source_does_not_do(case, kw, words):
    base = dict(Src_mtype=2, Src_wlen=3.75, Src_fsol=10.0, Src_the=140.0)
    _check_supported(_thermal_nml(**base))
    _check_supported(_thermal_nml(**dict(base, Src_fsol=0.0)))
    _check_supported(_thermal_nml(**dict(base, Wld_mtarget=1, Flx_mhrt=2)))
    with pytest.raises(OSError) as err:
        _check_supported(_thermal_nml(**dict(base, **kw)))
    assert words in str(err.value), (case, str(err.value))
    if case == 'no Src_fsol':
        assert 'needs <Src_fsol>' in str(err.value) and 'solar+thermal' in str(err.value)
    with pytest.raises(OSError) as err:                               # the local source stays refused
        _check_supported(_thermal_nml(Src_mtype=0))
    assert 'Src_mtype=0' in str(err.value)


class _MixFiles(_Files):
    def __init__(self, *a):
        super().__init__(*a)
        self.source, self.date = 'solar+thermal', gin.DATE


def test_mca_out_ng_combines_mixed_outputs(tmp_path):
    nx, ny, nz, Ng, Nrun, wl = 5, 4, 3, 4, 3, 3.75
    rng = np.random.default_rng(5)
    ab = abs_synth(WVL, atm_synth(np.arange(nz+1)*1.0), Ng=Ng)
    w = ab.coef['weight']['data']
    m = _MixFiles(str(tmp_path), Nrun, Ng, 'radiance', wl)
    rad = {}
    for ir in range(Nrun):
        for ig in range(Ng):
            x = (planck(wl, rng.uniform(270.0, 320.0, (nx, ny, 1, 1)))).astype(np.float32)
            rad[ir, ig] = x
            mca_out_write(m.fnames_out[ir][ig], [('rad', 'radiance', x)])
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
    for ir in range(Nrun):
        want = np.zeros((nx, ny), dtype=np.float32)
        for ig in range(Ng):
            want += rad[ir, ig][:, :, 0, 0]*np.float32(w[ig]*1.0e-3)        # the thermal route's float32 factors: no slit function
        assert np.array_equal(out['rad']['data'][..., ir], want)
    assert np.allclose(planck(wl, out['bt']['data']), out['rad']['data']*1.0e3, rtol=2e-6)
    # toa as in the solar route
    toa = np.sum(cal_sol_fac(gin.DATE)*ab.coef['solar']['data']*w)
    assert toa > 0.0 and out['toa']['data'] == toa
    th = _Files(str(tmp_path), Nrun, Ng, 'radiance', wl)
    same = mca.mca_out_ng(mca_obj=th, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
    assert np.array_equal(same['rad']['data'], out['rad']['data']) and same['toa']['data'] == 0.0
    mean = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert np.allclose(brightness_temperature(wl, mean['rad']['data']*1.0e3), mean['bt']['data'], rtol=1e-6)
    assert 'sunlight' in mean['bt']['name']
