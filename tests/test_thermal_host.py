"""
Thermal source (Src_mtype = 3) without a GPU: Planck's law and its inverse, the job files mcarats_ng writes for it (and that a solar
job from the same objects is unchanged), mca_exe's refusals, and mca_out_ng's g-combination of thermal outputs.
"""

import contextlib
import io
import os

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd.rtm.mca.mca_exe import _check_supported
from er3t_amd.rtm.mca.mca_out import mca_out_write
from er3t_amd.synth import atm_synth, abs_synth
from er3t_amd.thermal import planck, brightness_temperature
from tests.golden import inputs as gin


def test_planck_values_and_inverse():
    for wl, T, want in ((10.0, 300.0, 9.92403), (11.0, 288.0, 7.96577), (4.0, 250.0, 0.0656295)):
        assert abs(planck(wl, T)/want - 1.0) < 1.0e-5, (wl, T, planck(wl, T))
    T = np.linspace(180.0, 330.0, 31)
    for wl in (4.0, 8.5, 11.0, 12.0, 15.0):
        assert np.allclose(brightness_temperature(wl, planck(wl, T)), T, rtol=1.0e-6, atol=0.0)


def _objects(tmp_path, wvl):
    atm = atm_synth(np.arange(17)*1.0)                  # 16 layers of 1 km
    ab = abs_synth(wvl, atm, Ng=4)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    return atm, ab, a1


def _write(a1, ab, fdir, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=4, target='flux', surface_albedo=0.03, fdir=fdir, Nrun=1, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


def test_thermal_job_files(tmp_path):
    atm, ab, a1 = _objects(tmp_path, 11000.0)
    m = _write(a1, ab, str(tmp_path/'th'), source='thermal', surface_temperature=301.5)
    nml = mca.mca_inp_read(m.fnames_inp[0][0])
    assert nml['Src_mtype'] == 3 and abs(nml['Src_wlen'] - 11.0) < 1e-12
    t = np.atleast_1d(nml['Atm_tmp1d'])
    assert t.size == 17 and abs(t[0] - 301.5) < 1e-9
    assert np.allclose(t[1:], atm.lev['temperature']['data'][1:], rtol=1e-5)
    m2 = _write(a1, ab, str(tmp_path/'th2'), source='thermal', wavelength=12000.0)
    nml2 = mca.mca_inp_read(m2.fnames_inp[0][0])
    assert abs(nml2['Src_wlen'] - 12.0) < 1e-12 and abs(np.atleast_1d(nml2['Atm_tmp1d'])[0] - atm.lev['temperature']['data'][0]) < 1e-6
    _check_supported(nml)


def test_solar_job_files_do_not_change(tmp_path):
    """a solar job from the same objects, with and without the new keywords, writes what the code before the thermal source wrote:
    no Src_wlen, Src_mtype 1 and the nz LAYER temperatures"""
    atm, ab, a1 = _objects(tmp_path, 650.0)
    m0 = _write(a1, ab, str(tmp_path/'a'))
    m1 = _write(a1, ab, str(tmp_path/'b'), source='solar', wavelength=None, surface_temperature=None)
    t0 = open(m0.fnames_inp[0][0]).read()
    for a, b in zip(sum(m0.fnames_inp, []), sum(m1.fnames_inp, [])):
        ta, tb = open(a).read(), open(b).read()
        strip = lambda s: '\n'.join(l for l in s.splitlines() if 'Wld_jseed' not in l)
        assert strip(ta) == strip(tb)
    assert 'Src_wlen' not in t0
    nml = mca.mca_inp_read(m0.fnames_inp[0][0])
    assert nml['Src_mtype'] == 1 and np.atleast_1d(nml['Atm_tmp1d']).size == 16
    # the layout of the solar text itself: the source group as it was
    src = t0[t0.index('&mcarSrc_nml_job'):]
    src = src[:src.index('/')]
    assert [l.split('=')[0].strip() for l in src.splitlines()[1:]] == ['Src_mtype', 'Src_dwlen', 'Src_mphi', 'Src_flx', 'Src_qmax', 'Src_the', 'Src_phi']


def _thermal_nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 2, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3, 'Src_wlen': 11.0,
           'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1}
    nml.update(kw)
    return {k: v for k, v in nml.items() if v is not None}


@pytest.mark.parametrize('case, kw, words', [
    ('local', dict(Src_mtype=0), 'Src_mtype=0'),
    ('solar+thermal', dict(Src_mtype=2), 'Src_mtype=2'),
    ('brdf surface', dict(Sfc_mtype=4), 'Lambertian'),
    ('all-sky camera', dict(Rad_mrkind=1), 'all-sky'),
    ('heating rate', dict(Wld_mtarget=1, Flx_mhrt=1), 'heating rate'),
    ('no Src_wlen', dict(Src_wlen=None), 'Src_wlen'),
    ('layer temperatures', dict(Atm_tmp1d=np.linspace(290.0, 230.0, 4)), 'ambiguous'),
])
def test_mca_exe_refuses_what_the_thermal_source_does_not_do(case, kw, words):
    _check_supported(_thermal_nml())
    with pytest.raises(OSError) as err:
        _check_supported(_thermal_nml(**kw))
    assert words in str(err.value), (case, str(err.value))


def test_mca_exe_refuses_a_brdf_2d_surface_for_thermal_jobs(tmp_path):
    nxb = nyb = 3
    blocks = np.zeros((7, nyb, nxb), dtype='<f4'); blocks[1] = 1.0
    blocks.tofile(str(tmp_path/'sfc.bin'))
    nml = _thermal_nml(Sfc_inpfile='sfc.bin', Sfc_nxb=nxb, Sfc_nyb=nyb)
    _check_supported(nml, str(tmp_path))
    blocks[1, 1, 2] = 4.0
    blocks.tofile(str(tmp_path/'sfc.bin'))
    with pytest.raises(OSError) as err:
        _check_supported(nml, str(tmp_path))
    assert 'Lambertian' in str(err.value)


class _Files:
    """what mca_out_ng reads of a thermal mcarats_ng object"""
    def __init__(self, fdir, Nrun, Ng, target, wlen_um):
        self.Nrun, self.Ng, self.target, self.source, self.wlen_um = Nrun, Ng, target, 'thermal', wlen_um
        self.fnames_out = [['%s/r%02d.g%03d.out.bin' % (fdir, ir, ig) for ig in range(Ng)] for ir in range(Nrun)]
        self.photons = np.full(Nrun*Ng, 1000)
        self.Nview = 1
        self.fused = None


def test_mca_out_ng_combines_thermal_outputs(tmp_path):
    nx, ny, nz, Ng, Nrun, wl = 5, 4, 3, 4, 3, 11.0
    rng = np.random.default_rng(3)
    ab = abs_synth(11000.0, atm_synth(np.arange(nz+1)*1.0), Ng=Ng)
    w = ab.coef['weight']['data']
    m = _Files(str(tmp_path), Nrun, Ng, 'radiance', wl)
    rad = {}
    for ir in range(Nrun):
        for ig in range(Ng):
            x = (planck(wl, rng.uniform(240.0, 300.0, (nx, ny, 1, 1)))).astype(np.float32)
            rad[ir, ig] = x
            mca_out_write(m.fnames_out[ir][ig], [('rad', 'radiance', x)])
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
    for ir in range(Nrun):
        want = np.zeros((nx, ny), dtype=np.float32)
        for ig in range(Ng):
            want += rad[ir, ig][:, :, 0, 0]*np.float32(w[ig]*1.0e-3)
        assert np.array_equal(out['rad']['data'][..., ir], want)
    assert out['rad']['units'] == 'W/m^2/nm/sr'
    assert np.allclose(planck(wl, out['bt']['data']), out['rad']['data']*1.0e3, rtol=2e-6)
    mean = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert np.allclose(brightness_temperature(wl, mean['rad']['data']*1.0e3), mean['bt']['data'], rtol=1e-6)
    mf = _Files(str(tmp_path), Nrun, Ng, 'flux', wl)
    for ir in range(Nrun):
        for ig in range(Ng):
            f = rng.uniform(1.0, 30.0, (nx, ny, nz+1, 1)).astype(np.float32)
            mca_out_write(mf.fnames_out[ir][ig], [('f_down_direct', 'x', np.zeros_like(f)), ('f_down', 'x', f), ('f_up', 'x', 2*f)])
    fl = mca.mca_out_ng(mca_obj=mf, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert np.all(fl['f_down_direct']['data'] == 0.0) and np.allclose(fl['f_up']['data'], 2*fl['f_down']['data'], rtol=1e-6)
