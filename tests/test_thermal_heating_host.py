"""
Net heating rates of thermal jobs (Flx_mhrt = 2, a value of this project) without a GPU: the job files mcarats_ng writes for
source='thermal', target='heating rate' (and that a solar heating job's files are what they were), what Scene.from_nml and mca_exe
make of the key, the refusals, the C-ABI's table, and mca_out_ng's g-combination of thermal `hrt` files.
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
from er3t_amd.rtm.mca.mca_out import mca_out_write
from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_HEAT
from er3t_amd.synth import atm_synth, abs_synth
from tests.golden import inputs as gin

HERE = os.path.dirname(os.path.abspath(__file__))


def _objects(wvl):
    atm = atm_synth(np.arange(17)*1.0)                  # 16 layers of 1 km
    ab = abs_synth(wvl, atm, Ng=4)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    return atm, ab, a1


def _write(a1, ab, fdir, target='heating rate', **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=4, target=target, surface_albedo=0.03, fdir=fdir, Nrun=2, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


def _strip(text):
    return '\n'.join(l for l in text.splitlines() if 'Wld_jseed' not in l)


def _group(text, name):
    """the lines of one namelist group of a job file"""
    body = text[text.index('&'+name):]
    return body[:body.index('\n/')].splitlines()


def test_thermal_heating_job_files_carry_the_new_value(tmp_path):
    _, ab, a1 = _objects(11000.0)
    mc = _write(a1, ab, str(tmp_path/'coll'), source='thermal')
    mp = _write(a1, ab, str(tmp_path/'path'), source='thermal', heating_estimator='path')
    for fc, fp in zip(sum(mc.fnames_inp, []), sum(mp.fnames_inp, [])):
        nc, npth = mca.mca_inp_read(fc), mca.mca_inp_read(fp)
        assert nc['Src_mtype'] == 3 and nc['Wld_mtarget'] == 1 and nc['Flx_mflx'] == 3 and nc['Flx_mhrt'] == 2
        assert 'Flx_mhest' not in nc and 'Flx_mhest' not in open(fc).read()
        assert npth['Flx_mhrt'] == 2 and npth['Flx_mhest'] == 1
        assert thermal_heating(nc) and thermal_heating(npth)
    # a thermal FLUX job is what it was: no heating flag
    mf = _write(a1, ab, str(tmp_path/'flux'), target='flux', source='thermal')
    nf = mca.mca_inp_read(mf.fnames_inp[0][0])
    assert nf['Flx_mhrt'] == 0 and not thermal_heating(nf)


def test_scene_from_nml_maps_the_value_to_the_heating_target(tmp_path):
    _, ab, a1 = _objects(11000.0)
    for est, want in (('collision', 0), ('path', 1)):
        m = _write(a1, ab, str(tmp_path/est), source='thermal', heating_estimator=est)
        fname = m.fnames_inp[1][2]
        nml = mca.mca_inp_read(fname)
        _check_supported(nml, os.path.dirname(fname))
        sc = Scene.from_nml(nml, os.path.dirname(fname), solver=0)
        assert sc.src_mtype == 3 and sc.target == TARGET_FLUX | TARGET_HEAT and sc.heat_estimator == want
    # Flx_mhrt = 0 in a thermal job: fluxes alone
    nml0 = dict(nml, Flx_mhrt=0)
    assert Scene.from_nml(nml0, os.path.dirname(fname), solver=0).target == TARGET_FLUX


def test_a_solar_job_refuses_the_new_value_and_a_thermal_job_still_refuses_the_old_one(tmp_path):
    _, ab, a1 = _objects(650.0)
    m = _write(a1, ab, str(tmp_path/'solar'))
    fname = m.fnames_inp[0][0]
    nml = mca.mca_inp_read(fname)
    assert nml['Flx_mhrt'] == 1 and not thermal_heating(nml)
    assert Scene.from_nml(nml, os.path.dirname(fname), solver=0).target == TARGET_FLUX | TARGET_HEAT
    with pytest.raises(OSError) as err:
        Scene.from_nml(dict(nml, Flx_mhrt=2), os.path.dirname(fname), solver=0)
    assert 'Flx_mhrt=2' in str(err.value) and 'thermal' in str(err.value)
    nz = 4
    th = {'Wld_mtarget': 1, 'Flx_mflx': 3, 'Flx_mhrt': 2, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3,
          'Src_wlen': 11.0, 'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1}
    _check_supported(th)
    with pytest.raises(OSError) as err:
        _check_supported(dict(th, Flx_mhrt=1))
    assert 'heating rate' in str(err.value) and 'Flx_mhrt=2' in str(err.value)


def test_solar_heating_job_files_are_byte_for_byte_what_they_were(tmp_path):
    """with and without the thermal keywords a solar heating job writes the same text, and its Flx group is the golden namelist's
    (tests/golden/nml_hr_1d_g00.txt, written by the reference)"""
    _, ab, a1 = _objects(650.0)
    m0 = _write(a1, ab, str(tmp_path/'a'))
    m1 = _write(a1, ab, str(tmp_path/'b'), source='solar', wavelength=None, surface_temperature=None, heating_estimator='collision')
    for a, b in zip(sum(m0.fnames_inp, []), sum(m1.fnames_inp, [])):
        assert _strip(open(a).read()) == _strip(open(b).read())
    golden = open(os.path.join(HERE, 'golden', 'nml_hr_1d_g00.txt')).read()
    text = open(m0.fnames_inp[0][0]).read()
    assert _group(text, 'mcarFlx_nml_init') == _group(golden, 'mcarFlx_nml_init') == ['&mcarFlx_nml_init', ' Flx_mflx        = 3', ' Flx_mhrt        = 1']
    noseed = lambda lines: [l for l in lines if 'Wld_jseed' not in l]
    assert noseed(_group(text, 'mcarWld_nml_init')) == noseed(_group(golden, 'mcarWld_nml_init'))
    assert 'Src_wlen' not in text and mca.mca_inp_read(m0.fnames_inp[0][0])['Src_mtype'] == 1


def test_the_header_declares_the_emission_getter_and_the_table_lists_it():
    header = open(os.path.join(HERE, '..', 'include', 'mi3d.h')).read()
    assert 'int mi3d_get_emission(mi3d_solver *h, float *out);' in header
    sig = {n: (r, a) for n, r, a in solver_mod._SIGNATURES}
    assert 'mi3d_get_emission' in sig
    import ctypes as C
    assert sig['mi3d_get_emission'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float)])
    assert callable(getattr(solver_mod.Mi3dSolver, 'emission'))
    # the contract is written down where the issue wants it
    assert re.search(r'NET', header) and 'Flx_mhrt = 2' in header


class _Files:
    """what mca_out_ng reads of a thermal mcarats_ng object"""
    def __init__(self, fdir, Nrun, Ng, target, source='thermal', heating_estimator='collision'):
        self.Nrun, self.Ng, self.target, self.source, self.wlen_um = Nrun, Ng, target, source, 11.0
        self.heating_estimator = heating_estimator
        self.fnames_out = [['%s/r%02d.g%03d.out.bin' % (fdir, ir, ig) for ig in range(Ng)] for ir in range(Nrun)]
        self.photons = np.full(Nrun*Ng, 1000)
        self.Nview = 1
        self.fused = None
        self.date = gin.DATE


@pytest.mark.parametrize('est', ['collision', 'path'])
def test_mca_out_ng_combines_thermal_hrt_files_with_the_thermal_factors(tmp_path, est):
    nx, ny, nz, Ng, Nrun = 5, 4, 3, 4, 3
    rng = np.random.default_rng(11)
    ab = abs_synth(11000.0, atm_synth(np.arange(nz+1)*1.0), Ng=Ng)
    w = ab.coef['weight']['data']
    m = _Files(str(tmp_path), Nrun, Ng, 'heating rate', heating_estimator=est)
    hrt = {}
    for ir in range(Nrun):
        for ig in range(Ng):
            f = rng.uniform(1.0, 30.0, (nx, ny, nz+1, 1)).astype(np.float32)
            h = rng.uniform(-3.0e-3, 1.0e-3, (nx, ny, nz, 1)).astype(np.float32)       # mostly cooling
            hrt[ir, ig] = h
            mca_out_write(m.fnames_out[ir][ig], [('fdnd', 'x', np.zeros_like(f)), ('fdn', 'x', f), ('fup', 'x', 2*f), ('hrt', 'net', h)])
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
    for ir in range(Nrun):
        want = np.zeros((nx, ny, nz), dtype=np.float32)
        for ig in range(Ng):
            want += hrt[ir, ig][..., 0]*np.float32(w[ig]*1.0e-3)                      # sum_g weight x / 1000: no solar factor, no slit
        assert np.array_equal(out['heating_rate']['data'][..., ir], want)
    assert out['heating_rate']['name'].startswith('Net absorbed power per unit volume') and out['heating_rate']['units'] == 'W/m^3/nm'
    assert ('path-length' in out['heating_rate']['name']) == (est == 'path')
    mean = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert np.allclose(mean['heating_rate']['data'], out['heating_rate']['data'].mean(axis=-1), rtol=1e-6)
    assert np.allclose(mean['heating_rate_std']['data'], out['heating_rate']['data'].std(axis=-1), rtol=1e-5)
    assert mean['heating_rate']['name'].startswith('Net absorbed power per unit volume (mean')
    assert mean['heating_rate']['data'].shape == (nx, ny, nz) and np.mean(mean['heating_rate']['data']) < 0.0
    # a solar object's names are what they were
    ms = _Files(str(tmp_path), Nrun, Ng, 'heating rate', source='solar')
    ab_s = abs_synth(650.0, atm_synth(np.arange(nz+1)*1.0), Ng=Ng)
    sol = mca.mca_out_ng(mca_obj=ms, abs_obj=ab_s, mode='mean', squeeze=True, quiet=True).data
    assert sol['heating_rate']['name'] == 'Absorbed power per unit volume (mean)'


def test_the_ctl_of_a_thermal_job_says_net(tmp_path):
    from er3t_amd.rtm.mca.mca_exe import JobRunner
    r = JobRunner.__new__(JobRunner)                     # (write needs the rank alone: no GPU)
    r.rank = 0
    flux = np.zeros((3, 4, 2, 3), dtype=np.float32); heat = np.full((3, 2, 3), -1.5e-3, dtype=np.float32)
    r.write(str(tmp_path/'t.out.bin'), {'flux': flux, 'heat': heat, 'heat_net': True})
    r.write(str(tmp_path/'s.out.bin'), {'flux': flux, 'heat': heat, 'heat_net': False})
    t, s = open(str(tmp_path/'t.out.bin.ctl')).read(), open(str(tmp_path/'s.out.bin.ctl')).read()
    assert 'net (absorbed - emitted)' in t and 'net' not in s
    assert 'absorbed power per unit volume (heating rate x air density x c_p)' in s
    raw = mca.mca_out_raw(str(tmp_path/'t.out.bin'))
    assert len(raw.data) == 4 and np.all(raw.data[3]['data'] == np.float32(-1.5e-3))
