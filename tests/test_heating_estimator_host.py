"""
The heating-rate tally's second estimator (path length, Flx_mhest = 1) without a GPU: the keyword of mcarats_ng and the job files it
writes (and that every job without it is written byte for byte as before), what mca_exe makes of such a file, the refusals, and the
C-ABI's table.
"""

import contextlib
import io
import os

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca.mca_exe import _check_supported
from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_HEAT
from er3t_amd.synth import atm_synth, abs_synth
from tests.golden import inputs as gin
from tests.util import slab_scene


def _objects(wvl=650.0):
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


def test_path_keyword_writes_flx_mhest_into_every_job_file_and_nothing_else_changes(tmp_path):
    _, ab, a1 = _objects()
    m0 = _write(a1, ab, str(tmp_path/'plain'))
    md = _write(a1, ab, str(tmp_path/'default'), heating_estimator='collision')
    mp = _write(a1, ab, str(tmp_path/'path'), heating_estimator='path')
    assert m0.heating_estimator == 'collision' and mp.heating_estimator == 'path'
    for f0, fd, fp in zip(sum(m0.fnames_inp, []), sum(md.fnames_inp, []), sum(mp.fnames_inp, [])):
        t0, td, tp = open(f0).read(), open(fd).read(), open(fp).read()
        assert 'Flx_mhest' not in t0
        assert _strip(t0) == _strip(td)                       # the default: byte for byte what is written without the keyword
        nml = mca.mca_inp_read(fp)
        assert nml['Flx_mhest'] == 1 and nml['Flx_mhrt'] == 1 and nml['Flx_mflx'] == 3
        assert 'Flx_mhest' not in mca.mca_inp_read(f0)
        # ... and the path job's text is the default's plus that one line, in the Flx group behind Flx_mhrt
        lines = _strip(tp).splitlines()
        extra = [l for l in lines if 'Flx_mhest' in l]
        assert len(extra) == 1 and [l for l in lines if 'Flx_mhest' not in l] == _strip(t0).splitlines()
        assert 'Flx_mhrt' in lines[lines.index(extra[0])-1]
    # a flux job is what it was, too
    f = _write(a1, ab, str(tmp_path/'flux'), target='flux')
    assert 'Flx_mhest' not in open(f.fnames_inp[0][0]).read()


@pytest.mark.parametrize('kw, words', [
    (dict(heating_estimator='tracklength'), 'heating_estimator'),
    (dict(heating_estimator='path', target='flux'), 'heating rate'),
    (dict(heating_estimator='path', target='radiance'), 'heating rate'),
])
def test_a_bad_word_and_a_wrong_target_are_refused(tmp_path, kw, words):
    _, ab, a1 = _objects()
    with pytest.raises(OSError) as err:
        _write(a1, ab, str(tmp_path/'x'), **kw)
    assert str(err.value).startswith('Error [mcarats_ng]:') and words in str(err.value), str(err.value)


def test_mca_exe_maps_the_key_to_the_scene(tmp_path):
    _, ab, a1 = _objects()
    mp = _write(a1, ab, str(tmp_path/'path'), heating_estimator='path')
    m0 = _write(a1, ab, str(tmp_path/'plain'))
    for m, want in ((mp, 1), (m0, 0)):
        fname = m.fnames_inp[1][2]
        nml = mca.mca_inp_read(fname)
        _check_supported(nml, os.path.dirname(fname))
        sc = Scene.from_nml(nml, os.path.dirname(fname), solver=0)
        assert sc.heat_estimator == want and sc.target == TARGET_FLUX | TARGET_HEAT
    nml = dict(mca.mca_inp_read(mp.fnames_inp[0][0]), Flx_mhest=2)
    with pytest.raises(OSError, match='Flx_mhest'):
        Scene.from_nml(nml, str(tmp_path/'path'), solver=0)


def test_a_thermal_job_still_refuses_heating_rates_whichever_estimator():
    nz = 4
    nml = {'Wld_mtarget': 1, 'Flx_mflx': 3, 'Flx_mhrt': 1, 'Flx_mhest': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3,
           'Src_wlen': 11.0, 'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1}
    with pytest.raises(OSError) as err:
        _check_supported(nml)
    assert 'heating rate' in str(err.value)


def test_scene_default_and_the_abi_table():
    assert Scene(zgrd=[0.0, 1000.0], ext1d=[[1e-4]], omg1d=[[1.0]], apf1d=[[0.5]], abs1d=[0.0]).heat_estimator == 0
    assert slab_scene().heat_estimator == 0
    names = [n for n, _, _ in solver_mod._SIGNATURES]
    assert 'mi3d_set_heating_estimator' in names
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'mi3d.h')).read()
    assert 'int mi3d_set_heating_estimator(mi3d_solver *h, int estimator);' in header
