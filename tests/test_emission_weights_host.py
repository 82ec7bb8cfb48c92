"""
Per-cell emission weights of the backward route without a GPU: the namelist key Rad_mwgt through mcarats_ng, mca_exe's
checks and Scene.from_nml; that every other job file stays byte for byte what it was; the float64 reference of the GPU tests
(tests/emission_weights_ref.py) against the line integral of tests/thermal_camera_ref.py; the g / run reduction of mca_out; dplanck_dT.
"""

import dataclasses
import os
import re
import types

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca import mca_out
from er3t_amd.rtm.mca.mca_exe import _check_supported, weights_fname, flatten_weights
from er3t_amd.scene import Scene, TARGET_RADIANCE
from er3t_amd.thermal import planck, dplanck_dT
from tests import emission_weights_ref as wref
from tests import thermal_camera_ref as ref
from tests.test_backward_host import _nml, _objects, _write, _text, SENSORS
from tests.test_gpu_backward import absorbing_scene, cameras


# ---- job files -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', sorted(SENSORS))
def test_job_files_carry_the_key_only_when_asked(tmp_path, kind):
    atm, ab, a1 = _objects(11000.0)
    fwd = _write(a1, ab, str(tmp_path/'fwd'), source='thermal', **SENSORS[kind])
    bwd = _write(a1, ab, str(tmp_path/'bwd'), source='thermal', camera_method='backward', **SENSORS[kind])
    off = _write(a1, ab, str(tmp_path/'off'), source='thermal', camera_method='backward', emission_weights=False, **SENSORS[kind])
    wgt = _write(a1, ab, str(tmp_path/'wgt'), source='thermal', camera_method='backward', emission_weights=True, **SENSORS[kind])
    tf, tb, to, tw = _text(fwd), _text(bwd), _text(off), _text(wgt)
    assert tb == to and not any('Rad_mwgt' in l for l in tf+tb)              # forward jobs and backward jobs without weights: what they were
    assert tf == _text(_write(a1, ab, str(tmp_path/'fwd2'), source='thermal', emission_weights=False, **SENSORS[kind]))
    assert sum('Rad_mwgt' in l for l in tw) == 1 and [l for l in tw if 'Rad_mwgt' not in l] == tb
    rad = tw[tw.index('&mcarRad_nml_job'):]
    assert any('Rad_mwgt' in l for l in rad[1:rad.index('/')])
    nml = mca.mca_inp_read(wgt.fnames_inp[0][0])
    assert nml['Rad_mwgt'] == 1 and nml['Rad_mbwd'] == 1
    _check_supported(nml)
    sc = Scene.from_nml(nml, str(tmp_path), solver=0)
    assert sc.cam_weights == 1 and sc.cam_method == 1
    assert Scene.from_nml(mca.mca_inp_read(bwd.fnames_inp[0][0]), str(tmp_path), solver=0).cam_weights == 0
    assert wgt.emission_weights is True and bwd.emission_weights is False


def test_refusals(tmp_path):
    atm, ab, a1 = _objects(11000.0)
    with pytest.raises(OSError) as err:
        _write(a1, ab, str(tmp_path/'bad'), source='thermal', camera_method='forward', emission_weights=True, **SENSORS['irradiance'])
    assert 'emission_weights' in str(err.value) and 'backward' in str(err.value)
    with pytest.raises(OSError):
        _write(a1, ab, str(tmp_path/'bad'), source='thermal', emission_weights=True, **SENSORS['irradiance'])
    _check_supported(_nml(Rad_mwgt=1)); _check_supported(_nml(Rad_mwgt=0)); _check_supported(_nml(Rad_mbwd=0, Rad_nimg=1, Rad_mwgt=0))
    for kw in (dict(Rad_mbwd=0, Rad_nimg=1, Rad_mwgt=1), dict(Rad_mbwd=None, Rad_nimg=2, Rad_mwgt=1), dict(Rad_mwgt=2), dict(Rad_mwgt=-1), dict(Rad_mwgt=0.5)):
        with pytest.raises(OSError) as err:
            _check_supported(_nml(**kw))
        assert 'Rad_mwgt' in str(err.value), kw
        with pytest.raises(OSError) as err:
            Scene.from_nml(_nml(**kw), '.', solver=0)
        assert 'Rad_mwgt' in str(err.value), kw
    base = dict(zgrd=np.arange(5)*1000.0, ext1d=np.zeros(4), omg1d=np.ones(4), apf1d=np.full(4, -1.0), abs1d=np.full(4, 1e-4),
                target=TARGET_RADIANCE, view_the=[0.0], view_phi=[0.0], view_zloc=[10.0], src_mtype=3, src_wlen=11.0, tmp1d=np.linspace(290.0, 230.0, 5))
    assert Scene(rad_kind=1, cam_method=1, cam_weights=1, **base).cam_weights == 1 and Scene(rad_kind=1, cam_method=1, **base).cam_weights == 0
    for kw in (dict(rad_kind=1, cam_method=0, cam_weights=1), dict(rad_kind=2, cam_weights=1), dict(rad_kind=1, cam_method=1, cam_weights=2)):
        with pytest.raises(ValueError) as err:
            Scene(**dict(base, **kw))
        assert 'Rad_mwgt' in str(err.value), kw


def test_header_declares_the_new_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(root, 'include', 'mi3d.h')).read(), flags=re.S)
    sig = dict((n, a) for n, _, a in solver_mod._SIGNATURES)
    for name in ('mi3d_set_emission_weights', 'mi3d_bind_weights_buffer', 'mi3d_get_emission_weights'):
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert m and len(m.group(1).split(',')) == len(sig[name]), name


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('albedo', [0.0, 0.1])
def test_reference_weights_give_the_line_integral(albedo):
    """sum_c K_c B_c is the radiance of tests/thermal_camera_ref.march (emission of the line and of the surface cell it ends on) to 1e-12"""
    base = absorbing_scene(albedo)
    rng = np.random.default_rng(7)
    psfc = np.zeros((5, 2, 2), dtype=np.float32); psfc[0] = albedo
    for sc in (base, dataclasses.replace(base, jsfc=np.ones((2, 2)), psfc=psfc, tmps2d=np.zeros((2, 2), dtype=np.float32))):
        sc = cameras(sc, [150.0], [500.0], xpos=0.45, ypos=0.3, mpmap=2, mrproj=0)
        d = rng.normal(size=(300, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        for org in ([900.0, 600.0, 500.0], [700.0, 1300.0, 1100.0], [100.0, 100.0, 50.0]):
            K = wref.line_weights(sc, np.array(org), d)
            B = wref.planck_cells(sc)
            want = ref.march(sc, np.array(org)[None], d)
            assert K.shape == (300, sc.nx*sc.ny*sc.nz3+sc.nz+(4 if sc.jsfc is not None else 1)) and K.min() >= 0.0
            assert np.all(np.abs(K @ B-want) <= 1.0e-12*want), np.abs(K @ B/want-1.0).max()
            assert np.all(K.sum(axis=1) <= 1.0+1e-12) and K[:, :sc.nx*sc.ny*sc.nz3].sum() > 0.0
            nvox = sc.nx*sc.ny*sc.nz3
            assert np.all(K[:, nvox+sc.iz3l-1:nvox+sc.iz3l-1+sc.nz3] == 0.0)       # layers inside the 3-D region carry nothing


def test_dplanck_dT_is_the_derivative():
    T = np.array([200.0, 250.0, 288.0, 320.0])
    for wl in (3.9, 11.0, 50.0):
        h = 1.0e-3
        num = (planck(wl, T+h)-planck(wl, T-h))/(2.0*h)
        assert np.allclose(dplanck_dT(wl, T), num, rtol=1.0e-8, atol=0.0)
    assert dplanck_dT(11.0, 0.0) == 0.0 and dplanck_dT(11.0, np.array([-5.0]))[0] == 0.0


# ---- the reduction of mca_out ------------------------------------------------------------------------------------------------------------------

def _fake(tmp_path, Nrun, Ng, geom, seed=1):
    """synthetic per-job .wgt.bin files and the objects read_emission_weights asks for"""
    nview, nyr, nxr, nz3, ny, nx, nz, nyb, nxb = geom
    npix, ncell = nview*nyr*nxr, nx*ny*nz3+nz+nyb*nxb
    rng = np.random.default_rng(seed)
    planck_c = rng.uniform(5.0, 9.0, ncell).astype(np.float32)
    inp = str(tmp_path/'job.inp.txt')
    nml = {'Rad_nrad': nview, 'Rad_nyr': nyr, 'Rad_nxr': nxr, 'Atm_nz3': nz3, 'Atm_ny': ny, 'Atm_nx': nx, 'Atm_nz': nz}
    if nyb*nxb > 1:
        nml.update(Sfc_inpfile='sfc.bin', Sfc_nxb=nxb, Sfc_nyb=nyb)
    jobs = rng.uniform(0.0, 1.0, (Nrun, Ng, npix, ncell)).astype(np.float32)
    outs = [[str(tmp_path/('r%02d.g%03d.out.bin' % (ir, ig))) for ig in range(Ng)] for ir in range(Nrun)]
    for ir in range(Nrun):
        for ig in range(Ng):
            with open(weights_fname(outs[ir][ig]), 'wb') as f:
                jobs[ir, ig].astype('<f4').tofile(f); planck_c.astype('<f4').tofile(f)
    weight = rng.uniform(0.1, 0.5, Ng)
    m = types.SimpleNamespace(fnames_inp=[[inp]], fnames_out=outs, Nrun=Nrun, Ng=Ng, source='thermal', fused=None, emission_weights=True)
    ab = types.SimpleNamespace(coef={'weight': {'data': weight}})
    return m, ab, nml, jobs, planck_c, weight


def test_reduction_is_the_numpy_formula_and_keeps_the_identity(tmp_path, monkeypatch):
    geom = (2, 1, 3, 2, 3, 4, 5, 2, 2)
    nview, nyr, nxr, nz3, ny, nx, nz, nyb, nxb = geom
    m, ab, nml, jobs, planck_c, weight = _fake(tmp_path, 3, 4, geom)
    import er3t_amd.rtm.mca.mca_inp as inp_mod
    monkeypatch.setattr(inp_mod, 'mca_inp_read', lambda f: nml)
    fac = np.array([np.float32(w*1.0e-3) for w in weight], dtype=np.float64)
    runs = np.einsum('g,rgpc->rpc', fac, jobs.astype(np.float64))
    mean, std = runs.mean(axis=0), runs.std(axis=0)
    nvox = nx*ny*nz3
    for squeeze in (True, False):
        d = mca_out.read_emission_weights(m, ab, mode='mean', squeeze=squeeze)
        a = mca_out.read_emission_weights(m, ab, mode='all', squeeze=squeeze)
        pix = (nxr, nview) if squeeze else (nxr, nyr, nview)
        assert d['emission_weight']['data'].shape == (nx, ny, nz3)+pix and d['emission_weight_layers']['data'].shape == (nz,)+pix
        assert d['emission_weight_surface']['data'].shape == (nxb, nyb)+pix and a['emission_weight']['data'].shape == (nx, ny, nz3)+pix+(3,)
        assert d['emission_planck']['data'].shape == (nx, ny, nz3) and d['emission_planck_layers']['data'].shape == (nz,)
        assert d['emission_weight']['dims_info'] == ['Nx', 'Ny', 'Nz3']+(['Nxr', 'Nview'] if squeeze else ['Nxr', 'Nyr', 'Nview'])
        for field, stat in (('emission_weight', mean), ('emission_weight_std', std)):
            want = stat.reshape(nview, nyr, nxr, -1)
            v = np.transpose(want[..., :nvox].reshape(nview, nyr, nxr, nz3, ny, nx), (5, 4, 3, 2, 1, 0)).reshape((nx, ny, nz3)+pix)
            l = np.transpose(want[..., nvox:nvox+nz], (3, 2, 1, 0)).reshape((nz,)+pix)
            s = np.transpose(want[..., nvox+nz:].reshape(nview, nyr, nxr, nyb, nxb), (4, 3, 2, 1, 0)).reshape((nxb, nyb)+pix)
            tol = dict(rtol=2.0**-23, atol=0.0) if field == 'emission_weight' else dict(rtol=1.0e-4, atol=1.0e-9)
            assert np.allclose(d[field]['data'], v, **tol) and np.allclose(d[field+'_layers']['data'], l, **tol)
            assert np.allclose(d[field+'_surface']['data'], s, **tol)
        assert np.allclose(a['emission_weight_layers']['data'][..., 1].reshape((nz,)+pix), np.transpose(runs[1].reshape(nview, nyr, nxr, -1)[..., nvox:nvox+nz], (3, 2, 1, 0)).reshape((nz,)+pix), rtol=2.0**-23)
        assert np.array_equal(d['emission_planck_layers']['data'], planck_c[nvox:nvox+nz])
        assert np.array_equal(d['emission_planck']['data'], np.transpose(planck_c[:nvox].reshape(nz3, ny, nx), (2, 1, 0)))
    # rad = sum_c weight_c planck_c survives the reduction: every job's reading is sum_c K B (Src_flx = 1), reduced like rad
    rad_jobs = np.einsum('rgpc,c->rgp', jobs.astype(np.float64), planck_c.astype(np.float64))
    rad = np.einsum('g,rgp->rp', fac, rad_jobs).mean(axis=0)
    d = mca_out.read_emission_weights(m, ab, mode='mean', squeeze=False)
    back = sum((d['emission_weight'+s]['data'].astype(np.float64)*d['emission_planck'+s]['data'].astype(np.float64).reshape(d['emission_planck'+s]['data'].shape+(1, 1, 1)))
               .reshape(-1, nxr, nyr, nview).sum(axis=0) for s in ('', '_layers', '_surface'))
    assert np.allclose(np.transpose(back, (2, 1, 0)).ravel(), rad, rtol=2.0**-22, atol=0.0)


def test_the_reducer_is_fed_job_by_job(tmp_path, monkeypatch):
    """what the reduction holds does not grow with the number of jobs: one job's file is read, added and released before the next is opened"""
    geom = (1, 1, 2, 1, 2, 2, 3, 1, 1)
    import er3t_amd.rtm.mca.mca_inp as inp_mod
    held = {}
    for Nrun, Ng in ((2, 2), (4, 6)):
        m, ab, nml, jobs, planck_c, weight = _fake(tmp_path, Nrun, Ng, geom)
        monkeypatch.setattr(inp_mod, 'mca_inp_read', lambda f, nml=nml: nml)
        events, live = [], [0, 0]
        real_fromfile, real_add = np.fromfile, mca_out.weights_reducer.add

        def fromfile(*a, **k):
            live[0] += 1; live[1] = max(live[1], live[0]); events.append('read')
            return real_fromfile(*a, **k)

        def add(self, ig, weights, planck=None):
            events.append('add')
            real_add(self, ig, weights, planck)
            live[0] -= 1

        monkeypatch.setattr(mca_out.np, 'fromfile', fromfile)
        monkeypatch.setattr(mca_out.weights_reducer, 'add', add)
        mca_out.read_emission_weights(m, ab, mode='mean')
        monkeypatch.setattr(mca_out.np, 'fromfile', real_fromfile)
        monkeypatch.setattr(mca_out.weights_reducer, 'add', real_add)
        assert events == ['read', 'add']*(Nrun*Ng) and live[1] == 1
        red = mca_out.weights_reducer(np.ones(Ng))
        for ir in range(Nrun):
            for ig in range(Ng):
                red.add(ig, jobs[ir, ig], planck_c)
            red.end_run()
        assert red.jobs_fed == Nrun*Ng and red.runs == []
        held[(Nrun, Ng)] = sum(a.nbytes for a in (red.run, red.s1, red.s2, red.planck))
    assert held[(2, 2)] == held[(4, 6)]


def test_flatten_weights_is_tally_order():
    w = {'voxels': np.arange(2*2*3*4, dtype=np.float32).reshape(2, 2, 3, 4), 'layers': 100+np.arange(10, dtype=np.float32).reshape(2, 5),
         'surface': 200+np.arange(2, dtype=np.float32).reshape(2, 1, 1),
         'planck': {'voxels': np.arange(24, dtype=np.float32).reshape(2, 3, 4), 'layers': np.arange(5, dtype=np.float32), 'surface': np.ones((1, 1), dtype=np.float32)}}
    k, b = flatten_weights(w)
    assert k.shape == (2, 24+5+1) and b.shape == (30,) and k[1, 24] == 105.0 and k[1, -1] == 201.0 and k[0, 23] == 23.0
