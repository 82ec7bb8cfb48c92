"""
Per-layer profiles of the backward route's satellite views (mi3d_set_view_profiles 1, Rad_mvprf = 1): what the host layers
do without a GPU -- the namelist key and its round trip, the refusals of mcarats_ng, Scene and mca_exe, the .prf.bin file with the g / run
reduction of its reader, the header against the binding, and the reference helper of the GPU tests against the line's transmittance.
"""

import contextlib
import io
import os
import re

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd import solver as solver_mod
from er3t_amd.rtm.mca import mca_exe
from er3t_amd.rtm.mca.mca_exe import _check_supported
from er3t_amd.rtm.mca.mca_out import read_view_profiles, g_factors
from er3t_amd.scene import Scene
from er3t_amd.synth import atm_synth, abs_synth
from tests import backward_views_ref as vref
from tests import emission_weights_ref as wref
from tests import view_profiles_ref as pref
from tests.golden import inputs as gin


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 2, 'Rad_mvbwd': 1, 'Rad_mvprf': 1, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3,
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


def _write(a1, ab, fdir, target='radiance', Nrun=1, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=2, target=target, surface_albedo=0.03, fdir=fdir, Nrun=Nrun, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


_text = lambda m: [l for l in open(m.fnames_inp[0][0]).read().splitlines() if 'Wld_jseed' not in l]
IRRADIANCE = dict(sensor_type='irradiance', sensor_xpos=[0.2, 0.7], sensor_ypos=0.5, sensor_altitude=10.0, sensor_zenith_angle=[0.0, 180.0])


def test_the_key_is_written_only_when_asked_and_every_other_file_is_unchanged(tmp_path):
    _, ab, a1 = _objects(11000.0)
    _, abs_sol, a1s = _objects(650.0)
    jobs = [(a1, ab, dict(source='thermal')), (a1, ab, dict(source='thermal', view_method='backward')),
            (a1, ab, dict(source='thermal', view_method='backward', sensor_zenith_angle=[0.0, 40.0])),
            (a1, ab, dict(source='thermal', target='flux')), (a1, ab, dict(source='thermal', camera_method='backward', **IRRADIANCE)),
            (a1s, abs_sol, dict()), (a1s, abs_sol, dict(target='flux'))]
    for i, (a, b, kw) in enumerate(jobs):
        x = _text(_write(a, b, str(tmp_path/('a%d' % i)), **kw))
        y = _text(_write(a, b, str(tmp_path/('b%d' % i)), view_profiles=False, **kw))
        assert x == y and not any('Rad_mvprf' in l for l in x), kw
    for i, kw in enumerate((dict(), dict(sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0]))):
        off = _write(a1, ab, str(tmp_path/('f%d' % i)), source='thermal', view_method='backward', **kw)
        on = _write(a1, ab, str(tmp_path/('v%d' % i)), source='thermal', view_method='backward', view_profiles=True, **kw)
        tf, tb = _text(off), _text(on)
        assert sum('Rad_mvprf' in l for l in tb) == 1 and [l for l in tb if 'Rad_mvprf' not in l] == tf
        rad = tb[tb.index('&mcarRad_nml_job'):]
        assert any('Rad_mvprf' in l for l in rad[1:rad.index('/')])
        assert on.view_profiles is True and off.view_profiles is False


def test_round_trip_into_a_scene_with_profiles(tmp_path):
    _, ab, a1 = _objects(11000.0)
    on = _write(a1, ab, str(tmp_path/'v'), source='thermal', view_method='backward', view_profiles=True, sensor_zenith_angle=[0.0, 40.0])
    off = _write(a1, ab, str(tmp_path/'f'), source='thermal', view_method='backward', sensor_zenith_angle=[0.0, 40.0])
    nml = mca.mca_inp_read(on.fnames_inp[0][0])
    assert nml['Rad_mvprf'] == 1 and nml['Rad_mvbwd'] == 1 and nml['Src_mtype'] == 3 and nml['Rad_mrkind'] == 2
    _check_supported(nml, str(tmp_path/'v'), solver=0)
    sc = Scene.from_nml(nml, str(tmp_path/'v'), solver=0)
    assert sc.view_profiles == 1 and sc.view_method == 1 and sc.rad_kind == 2 and sc.nview == 2
    nmf = mca.mca_inp_read(off.fnames_inp[0][0])
    assert 'Rad_mvprf' not in nmf and Scene.from_nml(nmf, str(tmp_path/'f'), solver=0).view_profiles == 0


def test_refusals_of_mcarats_ng_scene_and_mca_exe(tmp_path):
    _, ab, a1 = _objects(11000.0)
    for kw in (dict(source='thermal', view_profiles=True), dict(source='thermal', view_method='forward', view_profiles=True),
               dict(view_profiles=True), dict(source='thermal', camera_method='backward', view_profiles=True, **IRRADIANCE)):
        with pytest.raises(OSError) as err:
            _write(a1, ab, str(tmp_path/'bad'), **kw)
        assert 'view_profiles' in str(err.value) and 'view_method' in str(err.value), (kw, str(err.value))
    # the namelist: the key without Rad_mvbwd = 1, and values other than 0 and 1
    for kw in (dict(Rad_mvbwd=None), dict(Rad_mvbwd=0), dict(Rad_mvprf=2), dict(Rad_mvprf=-1), dict(Rad_mvprf=0.5)):
        for check in (lambda n: _check_supported(n, None, solver=0), lambda n: Scene.from_nml(n, str(tmp_path), solver=0)):
            with pytest.raises(OSError) as err:
                check(_nml(**kw))
            assert 'Rad_mvprf' in str(err.value), (kw, str(err.value))
    _check_supported(_nml(), None, solver=0); _check_supported(_nml(Rad_mvprf=0), None, solver=0); _check_supported(_nml(Rad_mvprf=0, Rad_mvbwd=0), None, solver=0)
    assert Scene.from_nml(_nml(), str(tmp_path), solver=0).view_profiles == 1 and Scene.from_nml(_nml(Rad_mvprf=0), str(tmp_path), solver=0).view_profiles == 0
    base = dict(zgrd=[0.0, 1000.0], ext1d=[0.0], omg1d=[1.0], apf1d=[-1.0], abs1d=[1e-4], nx=1, ny=1, dx=1000.0, dy=1000.0, target=2,
                view_the=[180.0], view_phi=[0.0], view_zloc=[1e6], src_mtype=3, src_wlen=11.0, tmp1d=[290.0, 280.0])
    assert Scene(rad_kind=2, view_method=1, view_profiles=1, **base).view_profiles == 1 and Scene(rad_kind=2, view_method=1, **base).view_profiles == 0
    for kw in (dict(rad_kind=2, view_method=0, view_profiles=1), dict(rad_kind=1, cam_method=1, view_profiles=1, cam_images=0),
               dict(rad_kind=2, view_method=1, view_profiles=2), dict(rad_kind=2, view_method=1, view_profiles=-1),
               dict(rad_kind=2, view_method=1, view_profiles=0.5)):
        with pytest.raises(ValueError) as err:
            Scene(**dict(base, **kw))
        assert 'Rad_mvprf' in str(err.value), kw


def test_header_declares_what_the_binding_lists():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'mi3d.h')).read()
    declared = set(re.findall(r'^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(mi3d_\w+)\s*\(', text, flags=re.M))
    listed = {s[0]: s for s in solver_mod._SIGNATURES}
    for name in ('mi3d_set_view_profiles', 'mi3d_bind_view_profiles_buffer', 'mi3d_get_view_profiles'):
        assert name in declared and name in listed, name
    assert len(listed['mi3d_get_view_profiles'][2]) == 4 and len(listed['mi3d_set_view_profiles'][2]) == 2
    for method in ('set_view_profiles', 'view_profiles'):
        assert callable(getattr(solver_mod.Mi3dSolver, method))
    import inspect
    assert 'prf_ptr' in inspect.signature(solver_mod.Mi3dSolver.bind).parameters


@pytest.mark.parametrize('mode', ['mean', 'all'])
def test_prf_bin_round_trip_and_the_g_run_reduction(tmp_path, mode):
    """synthetic profiles through JobRunner.write's helpers and back through read_view_profiles, against a numpy restatement"""
    _, ab, a1 = _objects(11000.0)
    m = _write(a1, ab, str(tmp_path/'v'), Nrun=3, source='thermal', view_method='backward', view_profiles=True,
               sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
    nml = mca.mca_inp_read(m.fnames_inp[0][0])
    nview, nyr, nxr, nz = int(nml['Rad_nrad']), int(nml.get('Rad_nyr', 1)), int(nml.get('Rad_nxr', 1)), int(nml['Atm_nz'])
    assert nview == 2 and nz == 16
    npix, nrow = nview*nyr*nxr, nz+1
    rng = np.random.default_rng(5)
    jobs = []
    for ir in range(m.Nrun):
        row = []
        for ig in range(m.Ng):
            k = rng.uniform(0.0, 1.0, size=(nview, nyr, nxr, nrow)).astype(np.float32)
            k[..., 3] = 0.0                                   # a row no line crosses
            c = (k*rng.uniform(5.0, 9.0, size=k.shape)).astype(np.float32)
            flat = mca_exe.flatten_profiles({'weight': k, 'contribution': c})
            assert flat.shape == (2, npix, nrow) and flat.dtype == np.float32
            fname = mca_exe.profiles_fname(m.fnames_out[ir][ig])
            assert fname.endswith('.prf.bin') and not fname.endswith('.out.bin.prf.bin')
            mca_exe.write_profiles(fname, flat)
            assert os.path.getsize(fname) == 4*2*npix*nrow
            back = mca_exe.read_profiles(fname, npix, nrow)
            assert np.array_equal(back, flat)
            row.append(flat)
        jobs.append(row)
    with pytest.raises(OSError):
        mca_exe.read_profiles(fname, npix+1, nrow)
    factors, _ = g_factors(m, ab, 1)
    runs, mean, std = pref.reduce_runs(jobs, factors[0])
    data = read_view_profiles(m, ab, mode=mode, squeeze=False)
    lay = lambda a: np.transpose(a.reshape((nview, nyr, nxr, nrow)+a.shape[2:]), (2, 1, 0, 3)+tuple(range(4, 2+a.ndim)))
    if mode == 'all':
        assert sorted(data) == ['view_contribution', 'view_layer_planck', 'view_weight']
        assert data['view_weight']['data'].shape == (nxr, nyr, nview, nrow, m.Nrun) and data['view_weight']['dims_info'] == ['Nxr', 'Nyr', 'Nview', 'Nz+1', 'Nr']
        assert np.allclose(data['view_weight']['data'], lay(runs[0]), rtol=2.0**-23, atol=0.0)
        assert np.allclose(data['view_contribution']['data'], lay(runs[1]), rtol=2.0**-23, atol=0.0)
        kk, cc = lay(runs[0]), lay(runs[1])
    else:
        assert sorted(data) == ['view_contribution', 'view_contribution_std', 'view_layer_planck', 'view_weight', 'view_weight_std']
        assert data['view_weight']['data'].shape == (nxr, nyr, nview, nrow) and data['view_weight']['dims_info'] == ['Nxr', 'Nyr', 'Nview', 'Nz+1']
        assert np.allclose(data['view_weight']['data'], lay(mean[0]), rtol=2.0**-23, atol=0.0)
        assert np.allclose(data['view_contribution']['data'], lay(mean[1]), rtol=2.0**-23, atol=0.0)
        # (a float32 of a standard deviation formed from sums of squares: absolute, at the rounding of the mean's square)
        assert np.allclose(data['view_weight_std']['data'], lay(std[0]), rtol=1.0e-4, atol=1.0e-6*float(mean[0].max()))
        assert np.allclose(data['view_contribution_std']['data'], lay(std[1]), rtol=1.0e-4, atol=1.0e-6*float(mean[1].max()))
        kk, cc = lay(mean[0]), lay(mean[1])
    b = data['view_layer_planck']['data']
    assert b.shape == data['view_weight']['data'].shape and np.all(np.isnan(b[:, :, :, 3]))
    ok = kk > 0.0
    assert np.array_equal(np.isnan(b), ~ok) and np.allclose(b[ok], (cc[ok]/kk[ok]), rtol=4.0*2.0**-23, atol=0.0)
    # squeeze drops the pixel axes of length 1 and nothing else
    sq = read_view_profiles(m, ab, mode=mode, squeeze=True)['view_weight']
    assert sq['data'].shape == tuple(n for i, n in enumerate(data['view_weight']['data'].shape) if i >= 3 or n > 1)
    assert sq['dims_info'] == [d for d, n in zip(data['view_weight']['dims_info'], data['view_weight']['data'].shape) if d not in ('Nxr', 'Nyr', 'Nview') or n > 1]


def test_layer_sums_of_the_line_weights_add_up_to_one_minus_the_transmittance():
    """the reference helper of the GPU tests: for lines that end at a black surface sum_k K_ref[k] = 1 - exp(-tau) over the layers and
    K_ref[nz] = exp(-tau) for the surface, tau the line's absorption optical depth worked out here layer by layer and voxel by voxel"""
    sc = vref.absorbing_scene(albedo=0.0)
    rng = np.random.default_rng(3)
    n = 40
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    org = np.stack([rng.uniform(0.0, Lx, n), rng.uniform(0.0, Ly, n), np.full(n, float(sc.zgrd[-1]))], axis=-1)
    the = np.radians(rng.uniform(0.0, 50.0, n)); phi = rng.uniform(0.0, 2.0*np.pi, n)
    d = np.stack([np.sin(the)*np.cos(phi), np.sin(the)*np.sin(phi), -np.cos(the)], axis=-1)
    d[0] = (0.0, 0.0, -1.0)                                    # a vertical line among them
    K = wref.line_weights(sc, org, d)
    rows, crow = pref.line_profiles(sc, org, d)
    assert rows.shape == crow.shape == (n, sc.nz+1) and np.all(rows >= 0.0)
    assert np.allclose(rows.sum(axis=1), K.sum(axis=1), rtol=1.0e-14, atol=0.0)
    # the optical depth by a walk of its own: fine steps along the line, the cell looked up at every midpoint
    ka, B, eps, nvox, nsfc = wref.cell_tables(sc)
    assert eps.size == 1 and eps[0] == 1.0
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    m = 200000
    for i in range(0, n, 8):
        smax = (zg[-1]-zg[0])/-d[i, 2]
        s = (np.arange(m)+0.5)*smax/m
        p = org[i][None, :]+s[:, None]*d[i][None, :]
        k = np.clip(np.searchsorted(zg, p[:, 2], side='right')-1, 0, sc.nz-1)
        ix = np.floor(np.mod(p[:, 0], Lx)/sc.dx).astype(int) % sc.nx; iy = np.floor(np.mod(p[:, 1], Ly)/sc.dy).astype(int) % sc.ny
        k3 = k-(sc.iz3l-1)
        in3 = (k3 >= 0) & (k3 < sc.nz3)
        kk = np.where(in3, ka[(np.clip(k3, 0, sc.nz3-1)*sc.ny+iy)*sc.nx+ix], ka[nvox+k])
        tau = kk.sum()*smax/m
        # (midpoint rule over cells of constant ka: its error is one step at each of the line's < 40 faces)
        tol = 40.0*ka.max()*smax/m
        assert abs(rows[i, :sc.nz].sum()-(1.0-np.exp(-tau))) <= tol and abs(rows[i, sc.nz]-np.exp(-tau)) <= tol, (i, rows[i], tau)
        # per layer: the transmittance in front of the layer times its own absorptance
        for kl in range(sc.nz):
            sel = k == kl
            t_front = np.exp(-(kk[k > kl].sum())*smax/m); t_lay = kk[sel].sum()*smax/m
            assert abs(rows[i, kl]-t_front*(1.0-np.exp(-t_lay))) <= tol, (i, kl)
    # rows of C are the rows of K times one Planck radiance where the layer is uniform (the two 1-D layers above the voxels)
    for kl in (4, 5):
        assert np.allclose(crow[:, kl], rows[:, kl]*B[nvox+kl], rtol=1.0e-14, atol=0.0)
