"""
Backward Monte Carlo for the satellite views of thermal jobs (mi3d_set_view_method 1, Rad_mvbwd = 1) on the GPU.  Scenes and
the float64 reference: tests/backward_views_ref.py -- 6 x 5 x 4 voxels under two 1-D layers, dx != dy, an image of 20 x 9 pixels (3 x 2 tiles
of 8 x 8, clipped both ways) and three views: nadir from above the top, a down-looking slant from inside the atmosphere with Rad_zref != 0,
an up-looking slant from a plane above the surface.

Every statistical comparison: batches over disjoint id ranges whose size is a multiple of npix, allowance 4 batch standard errors plus the
reference's own error, estimated in the test.  The scattering test takes 16 batches.  The grey surface takes 256: it holds each of 360 pixels
to 4 se, and with the se of 16 batches (Student's t, 15 degrees of freedom: P(|t| > 4) = 1.2e-3) a correct kernel would miss that in one
pixel or another with probability 0.35; with 256 batches the statistic is all but normal (6.3e-5 per pixel, 0.023 for the image).  Single histories: the allowance is 4 x the largest gap between a float32 restatement of the
kernel's sum (tests/test_gpu_backward.py: _march32) and the float64 march over the same lines, computed in the test.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import TARGET_FLUX
from er3t_amd.thermal import planck
from tests import backward_views_ref as vref
from tests import thermal_camera_ref as ref
from tests.test_gpu_backward import _march32

pytestmark = pytest.mark.gpu

NAME = 'k_backward<0,V> [thermal]'
CHUNK = -1                 # the default of mi3d_set_tuning "bwd_chunk": chosen per launch, at most 4


@pytest.fixture(autouse=True)
def defaults_again(solver):
    yield
    solver.set_tuning(bwd_chunk=CHUNK, batch_log2=30)
    solver.set_counting(False)
    solver.set_emission_weights(False)
    solver.set_view_method('forward')


def _chunk(sol):
    """the chunk of the tile hand-out that the last launch ran with (0: the stride)"""
    return sol.lib.mi3d_debug_backward_chunk(sol._h)


def _pixels(sc, ids):
    npix, plane = sc.nview*sc.nxr*sc.nyr, sc.nxr*sc.nyr
    pix = ids % npix
    return pix, pix//plane, (pix % plane)//sc.nxr, pix % sc.nxr


def batches(sol, scene, nb, nper, seed):
    """nb batches over disjoint id ranges: mean image and standard error of that mean, (nview, nyr, nxr)"""
    sol.load_scene(scene)
    out = []
    for b in range(nb):
        sol.reset()
        sol.run(nper, seed=seed, offset=b*nper)
        out.append(sol.radiance(nper).astype(np.float64))
        assert sol.kernel_name() == NAME, sol.kernel_name()
        assert sol.debug_backward_views(seed, 0, 0)[3] == 0          # no history was capped
    a = np.array(out)
    return a.mean(axis=0), a.std(axis=0, ddof=1)/np.sqrt(nb)


# ---- 1: starts ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('chunk', [0, 16])
def test_starts_lie_on_the_sensor_plane_inside_their_pixels(solver, chunk):
    sc = vref.absorbing_scene()
    npix = sc.nview*sc.nxr*sc.nyr
    N, id0 = 20*npix+7, 3
    solver.set_tuning(bwd_chunk=chunk)
    solver.load_scene(sc); solver.reset()
    st, d, score, capped = solver.debug_backward_views(81, id0, N)
    assert capped == 0
    pix, iv, jr, ir = _pixels(sc, id0+np.arange(N))
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    n_p = np.bincount(pix, minlength=npix)
    assert n_p.min() == 20 and n_p.max() == 21
    for v in range(sc.nview):
        vv, zs, zreg = vref.view_geometry(sc, v)
        m = iv == v
        assert np.all(st[m, 2] == np.float32(zs)) and np.all(d[m] == (-vv).astype(np.float32)[None, :])
        t = (zreg-zs)/vv[2]                                          # along v from the sensor plane to the registration level, float64
        for axis, (L, nr, idx, what) in enumerate(((Lx, sc.nxr, ir[m], 'u0'), (Ly, sc.nyr, jr[m], 'u1'))):
            u = np.mod(st[m, axis].astype(np.float64)+vv[axis]*t, L)/(L/nr)-idx
            u = u-nr*np.round((u-0.5)/nr)                            # (the domain is cyclic: 0 and L are the same point)
            edge = float(np.spacing(np.float32(L)))/(L/nr)           # one float32 ulp of the domain length, in pixels
            assert np.all((u >= -edge) & (u <= 1.0+edge)), (v, what, u.min(), u.max(), edge)
            pm = pix[m]
            means = np.bincount(pm, weights=u, minlength=npix)[np.unique(pm)]/n_p[np.unique(pm)]
            tol = 4.5*0.2887/np.sqrt(n_p[np.unique(pm)])
            print('starts: chunk %d, view %d, %s: largest offset of a pixel mean from 0.5: %.4f (allowed %.4f)' % (chunk, v, what, np.abs(means-0.5).max(), tol.min()))
            assert np.all(np.abs(means-0.5) <= tol), (v, what)


# ---- 2: single histories against the line integral ---------------------------------------------------------------------------------------------

def test_single_histories_against_the_line_integral(solver):
    """a scene that never scatters over a black surface: a history IS the line integral from its start along -v"""
    sc = vref.absorbing_scene()
    npix = sc.nview*sc.nxr*sc.nyr
    N = 3*npix                                                       # 540 lines per view
    solver.load_scene(sc); solver.reset()
    st, d, score, capped = solver.debug_backward_views(83, 0, N)
    assert capped == 0
    _, iv, _, _ = _pixels(sc, np.arange(N))
    want = ref.march(sc, st.astype(np.float64), d.astype(np.float64))
    r32 = _march32(sc, st, d)
    gap32 = np.abs(r32/want-1.0).max()
    gap = np.abs(score/want-1.0)
    print('single histories: %d lines; float32 restatement: largest relative gap to the float64 march %.3e; the kernel: %.3e (allowed %.3e)'
          % (N, gap32, gap.max(), 4.0*gap32))
    assert want.min() > 0.0 and all((iv == v).sum() >= 500 for v in range(3))
    assert gap.max() <= 4.0*gap32, (gap.max(), gap32, int(np.argmax(gap)))


# ---- 3: a grey surface ---------------------------------------------------------------------------------------------------------------------------

def test_grey_surface_against_the_line_integral_with_reflection(solver):
    """albedo 0.3 on a 3 x 2 surface with temperature anomalies: every pixel of the down-looking views within 4 se of the pixel mean of the
    line integral with the surface's emission and the downwelling irradiance it reflects, plus that quadrature's own error (halved grid)"""
    sc = vref.absorbing_scene(views=vref.VIEWS[:2], albedo=0.3, sfc2d=True)
    twin = vref.absorbing_scene(views=vref.VIEWS[:2], albedo=0.3)    # the same air over a uniform surface: what the line integral is written for
    _, _, eps, Bs = ref.cells(twin)
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    Bsfc = planck(vref.WL, float(sc.tmp1d[0])+np.asarray(sc.tmps2d, dtype=np.float64))          # (nyb, nxb)

    def surface(m, nmu, nphi):
        r = ref.surface_reflection(twin, m, nmu, nphi)

        def up(x, y):
            ib = np.clip(np.floor(np.mod(x, Lx)/Lx*Bsfc.shape[1]).astype(int), 0, Bsfc.shape[1]-1)
            jb = np.clip(np.floor(np.mod(y, Ly)/Ly*Bsfc.shape[0]).astype(int), 0, Bsfc.shape[0]-1)
            return r(x, y)+eps*(Bsfc[jb, ib]-Bs)                     # (march adds eps Bs of the uniform twin itself)
        return up
    fine, coarse = surface(24, 8, 16), surface(12, 4, 8)
    npix = sc.nview*sc.nxr*sc.nyr
    mean, se = batches(solver, sc, 256, 16*npix, 87)
    for v in range(2):
        want, half = vref.view_image(twin, v, 4, refl=fine), vref.view_image(twin, v, 2, refl=coarse)
        qerr = np.abs(want-half)
        print('grey surface: view %d: largest |image - reference| / reference %.4f, 4 se %.4f, quadrature %.4f'
              % (v, np.abs(mean[v]/want-1.0).max(), (4.0*se[v]/want).max(), (qerr/want).max()))
        assert np.all(4.0*se[v] < 0.05*want) and np.all(qerr < 0.01*want)
        assert np.all(np.abs(mean[v]-want) <= 4.0*se[v]+qerr), (v, np.abs(mean[v]-want).max())


# ---- 4: scattering against the oracle's forward image -------------------------------------------------------------------------------------------

def test_scattering_against_the_oracles_forward_image(solver, oracle, nthreads):
    """a checkerboard cloud, omega = 0.6, a tabulated and an analytic constituent, views 1 and 2, 6 x 6 pixels: the backward image (16
    batches) against the oracle's forward thermal job on the CPU (32 batches of fixed seeds; 2 s on 16 threads, its se below 1 %)"""
    sc = vref.scattering_scene()
    fwd = dataclasses.replace(sc, view_method=0)
    runs = np.array([oracle.run(fwd, 125000, seed=900+b, nthreads=nthreads)['rad'] for b in range(32)], dtype=np.float64)
    mf, sf = runs.mean(axis=0), runs.std(axis=0, ddof=1)/np.sqrt(32.0)
    solver.set_tuning(bwd_chunk=16)                          # (2000 histories a pixel and batch: 125 chunks)
    mb, sb = batches(solver, sc, 16, 2000*72, 89)
    assert _chunk(solver) == 16
    z = ((mb-mf)/np.sqrt(sb**2+sf**2)).ravel()
    M = z.size
    print('scattering: %d pixels; se / value: backward %.4f, forward %.4f (largest); max |z| %.2f, mean z %.3f (allowed %.3f)'
          % (M, (sb/mb).max(), (sf/mf).max(), np.abs(z).max(), z.mean(), 3.0/np.sqrt(M)))
    assert M == 72 and (sb/mb).max() < 0.02 and (sf/mf).max() < 0.02
    assert np.abs(z).max() < 4.5 and abs(z.mean()) < 3.0/np.sqrt(M), (np.abs(z).max(), z.mean())


# ---- 5: every id exactly once --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nxr, nyr, nview', [(20, 9, 3), (3, 2, 1), (1, 1, 1)])
def test_every_id_is_taken_exactly_once(solver, nxr, nyr, nview):
    """an opaque isothermal scene: every history scores B to float32, so raw_tally[p] / B rounds to the number of histories pixel p was given"""
    import torch
    T = 285.0
    B = float(planck(vref.WL, T))
    sc = vref.opaque_scene(views=vref.VIEWS if nview == 3 else vref.VIEWS[1:2], nxr=nxr, nyr=nyr, T=T)
    npix = nview*nxr*nyr
    buf = torch.zeros(npix, dtype=torch.float64, device='cuda:0')
    try:
        solver.bind(buf.data_ptr(), None, None)
        solver.set_counting(True)
        for chunk in (0, 1, 16):
            solver.set_tuning(bwd_chunk=chunk)
            solver.load_scene(sc)
            for id0, N in ((0, 1), (0, 63), (5, npix-1), (npix+3, 5*npix+3), (7, 64*npix)):
                solver.reset()
                solver.run(N, seed=91, offset=id0); solver.sync()
                raw = buf.cpu().numpy()/B
                want = np.bincount((id0+np.arange(N)) % npix, minlength=npix)
                assert solver.kernel_name() == 'k_backward<1,V> [thermal]' and (N == 0 or _chunk(solver) == chunk), (chunk, _chunk(solver))
                assert np.array_equal(np.rint(raw), want) and np.abs(raw-want).max() < 1.0e-4, (chunk, id0, N, raw, want)
                assert solver.counters()['photons'] == N, (chunk, id0, N)
    finally:
        solver.bind(None, None, None)


# ---- 6: bookkeeping ------------------------------------------------------------------------------------------------------------------------------

def test_raw_tallies_add_over_id_ranges(solver):
    import torch
    sc = vref.absorbing_scene(albedo=0.3)
    npix = sc.nview*sc.nxr*sc.nyr
    buf = torch.zeros(npix, dtype=torch.float64, device='cuda:0')
    N, n1 = 37*npix+211, 11*npix+97
    try:
        solver.bind(buf.data_ptr(), None, None)
        solver.set_tuning(bwd_chunk=16)                      # (38 histories a pixel: two full chunks and a partial one)
        solver.load_scene(sc); solver.reset()
        solver.run(N, seed=67); solver.sync()
        whole = buf.cpu().numpy().copy()
        solver.reset()
        solver.run(n1, seed=67); solver.run(N-n1, seed=67, offset=n1); solver.sync()
        parts = buf.cpu().numpy().copy()
        assert solver.kernel_name() == NAME and _chunk(solver) == 16 and solver.debug_backward_views(67, 0, 0)[3] == 0
    finally:
        solver.bind(None, None, None)
    assert whole.min() > 0.0 and np.allclose(parts, whole, rtol=1.0e-12, atol=0.0), (parts/whole-1.0)


def test_same_ids_same_image_whatever_the_hand_out(solver):
    sc = vref.absorbing_scene(albedo=0.3)
    N = 60*sc.nview*sc.nxr*sc.nyr+17
    res = []
    for chunk, lg in ((1, 30), (16, 30), (16, 12), (0, 30)):
        solver.set_tuning(bwd_chunk=chunk, batch_log2=lg)
        solver.load_scene(sc); solver.reset(); solver.run(N, seed=79, offset=1000)
        res.append(solver.radiance(N).astype(np.float64))
        assert solver.kernel_name() == NAME and _chunk(solver) == chunk and solver.debug_backward_views(79, 0, 0)[3] == 0
    solver.set_tuning(bwd_chunk=-1, batch_log2=30)           # the default: at most 4, and here -- 54 tiles for 5120 resident waves -- 1
    solver.load_scene(sc); solver.reset(); solver.run(N, seed=79, offset=1000)
    res.append(solver.radiance(N).astype(np.float64))
    assert 1 <= _chunk(solver) <= 4
    for r in res[1:]:
        assert res[0].min() > 0.0 and np.allclose(res[0], r, rtol=2.0e-7, atol=0.0)           # (float32 read-out of sums in another order)


def test_with_the_switch_off_the_job_runs_the_forward_kernel(solver):
    sc = vref.absorbing_scene()
    solver.load_scene(dataclasses.replace(sc, view_method=0)); solver.reset(); solver.run(20000, seed=3)
    assert solver.kernel_name() == 'k_transport<0,1,0,0> [thermal]', solver.kernel_name()
    solver.load_scene(sc); solver.reset(); solver.run(20000, seed=3)
    assert solver.kernel_name() == NAME


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_what_the_route_does_not_serve_is_refused(solver):
    sc = vref.absorbing_scene()
    lsrt = dataclasses.replace(sc, sfc_mtype=4, sfc_param=np.array([0.1, 0.05, 0.02, 0, 0], dtype=np.float32))
    cams = dataclasses.replace(sc, view_method=0, rad_kind=1, view_the=[180.0], view_phi=[0.0], view_zloc=[500.0], nxr=2, nyr=2, cam_images=0)
    cases = [(dataclasses.replace(sc, src_mtype=1, view_method=0), 'solar', False),
             (dataclasses.replace(sc, src_mtype=2, src_fsol=5.0, src_the=150.0, view_method=0), 'solar+thermal', False),
             (dataclasses.replace(sc, target=TARGET_FLUX), 'flux', False),
             (dataclasses.replace(sc, solver=1), 'partial 3-D', False),
             (dataclasses.replace(sc, solver=2), 'independent columns', False),
             (lsrt, 'Lambertian', False),
             (sc, 'emission weights', True),
             (cams, 'Rad_mrkind=1', False)]
    for s, word, weights in cases:
        try:
            solver.load_scene(s)
        except OSError:
            pass                                             # (mi3d_prepare refuses the LSRT surface of a thermal job already)
        solver.set_view_method('backward')
        solver.set_emission_weights(weights)
        rc = solver.lib.mi3d_run(solver._h, 1000, 1, 0)
        msg = solver.lib.mi3d_last_error().decode()
        solver.set_emission_weights(False)
        assert rc == -4 and word in msg and (s is lsrt or 'mi3d_set_view_method 1' in msg), (word, rc, msg)
    below = dataclasses.replace(sc, view_zloc=[1.0e6, 0.0, 150.0])
    solver.load_scene(below)
    assert solver.lib.mi3d_run(solver._h, 1000, 1, 0) == -1 and 'surface' in solver.lib.mi3d_last_error().decode()
    assert solver.lib.mi3d_set_view_method(solver._h, 2) == -1
    # no view set: MI3D_ESTATE from mi3d_run under either hand-out and from the debug entry, as the forward route answers
    for chunk in (-1, 0, 16):
        solver.set_tuning(bwd_chunk=chunk)
        solver.load_scene(dataclasses.replace(sc, view_the=[], view_phi=[], view_zloc=[]))
        assert solver.lib.mi3d_run(solver._h, 1000, 1, 0) == -2 and 'no view' in solver.lib.mi3d_last_error().decode()
        with pytest.raises(OSError) as err:
            solver.debug_backward_views(1, 0, 8)
        assert 'no view' in str(err.value)
    solver.set_tuning(bwd_chunk=-1)
    solver.load_scene(sc); solver.reset(); solver.run(1000, seed=1)
    assert solver.kernel_name() == NAME and solver.radiance(1000).max() > 0.0


# ---- the drop-in ---------------------------------------------------------------------------------------------------------------------------------

def test_dropin_files_against_fused_statistics(tmp_path):
    """mcarats_ng(source='thermal', view_method='backward') with two views: the file route and the fused statistics (abs_obj, keep_files=False)
    under the same seeds, bit for bit; rad, bt and the view axis as for a forward job"""
    import contextlib
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=3)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=3, target='radiance', surface_albedo=0.05, source='thermal', view_method='backward', Nrun=3,
                  photons=6e4, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True,
                  sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
        np.random.seed(7)                                    # (mcarats_ng shuffles the seeds over its jobs)
        files = mca.mcarats_ng(fdir=str(tmp_path/'files'), **kw)
        np.random.seed(7)
        fused = mca.mcarats_ng(fdir=str(tmp_path/'fused'), abs_obj=ab, keep_files=False, **kw)
    sol = get_runner().sol
    assert sol.kernel_name() == NAME and sol.debug_backward_views(1, 0, 0)[3] == 0
    assert fused.fused is not None and files.fused is None
    nml = mca.mca_inp_read(files.fnames_inp[0][0])
    assert nml['Rad_mvbwd'] == 1 and nml['Rad_mrkind'] == 2 and [mca.mca_inp_read(f)['Wld_jseed'] for f in sum(files.fnames_inp, [])] == \
        [mca.mca_inp_read(f)['Wld_jseed'] for f in sum(fused.fnames_inp, [])]
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=fused, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys()) and 'bt' in a
        for k in ('rad', 'bt'):
            assert a[k]['data'].shape == b[k]['data'].shape and a[k]['data'].shape[:3] == (12, 10, 2), (mode, k, a[k]['data'].shape)
            assert np.array_equal(a[k]['data'], b[k]['data']), (mode, k)
    bt = b['bt']['data']
    assert np.all(bt > 200.0) and np.all(bt < 300.0)


def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on the one GPU) against one rank on the same ids: the shards of [0, N) add to the
    job's raw tally, and the read-out divides by the job's counts (tests/backward_views_dist_worker.py)"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'backward_views_dist_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(str(tmp_path), 'result.npz'))
    assert str(z['kernel']) == NAME and int(z['capped']) == 0
    a, b = z['job_dist_rad'].astype(np.float64), z['job_solo_rad'].astype(np.float64)
    # The same histories.  Two ranks and one differ in the order of the float64 sums of a pixel (1e-16 relative); either value is then rounded
    # to float32 once, so the two lie on the same or on neighbouring float32 numbers: at most 2^-23 relative
    ulp = 2.0**-23
    print('two ranks against one: largest relative gap %.3e (allowed %.3e)' % (np.abs(a/b-1.0).max(), ulp))
    assert a.shape == b.shape == (2, 10, 12) and a.min() > 0.0 and np.all(np.abs(a-b) <= ulp*np.maximum(a, b)), np.abs(a/b-1.0).max()
    # File route against fused statistics under the same seeds: again the same histories.  What differs is where float32 roundings fall.  Either
    # route rounds a job's image to float32 (the fused one on every rank, for the rank's share), multiplies it by the g's factor and adds it
    # to the run's sum over g in float32: 3 roundings per g; the fused route then adds the ranks' run fields in float32 (1); the mean over the
    # runs is rounded once by either.  All terms are positive, so a rounding moves the result by at most 2^-24 of it: 3 Ng + 1 = 7 for the
    # file route and 3 Ng + 2 = 8 for the fused one, 15 in all with Ng = 2.  bt moves less than rad does, relatively.
    assert list(z['seeds_file']) == list(z['seeds_fused'])
    tol = 15.0*2.0**-24
    for v in ('rad', 'bt'):
        a, b = z['file_'+v].astype(np.float64), z['fused_'+v].astype(np.float64)
        print('file route against fused statistics, %s: largest relative gap %.3e (allowed %.3e)' % (v, np.abs(a/b-1.0).max(), tol))
        assert a.shape == b.shape and a.shape[:3] == (12, 10, 2) and b.min() > 0.0 and np.all(np.abs(a-b) <= tol*np.maximum(a, b)), v
