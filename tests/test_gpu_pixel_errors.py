"""
Per-pixel standard errors of the backward routes on the GPU (mi3d_set_pixel_errors 1, Rad_mserr = 1): the second tally
rad2 of k_backward_s (cameras) and k_backward_vs (satellite views) and the read-out k_backward_norm_se.

  1  exact           raw rad and rad2 against sum s and sum s^2 of the debug entries' scores, every tally path
  2  formula         radiance_se against the formula in float64 numpy on the raw sums; pixels with one history and with none read 0
  3  additivity      raw rad2 over id ranges and launch sizes
  4  no spread       a scene whose histories all score the same: se <= 1e-6 rad (the clamp, the cancellation floor)
  5  standard error  the spread of 128 independent batch means against the mean of se^2, pixel by pixel
  6  contract        the switch, its refusals, MI3D_ESTATE, the plain builds with the switch off again
  7  run_until       stops below the target, returns max_histories for an unreachable one
  8  drop-in         mcarats_ng(pixel_errors=True) through files and fused: rad_se, bt_se, f_se
  9  two ranks       sharded ids all-reduced against one rank (tests/pixel_errors_dist_worker.py)

Cameras: the scene of tests/test_gpu_backward.py (an 8 x 8 x 5 checkerboard of scattering cloud over a grey surface, an opaque lid) with a
lapse rate, two sensors in the gap, one looking up and one down.  Views: the scattering scene of tests/backward_views_ref.py.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import TARGET_FLUX
from er3t_amd.thermal import dplanck_dT
from tests import backward_views_ref as vref
from tests.test_gpu_backward import cameras, iso_scene, ZS_ISO

pytestmark = pytest.mark.gpu

CAM, CAM_PLAIN = 'k_backward<0,S> [thermal]', 'k_backward<0> [thermal]'
SAT, SAT_PLAIN = 'k_backward<0,V,S> [thermal]', 'k_backward<0,V> [thermal]'
U24 = 2.0**-24


@pytest.fixture(autouse=True)
def defaults_again(solver):
    solver.set_counting(False)               # (the solver is the session's: a test before this file may have left the counting builds on)
    solver.set_kernel(general=False)
    yield
    solver.bind(None, None, None)
    solver.set_tuning(bwd_chunk=-1, batch_log2=30)
    solver.set_counting(False)
    solver.set_pixel_errors(False)
    solver.set_emission_weights(False)
    solver.set_view_profiles(False)
    solver.set_view_method('forward')
    solver.set_camera_method('forward')


def cam_scene(nxr=2, nyr=3, on=1):
    """two sensors (one looking up, one down) in the gap of the checkerboard scene, rectangular map, with a lapse rate so that scores differ"""
    base = dataclasses.replace(iso_scene(), tmp1d=np.linspace(300.0, 272.0, 8))
    sc = cameras(base, [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=2, mrproj=0, nxr=nxr, nyr=nyr, umax=80.0, vmax=180.0)
    return dataclasses.replace(sc, pixel_errors=on)


def sat_scene(nxr=5, nyr=3, on=1):
    """nadir and 45 degrees over the scattering checkerboard and its grey surface; 5 x 3 pixels: one tile of 8 x 8 a view, clipped both ways"""
    sc = vref.scattering_scene(nxr=nxr, nyr=nyr)
    return dataclasses.replace(sc, view_the=[180.0, 135.0], view_phi=[0.0, 70.0], view_zloc=[1.0e6, 1000.0], pixel_errors=on)


def _raw(solver, sc, ranges, seed, chunk=-1, lg=30):
    """the raw tallies of the scene's job over the id ranges [(offset, n), ...] through bound buffers: (rad [npix], rad2 [npix] or None where the
    scene's switch is off) float64, and the kernel's name.  The solver is left with the job run (for the read-outs) and the buffers bound"""
    import torch
    npix = sc.nview*sc.nxr*sc.nyr
    on = bool(sc.pixel_errors)
    rad = torch.zeros(npix, dtype=torch.float64, device='cuda:0')
    rad2 = torch.zeros(npix, dtype=torch.float64, device='cuda:0') if on else None
    solver.bind(rad.data_ptr(), None, None, err_ptr=None if rad2 is None else rad2.data_ptr())
    solver.set_tuning(bwd_chunk=chunk, batch_log2=lg)
    solver.load_scene(sc); solver.reset()
    for off, n in ranges:
        solver.run(n, seed=seed, offset=off)
    solver.sync()
    torch.cuda.synchronize()
    name = solver.kernel_name()
    keep = (rad, rad2)                                                  # (alive until the caller has read out)
    return rad.cpu().numpy().copy(), (rad2.cpu().numpy().copy() if on else None), name, keep


def _scores(solver, sc, seed, N):
    """the scores s of ids [0, N) from the debug entry of the scene's route, and their pixels id mod npix"""
    solver.load_scene(sc)
    if sc.rad_kind == 1:
        s, capped = solver.debug_backward(seed, 0, N)[1:]
    else:
        s, capped = solver.debug_backward_views(seed, 0, N)[2:]
    assert capped == 0
    return s, np.arange(N) % (sc.nview*sc.nxr*sc.nyr)


def _counts(N, npix):
    return N//npix+(np.arange(npix) < N % npix)


def _se_ref(rad, rad2, n):
    n = n.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = np.maximum(rad2-rad*rad/n, 0.0)/(n*(n-1.0))
    return np.where(n >= 2.0, np.sqrt(v), 0.0)


# ---- 1: exact, against the debug entries ---------------------------------------------------------------------------------------------------------

CASES = [('camera-lds', lambda: cam_scene(2, 3), -1, 12*200+5), ('camera-atomics', lambda: cam_scene(24, 24), -1, 1152*20+5),
         ('views-auto', lambda: sat_scene(), -1, 30*200+5), ('views-stride', lambda: sat_scene(), 0, 30*200+5),
         ('views-16', lambda: sat_scene(), 16, 30*200+5)]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_raw_sums_are_the_sums_of_the_debug_scores_and_of_their_squares(solver, case):
    """Every id's score s from the debug entry; after reset and run(N) the raw rad is sum s and the raw rad2 sum s^2 per pixel, float64 sums of
    the same float64 terms in another order: 1e-12.  camera-lds: 12 pixels, both sums per workgroup in LDS; camera-atomics: 1152 pixels, above
    the 1024 of the errors build and below the 2048 of the plain one, two global atomics a history; views: the tile hand-out's two registers
    (auto, 16) and the plain stride (0).  N is no multiple of npix.  radiance() is that of the run with the switch off"""
    tag, make, chunk, N = case
    sc = make()
    npix = sc.nview*sc.nxr*sc.nyr
    assert N % npix == 5
    cam = sc.rad_kind == 1
    seed = 83
    rad, rad2, name, keep = _raw(solver, sc, [(0, N)], seed, chunk=chunk)
    assert name == (CAM if cam else SAT), name
    if not cam and chunk >= 0:
        assert solver.lib.mi3d_debug_backward_chunk(solver._h) == chunk
    img_on = solver.radiance(N)
    s, pix = _scores(solver, sc, seed, N)
    want, want2 = np.bincount(pix, weights=s, minlength=npix), np.bincount(pix, weights=s*s, minlength=npix)
    assert want.min() > 0.0 and np.unique(np.round(s/s.max(), 6)).size > 50           # (the scores differ)
    print('%s: largest relative gap of rad %.2e, of rad2 %.2e' % (tag, np.abs(rad/want-1.0).max(), np.abs(rad2/want2-1.0).max()))
    assert np.allclose(rad, want, rtol=1.0e-12, atol=0.0)
    assert np.allclose(rad2, want2, rtol=1.0e-12, atol=0.0)
    solver.bind(None, None, None)
    off = dataclasses.replace(sc, pixel_errors=0)
    solver.set_tuning(bwd_chunk=chunk)
    solver.load_scene(off); solver.reset(); solver.run(N, seed=seed)
    img_off = solver.radiance(N)
    assert solver.kernel_name() == (CAM_PLAIN if cam else SAT_PLAIN)
    assert img_off.min() > 0.0 and np.allclose(img_on, img_off, rtol=2.0e-7, atol=0.0)


# ---- 2: the formula ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['camera', 'views'])
def test_read_out_is_the_formula_on_the_raw_sums(solver, which):
    """radiance_se(N) against sqrt(max(rad2 - rad^2 / n, 0) / (n (n - 1))) in float64 numpy on the raw sums and the exact counts n of every
    pixel: the device does the same float64 operations and rounds to float32 once (2^-24); 4 x 2^-24 allowed.  N < npix: no pixel has two
    histories, all read 0; N = npix + 3: three pixels have two, the others one and read 0"""
    sc = cam_scene() if which == 'camera' else sat_scene()
    npix = sc.nview*sc.nxr*sc.nyr
    for N in (npix-4, npix+3, 57*npix+11):
        rad, rad2, name, keep = _raw(solver, sc, [(0, N)], seed=89)
        se = solver.radiance_se(N).astype(np.float64).ravel()
        n = _counts(N, npix)
        ref = _se_ref(rad, rad2, n)
        assert np.all(np.isfinite(se)) and se.shape == (npix,)
        assert np.all(se[n < 2] == 0.0)
        if N < npix:
            assert np.all(se == 0.0) and rad2[:N].min() > 0.0 and np.all(rad2[N:] == 0.0)
        else:
            assert np.all(se[n >= 2] > 0.0)
        gap = np.abs(se-ref)[n >= 2]/ref[n >= 2] if (n >= 2).any() else np.zeros(1)
        print('%s N = %d: largest |se / formula - 1| %.2e (allowed %.2e)' % (which, N, gap.max(), 4.0*U24))
        assert np.all(np.abs(se-ref) <= 4.0*U24*ref)
        solver.bind(None, None, None)


# ---- 3: additivity -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['camera', 'views'])
def test_raw_second_tally_adds_over_id_ranges_and_launch_sizes(solver, which):
    sc = cam_scene() if which == 'camera' else sat_scene()
    npix = sc.nview*sc.nxr*sc.nyr
    N, n1 = 700*npix+7, 211*npix+3
    rad, whole, name, keep = _raw(solver, sc, [(0, N)], seed=97)
    assert whole.min() > 0.0
    _, parts, _, keep = _raw(solver, sc, [(0, n1), (n1, N-n1)], seed=97)
    assert np.allclose(parts, whole, rtol=1.0e-12, atol=0.0)
    r12, small, _, keep = _raw(solver, sc, [(0, N)], seed=97, lg=12)
    assert np.allclose(small, whole, rtol=1.0e-12, atol=0.0) and np.allclose(r12, rad, rtol=1.0e-12, atol=0.0)
    solver.bind(None, None, None)


# ---- 4: no spread, no error ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('chunk', [-1, 0])
def test_histories_that_all_score_the_same_have_no_error(solver, chunk):
    """A horizontally uniform, absorbing scene with a lapse rate over a black surface, seen at nadir: a vertical line crosses levels alone,
    every history of every pixel adds the same float32 terms.  rad2 - rad^2 / n is then the rounding of two float64 sums of n terms:
    either sign -- the clamp -- and far below 1e-6 |mean| -- the floor include/mi3d.h states.  Both tally paths of the view build"""
    sc = vref.opaque_scene(views=vref.VIEWS[:1], nxr=5, nyr=3)
    nz = sc.nz
    absk = np.zeros(nz); absk[4] = 2.0e-4; absk[5] = 1.0e-4
    sc = dataclasses.replace(sc, abs1d=absk.astype(np.float32), tmp1d=np.array([299.0, 292.0, 290.0, 288.0, 286.0, 283.0, 279.0], dtype=np.float32),
                             pixel_errors=1)
    npix = sc.nview*sc.nxr*sc.nyr
    N = 1000*npix+7
    rad, rad2, name, keep = _raw(solver, sc, [(0, N)], seed=101, chunk=chunk)
    assert name == SAT
    img, se = solver.radiance(N).astype(np.float64), solver.radiance_se(N).astype(np.float64)
    s, _ = _scores(solver, sc, 101, 4*npix)
    assert np.all(s == s[0]) and s[0] > 0.0                              # (the premise: one score)
    raw = rad2-rad*rad/_counts(N, npix)
    print('no spread (bwd_chunk %d): largest se / rad %.3e (allowed 1e-6); rad2 - rad^2 / n from %.3e to %.3e of rad2'
          % (chunk, (se/img).max(), (raw/rad2).min(), (raw/rad2).max()))
    assert np.all(np.isfinite(se)) and img.min() > 0.0 and np.all(se <= 1.0e-6*img)
    solver.bind(None, None, None)


# ---- 5: it is the standard error -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['camera', 'views'])
def test_se_squared_is_the_variance_of_independent_batch_means(solver, which):
    """M = 128 batches of n = 1000 histories a pixel under seeds of their own.  Per pixel R = var(batch means, ddof = 1) / mean(se^2) follows
    chi^2(M - 1) / (M - 1) -- standard deviation sqrt(2 / (M - 1)) = 0.125 -- up to the relative error of the mean of the variance estimates,
    sqrt((kappa - 1) / (n M)), kappa the kurtosis of a pixel's scores.  |R - 1| <= 4 sqrt(2 / (M - 1)) + 0.1; the 0.1 allows for heavy tails:
    four of the latter standard errors up to kappa = 81, and the kurtosis is printed (measured: DESIGN.md §5.17).  No pixel is left out:
    every pixel of either scene has scatter (se > 0)"""
    sc = cam_scene() if which == 'camera' else sat_scene()
    npix = sc.nview*sc.nxr*sc.nyr
    M, n = 128, 1000
    N = n*npix
    solver.load_scene(sc)
    means, ses = [], []
    for b in range(M):
        solver.reset(); solver.run(N, seed=1000+b)
        means.append(solver.radiance(N).astype(np.float64).ravel())
        ses.append(solver.radiance_se(N).astype(np.float64).ravel())
    assert solver.kernel_name() == (CAM if which == 'camera' else SAT)
    means, ses = np.array(means), np.array(ses)
    assert np.all(ses > 0.0) and np.all(np.isfinite(ses))
    R = means.var(axis=0, ddof=1)/(ses**2).mean(axis=0)
    s, pix = _scores(solver, sc, 1000, N)
    kappa = np.zeros(npix)
    for p in range(npix):
        d = s[pix == p]-s[pix == p].mean()
        kappa[p] = (d**4).mean()/(d**2).mean()**2
    bound = 4.0*np.sqrt(2.0/(M-1))+0.1
    print('%s: R from %.3f to %.3f over %d pixels (allowed 1 +- %.3f); kurtosis of the scores from %.1f to %.1f: the variance estimate is good to '
          '%.3f at worst; se / rad from %.2e to %.2e' % (which, R.min(), R.max(), npix, bound, kappa.min(), kappa.max(),
                                                         np.sqrt((kappa.max()-1.0)/(n*M)), (ses.mean(axis=0)/means.mean(axis=0)).min(),
                                                         (ses.mean(axis=0)/means.mean(axis=0)).max()))
    assert np.all(np.abs(R-1.0) <= bound), R


# ---- 6: the contract -----------------------------------------------------------------------------------------------------------------------------

def test_switch_refusals_and_state(solver):
    lib = solver.lib
    err = lambda: lib.mi3d_last_error().decode()
    cam, sat = cam_scene(on=0), sat_scene(on=0)
    out = np.zeros(64, dtype=np.float32)
    ptr = out.ctypes.data_as(lib.mi3d_get_radiance_se.argtypes[2])
    assert lib.mi3d_set_pixel_errors(solver._h, 2) == -1 and lib.mi3d_set_pixel_errors(solver._h, -1) == -1
    # off: nothing to read
    solver.load_scene(cam); solver.reset(); solver.run(1200, seed=3)
    assert solver.kernel_name() == CAM_PLAIN
    assert lib.mi3d_get_radiance_se(solver._h, 1200, ptr) == -2 and 'mi3d_set_pixel_errors' in err()
    # on, and not served: the weights build, the profiles build, the forward routes, a flux job
    flux = dataclasses.replace(sat, target=TARGET_FLUX)
    for s, cm, vm, wg, pf, word in ((cam, 1, 0, 1, 0, 'mi3d_set_emission_weights'), (sat, 0, 1, 0, 1, 'mi3d_set_view_profiles'),
                                    (cam, 0, 0, 0, 0, 'forward'), (sat, 0, 0, 0, 0, 'forward'), (flux, 0, 1, 0, 0, 'flux'), (flux, 0, 0, 0, 0, 'flux')):
        solver.load_scene(s)
        solver.set_camera_method(cm); solver.set_view_method(vm); solver.set_emission_weights(wg); solver.set_view_profiles(pf); solver.set_pixel_errors(1)
        rc = lib.mi3d_run(solver._h, 1000, 1, 0)
        msg = err()
        solver.set_pixel_errors(0); solver.set_view_profiles(0); solver.set_emission_weights(0); solver.set_view_method(0); solver.set_camera_method(0)
        assert rc == -4 and 'mi3d_set_pixel_errors' in msg and word in msg, (cm, vm, wg, pf, rc, msg)
    # on: nothing to read before a run, and again after a reset
    for sc, name, plain in ((cam_scene(), CAM, CAM_PLAIN), (sat_scene(), SAT, SAT_PLAIN)):
        npix = sc.nview*sc.nxr*sc.nyr
        solver.load_scene(sc)
        assert lib.mi3d_get_radiance_se(solver._h, 1000, ptr) == -2 and 'nothing has been tallied' in err()
        solver.reset()
        assert lib.mi3d_get_radiance_se(solver._h, 1000, ptr) == -2
        solver.run(40*npix, seed=9)
        assert solver.kernel_name() == name
        se = solver.radiance_se(40*npix)
        assert se.shape == (sc.nview, sc.nyr, sc.nxr) and se.dtype == np.float32 and se.min() > 0.0
        solver.reset()
        assert lib.mi3d_get_radiance_se(solver._h, 1000, ptr) == -2
        # the library's own tally was zeroed by the reset: the same run gives the same errors
        solver.run(40*npix, seed=9)
        assert np.allclose(solver.radiance_se(40*npix), se, rtol=2.0*U24, atol=0.0)
        # off again: the plain build, its old name, nothing to read
        solver.set_pixel_errors(0)
        solver.reset(); solver.run(40*npix, seed=9)
        assert solver.kernel_name() == plain
        assert lib.mi3d_get_radiance_se(solver._h, 1000, ptr) == -2 and 'mi3d_set_pixel_errors' in err()
    # the debug entries ignore the switch
    solver.load_scene(sat_scene())
    a = solver.debug_backward_views(9, 0, 64)
    solver.set_pixel_errors(0)
    b = solver.debug_backward_views(9, 0, 64)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    # the refusals of the routes read as before with the switch on
    for s, word in ((dataclasses.replace(sat, solver=2), 'independent columns'), (dataclasses.replace(sat, src_mtype=1, view_method=0), 'solar')):
        msgs = []
        for on in (0, 1):
            solver.load_scene(s)
            solver.set_view_method('backward'); solver.set_pixel_errors(on)
            rc = lib.mi3d_run(solver._h, 1000, 1, 0)
            msgs.append((rc, err()))
            solver.set_pixel_errors(0)
        assert msgs[0][0] == -4 and word in msgs[0][1] and msgs[0] == msgs[1], (word, msgs)


# ---- 7: run_until --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['camera', 'views'])
def test_run_until_stops_when_the_image_is_quiet_enough(solver, which):
    sc = cam_scene() if which == 'camera' else sat_scene()
    npix = sc.nview*sc.nxr*sc.nyr
    solver.load_scene(sc)
    solver.reset(); solver.run(500*npix, seed=31)
    se0 = float(solver.radiance_se(500*npix).max())
    target = 0.4*se0                                                    # (1 / 0.4^2 = 6.25 times the histories: about 3100 a pixel)
    nmax = 64*500*npix
    N = solver.run_until(target, max_histories=nmax, seed=31, chunk=500*npix)
    se = solver.radiance_se(N)
    img = solver.radiance(N)
    print('%s: run_until(%.3e) stopped at %d histories a pixel with max(se) = %.3e' % (which, target, N//npix, se.max()))
    assert N % npix == 0 and 500*npix < N < nmax and float(se.max()) <= target
    assert N % (500*npix) == 0 and float(solver.radiance_se(N).max()) > 0.0
    solver.reset(); solver.run(N, seed=31)
    assert np.allclose(img, solver.radiance(N), rtol=2.0e-7, atol=0.0)
    # relative: every pixel below its own share
    Nr = solver.run_until(0.02, relative=True, max_histories=nmax, seed=31, chunk=500*npix)
    assert Nr % npix == 0 and Nr < nmax and np.all(solver.radiance_se(Nr) <= 0.02*solver.radiance(Nr))
    # an unreachable target: the cap
    few = 6*100*npix
    assert solver.run_until(1.0e-30, max_histories=few, seed=31, chunk=100*npix) == few
    assert solver.run_until(1.0e-30, max_histories=few+npix-1, seed=31, chunk=400*npix) == few


# ---- 8: the drop-in ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['views', 'radiometers'])
@pytest.mark.parametrize('nrun', [1, 3])
def test_dropin_files_against_fused(tmp_path, kind, nrun):
    """mcarats_ng(source='thermal', pixel_errors=True), Ng = 2, through the file route (*.err.bin) and the fused one under the same seeds: the
    same float32 job arrays combined by the same function, so rad_se, bt_se and f_se are equal as arrays; against the formula in numpy on the
    per-job files (float64, rounded once: 2 x 2^-24); bt_se dB/dT = rad_se; out.bin is that of the job without the key"""
    import contextlib
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner, errors_fname, read_errors
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    if kind == 'views':
        sensor = dict(view_method='backward', sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
        shape, name = (12, 10, 2), SAT
    else:
        sensor = dict(camera_method='backward', sensor_type='irradiance', sensor_xpos=[0.1, 0.35, 0.6, 0.85], sensor_ypos=0.5,
                      sensor_altitude=[10.0, 700.0, 10.0, 5000.0], sensor_zenith_angle=[0.0, 0.0, 20.0, 180.0])
        shape, name = (4,), CAM
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target='radiance', surface_albedo=0.05, source='thermal', pixel_errors=True, Nrun=nrun,
                  photons=6e4, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True, **sensor)
        np.random.seed(7)                                    # (mcarats_ng shuffles the seeds over its jobs)
        files = mca.mcarats_ng(fdir=str(tmp_path/'files'), **kw)
        np.random.seed(7)
        fused = mca.mcarats_ng(fdir=str(tmp_path/'fused'), abs_obj=ab, keep_files=False, **kw)
        np.random.seed(7)
        plain = mca.mcarats_ng(fdir=str(tmp_path/'plain'), **dict(kw, pixel_errors=False))
    assert get_runner().sol.kernel_name() == name.replace(',S>', '>')
    assert fused.fused is not None and fused.fused['se'].shape[:2] == (nrun, 2) and files.fused is None
    nml = mca.mca_inp_read(files.fnames_inp[0][0])
    assert nml['Rad_mserr'] == 1
    nview, nyr, nxr = int(nml['Rad_nrad']), int(nml.get('Rad_nyr', 1)), int(nml.get('Rad_nxr', 1))
    se = np.array([[read_errors(errors_fname(f), nview, nyr, nxr) for f in row] for row in files.fnames_out])
    assert se.min() > 0.0 and all(os.path.getsize(errors_fname(f)) == 4*nview*nyr*nxr for f in sum(files.fnames_out, []))
    assert not os.path.exists(errors_fname(plain.fnames_out[0][0]))
    for ig in range(2):                                      # (the same seeds: the same job, the same out.bin but for the order of its sums)
        a, b = mca.mca_out_raw(files.fnames_out[0][ig]).data[0]['data'], mca.mca_out_raw(plain.fnames_out[0][ig]).data[0]['data']
        assert np.allclose(a, b, rtol=2.0e-7, atol=0.0)
    f = np.float32(ab.coef['weight']['data']*1.0e-3).astype(np.float64)
    var = ((f[None, :, None, None, None]*se.astype(np.float64))**2).sum(axis=1)          # (Nrun, nview, nyr, nxr)
    lay = lambda a: np.squeeze(np.transpose(a, (2, 1, 0)+tuple(range(3, a.ndim))))
    want = {'all': lay(np.moveaxis(np.sqrt(var), 0, -1)).reshape(shape+(nrun,)), 'mean': lay(np.sqrt(var.sum(axis=0))/nrun).reshape(shape)}
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=fused, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        keys = ['rad_se']+(['bt_se'] if kind == 'views' else ['f_se'])
        assert sorted(a.keys()) == sorted(b.keys()) and all(k in a for k in keys)
        for k in keys:
            assert a[k]['data'].shape == b[k]['data'].shape == want[mode].shape, (mode, k, a[k]['data'].shape)
            assert np.array_equal(a[k]['data'], b[k]['data']), (mode, k)
        assert np.allclose(b['rad_se']['data'], want[mode], rtol=2.0*U24, atol=0.0) and b['rad_se']['data'].min() > 0.0
        if kind == 'views':
            d = dplanck_dT(files.wlen_um, b['bt']['data'].astype(np.float64))
            assert np.allclose(b['bt_se']['data'].astype(np.float64)*d, b['rad_se']['data'].astype(np.float64)*1.0e3, rtol=2.0*U24, atol=0.0)
            if mode == 'mean':
                print('drop-in views, Nrun = %d: bt_se from %.3f to %.3f K' % (nrun, b['bt_se']['data'].min(), b['bt_se']['data'].max()))
        else:
            assert np.array_equal(b['f_se']['data'], b['rad_se']['data']*np.float32(np.pi))
        if mode == 'mean':
            assert ('rad_std' if kind == 'views' else 'f_std') in b


# ---- 9: two ranks --------------------------------------------------------------------------------------------------------------------------------

def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on the one GPU) against one rank on the same ids (tests/pixel_errors_dist_worker.py):
    the shards of [0, N) add to the job's raw sums -- sums are reduced, never standard errors --: 1e-12.  The read-out of either is rounded to
    float32 once, and the cancellation in rad2 - rad^2 / n magnifies the 1e-16 of the sums' order by rad2 / variance, far below 2^-24: at most
    one float32 apart, 2^-23 relative"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'pixel_errors_dist_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(str(tmp_path), 'result.npz'))
    assert str(z['kernel']) == SAT and int(z['capped']) == 0
    for v in ('rad_raw', 'rad2_raw'):
        a, b = z['dist_'+v], z['solo_'+v]
        print('two ranks against one, %s: largest relative gap %.3e (allowed 1e-12)' % (v, np.abs(a/b-1.0).max()))
        assert a.shape == b.shape == (240,) and b.min() > 0.0 and np.allclose(a, b, rtol=1.0e-12, atol=0.0), v
    ulp = 2.0**-23
    for v in ('se', 'file_rad_se', 'fused_rad_se'):
        a, b = z['dist_'+v].astype(np.float64), z['solo_'+v].astype(np.float64)
        assert a.shape == b.shape and b.min() > 0.0 and np.all(np.abs(a-b) <= ulp*np.maximum(a, b)), v
