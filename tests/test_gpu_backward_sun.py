"""
The sunlight term of the backward satellite views (mi3d_set_view_sunlight 1, Rad_mvsun = 1) on the GPU: solar+thermal jobs
(Src_mtype = 2) served by k_backward_vn / k_backward_vns.  Scenes and the float64 reference: tests/backward_sun_ref.py.

References: the closed form of a history that meets nothing but an absorbing atmosphere and a reflecting surface (single histories, float64
against a float32 restatement of the kernel's own sums); the thermal job itself (Src_fsol = 0, bit for bit); linearity in Src_fsol on the same
ids; the deterministic plane-parallel solver oracle/k16.py (multiple anisotropic scattering, twelve views); the CPU oracle's forward solar and
thermal runs, summed (a 3-D cloud).  Every test here fails without the feature: the library refuses the job.
"""

import dataclasses

import numpy as np
import pytest

from er3t_amd.scene import TARGET_FLUX
from er3t_amd.thermal import planck
from tests import backward_sun_ref as sref
from tests import backward_views_ref as vref
from tests.test_k16 import ORACLE_CASES, slab, k16_answer, compare, check_group

pytestmark = pytest.mark.gpu

SUN = 'k_backward<0,V,N> [solar+thermal]'
SUN_ERR = 'k_backward<0,V,N,S> [solar+thermal]'
PLAIN = 'k_backward<0,V> [thermal]'


@pytest.fixture(autouse=True)
def defaults_again(solver):
    yield
    solver.bind(None, None, None)
    solver.set_tuning(bwd_chunk=-1, batch_log2=30)
    solver.set_counting(False)
    solver.set_emission_weights(False)
    solver.set_view_profiles(False)
    solver.set_pixel_errors(False)
    solver.set_view_sunlight(False)
    solver.set_view_method('forward')


def batches(sol, scene, nb, nper, seed, name=SUN):
    """nb batches over disjoint id ranges: mean image and standard error of that mean, (nview, nyr, nxr), and the batches themselves"""
    sol.load_scene(scene)
    out = []
    for b in range(nb):
        sol.reset()
        sol.run(nper, seed=seed, offset=b*nper)
        out.append(sol.radiance(nper).astype(np.float64))
        assert sol.kernel_name() == name, sol.kernel_name()
    assert sol.debug_backward_views(seed, 0, 0)[3] == 0              # nothing was capped, no history and no sun ray
    a = np.array(out)
    return a.mean(axis=0), a.std(axis=0, ddof=1)/np.sqrt(nb), a


def _raw(sol, scene, ranges, seed, chunk, name):
    """the raw float64 tally after the id ranges [(id0, n), ...] of scene"""
    import torch
    npix = scene.nview*scene.nxr*scene.nyr
    buf = torch.zeros(npix, dtype=torch.float64, device='cuda:0')
    try:
        sol.bind(buf.data_ptr(), None, None)
        sol.set_tuning(bwd_chunk=chunk)
        sol.load_scene(scene); sol.reset()
        for id0, n in ranges:
            sol.run(n, seed=seed, offset=id0)
        sol.sync()
        assert sol.kernel_name() == name, sol.kernel_name()
        assert sol.debug_backward_views(seed, 0, 0)[3] == 0
        return buf.cpu().numpy().copy()
    finally:
        sol.bind(None, None, None)


# ---- 1: single histories against the closed form ---------------------------------------------------------------------------------------------

def _history32(sc, st, d):
    """the kernel's sums for a scene that neither scatters nor emits, restated in float32: the incremental walk on (tx, ty, tz) down to the
    surface with w *= exp(-ka l) per cell, the coefficient w (1 - eps) / pi F mu0 there, and the sun ray from the hit point -- the same walk
    on the ray's own (tx, ty, tz), tau += (ka + ks) l per cell, closed above the 3-D region with the layer table's bt, dz and tabove"""
    f = np.float32
    ke = sref.extinction(sc)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    dzl = np.diff(zg).astype(f)
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, f(sc.dx), f(sc.dy)
    k3lo, k3hi = sc.iz3l-1, sc.iz3l-1+sc.nz3
    bt = ke[:, 0, 0].astype(f)                                       # (read outside the 3-D region only)
    tabove = np.array([float((ke[k+1:, 0, 0]*np.diff(zg)[k+1:]).sum()) for k in range(nz)]).astype(f)
    ke = ke.astype(f)
    alb = np.asarray(sc.psfc[0], dtype=f)
    nyb, nxb = alb.shape
    sfx, sfy = f(nxb/(sc.nx*sc.dx)), f(nyb/(sc.ny*sc.dy))
    sun = sref.sun_direction(sc.src_the, sc.src_phi).astype(f)
    F, mu0 = f(sc.src_fsol), f(abs(sun[2]))
    tiny = f(1e-20)

    def dda(u, px, py, pz, dzk):
        ax, ay, az = f(1)/max(abs(u[0]), tiny), f(1)/max(abs(u[1]), tiny), f(1)/max(abs(u[2]), tiny)
        return (f(dx*ax), f(dy*ay), az, f((dx-px if u[0] > 0 else px)*ax), f((dy-py if u[1] > 0 else py)*ay), f((dzk-pz if u[2] > 0 else pz)*az))

    out = np.zeros(len(d))
    for i, (o, u) in enumerate(zip(np.asarray(st, dtype=f), np.asarray(d, dtype=f))):
        k = int(np.clip(np.searchsorted(zg, float(o[2]), side='right')-1, 0, nz-1))
        if float(o[2]) == zg[k] and u[2] < 0 and k > 0:
            k -= 1
        cx, cy = np.floor(o[0]/dx), np.floor(o[1]/dy)
        px, py, pz = f(o[0]-cx*dx), f(o[1]-cy*dy), f(o[2]-f(zg[k]))
        ix, iy = int(cx) % nx, int(cy) % ny
        sx, sy, az, tx, ty, tz = dda(u, px, py, pz, dzl[k])
        w = f(1)
        while True:                                                   # the line of sight down to the surface
            in3d = k3lo <= k < k3hi
            ds = min(tx, ty, tz) if in3d else tz
            w = f(w*np.exp(-f(ke[k, iy, ix]*ds), dtype=f))
            hz = (not in3d) or (tz <= tx and tz <= ty)
            hx = (not hz) and tx <= ty
            tx, ty, tz = f(tx-ds), f(ty-ds), f(tz-ds)
            if not in3d:
                if tx < 0:
                    nc = np.floor(-tx/sx)+1; tx = f(tx+f(nc)*sx); ix = int(ix+(nc if u[0] > 0 else -nc)) % nx
                if ty < 0:
                    nc = np.floor(-ty/sy)+1; ty = f(ty+f(nc)*sy); iy = int(iy+(nc if u[1] > 0 else -nc)) % ny
            if hz:
                k -= 1
                if k < 0:
                    break
                tz = f(dzl[k]*az)
            elif hx:
                tx = sx; ix = (ix+(1 if u[0] > 0 else -1)) % nx
            else:
                ty = sy; iy = (iy+(1 if u[1] > 0 else -1)) % ny
        ex, ey = f(tx*max(abs(u[0]), tiny)), f(ty*max(abs(u[1]), tiny))
        px = min(max(f(dx-ex) if u[0] > 0 else ex, f(0)), dx); py = min(max(f(dy-ey) if u[1] > 0 else ey, f(0)), dy)
        ib, jb = min(int(f(f(f(ix)*dx+px)*sfx)), nxb-1), min(int(f(f(f(iy)*dy+py)*sfy)), nyb-1)
        eps = f(1.0-min(max(float(alb[jb, ib]), 0.0), 1.0))
        c = f(f(f(f(w*f(f(1)-eps))*f(1.0/np.float32(np.pi)))*mu0)*F)
        v = -sun
        k = 0
        sx, sy, az, tx, ty, tz = dda(v, px, py, f(0), dzl[0])
        tau = f(0)
        while True:                                                   # the sun ray
            if k >= k3hi:                                             # (a scene without layers below its 3-D region)
                tau = f(float(tau)+float(f(float(bt[k])*float(dzl[k])+float(tabove[k])))*float(az))
                break
            ds = min(tx, ty, tz)
            tau = f(float(ke[k, iy, ix])*float(ds)+float(tau))
            hz = tz <= tx and tz <= ty
            hx = (not hz) and tx <= ty
            tx, ty, tz = f(tx-ds), f(ty-ds), f(tz-ds)
            if hz:
                k += 1
                if k >= nz:
                    break
                tz = f(dzl[k]*az)
            elif hx:
                tx = sx; ix = (ix+(1 if v[0] > 0 else -1)) % nx
            else:
                ty = sy; iy = (iy+(1 if v[1] > 0 else -1)) % ny
        out[i] = float(f(c*np.exp(-tau, dtype=f)))
    return out


@pytest.mark.parametrize('the, phi', [(120.0, 40.0), (180.0, 0.0)], ids=['slant_sun_wraps', 'vertical_sun'])
def test_single_histories_against_the_closed_form(solver, the, phi):
    """no scattering, nothing emits (20 K: planck(3.75, 20) is 0 in float32), a 3 x 2 albedo map: a history's score IS the one term
    w_sfc a / pi F mu0 T_sun at its hit point.  Src_the = 120: the sun ray from the surface travels 2.6 km horizontally through a domain of
    1.8 x 1.25 km, it wraps in x and y; Src_the = 180: the exactly vertical sun, which must keep its column.  Allowance: 4 x the largest gap
    between the float32 restatement above and float64, as tests/test_gpu_backward_views.py::test_single_histories_against_the_line_integral"""
    sc = sref.absorbing_sunlit(the, phi)
    assert np.float32(planck(sref.WL, sref.COLD+6.0)) == 0.0          # (the warmest cell: 20 K + 5.5 K of anomalies)
    npix = sc.nview*sc.nxr*sc.nyr
    N = 3*npix
    solver.load_scene(sc); solver.reset()
    st, d, score, capped = solver.debug_backward_views(83, 0, N)
    assert capped == 0
    iv = (np.arange(N) % npix)//(sc.nxr*sc.nyr)
    want, _ = sref.surface_scores(sc, st.astype(np.float64), d.astype(np.float64))
    r32 = _history32(sc, st, d)
    gap32 = np.abs(r32/want-1.0).max()
    gap = np.abs(score/want-1.0)
    print('single histories, Src_the %g: %d lines; float32 restatement: largest relative gap to float64 %.3e; the kernel: %.3e (allowed %.3e)'
          % (the, N, gap32, gap.max(), 4.0*gap32))
    assert all(((iv == v) & (want > 0.0)).sum() >= 500 for v in range(sc.nview)) and sc.nview == 2
    assert gap.max() <= 4.0*gap32, (gap.max(), gap32, int(np.argmax(gap)))


# ---- 2: Src_fsol = 0 is the thermal job ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('chunk', [0, 16])
@pytest.mark.parametrize('qmax', [0.0, 0.533])
def test_no_sunlight_is_the_thermal_job_bit_for_bit(solver, qmax, chunk):
    sc = sref.scattering_sunlit(140.0, 30.0, 0.0, qmax=qmax)
    npix = sc.nview*sc.nxr*sc.nyr
    N = 300*npix+17
    a = _raw(solver, sref.thermal_twin(sc), [(5, N)], 71, chunk, PLAIN)
    b = _raw(solver, sc, [(5, N)], 71, chunk, SUN)
    assert a.min() > 0.0 and np.array_equal(a, b), np.abs(b/a-1.0).max()


# ---- 3: linearity on the same ids ------------------------------------------------------------------------------------------------------------

def test_radiance_is_affine_in_the_solar_irradiance(solver):
    """rad(2F) - rad(0) = 2 (rad(F) - rad(0)) on the same ids, to the rounding of the float64 tallies.  A history's float32 terms are the
    thermal ones, the same under every F, and the sun's, each g T F with g and T free of F: doubling F doubles the term exactly, and whether
    a ray is flown, and how far, is decided on g alone.  What is left is the rounding of float64 sums: a history adds at most 2^20 + 2^20
    terms (its cell steps and events: kBwdMaxCells), a pixel its n histories, each sum good to (number of addends) x 2^-53 of the sum of its
    (positive) addends; the three tallies enter with weights 1, 2 and 1 (+ 2 for rad(0))"""
    F = 10.0
    base = sref.scattering_sunlit(140.0, 30.0, F, omgp=0.9)
    npix = base.nview*base.nxr*base.nyr
    n = 400
    N = n*npix
    T = {}
    for k in (0.0, 1.0, 2.0):
        T[k] = _raw(solver, dataclasses.replace(base, src_fsol=k*F), [(0, N)], 73, 16, SUN)
    rounding = (2.0**21+n+1)*2.0**-53*(T[2.0]+2.0*T[1.0]+3.0*T[0.0])
    lhs, rhs = T[2.0]-T[0.0], 2.0*(T[1.0]-T[0.0])
    print('linearity: %d pixels, %d histories each; largest |lhs - rhs| %.3e (allowed: rounding, from %.3e); solar share %.2f'
          % (npix, n, np.abs(lhs-rhs).max(), rounding.min(), (lhs/T[2.0]).mean()))
    assert T[0.0].min() > 0.0 and np.all(lhs > 0.05*T[2.0])                # (both sources matter)
    assert np.all(np.abs(lhs-rhs) <= rounding), np.abs(lhs-rhs).max()


# ---- 4: multiple anisotropic scattering against K16 --------------------------------------------------------------------------------------------

def test_multiple_scattering_against_k16(solver):
    """the gridded 16 x 16 x 4 slabs of tests/test_k16.py's ORACLE_CASES as solar+thermal jobs of a cold atmosphere (20 K: nothing emits) with
    F = 1 -- K16's radiance is per unit irradiance normal to the beam --, all twelve views, image means over 16 batches, held by compare and
    check_group as they stand.  2048 histories a pixel and batch, 8.4e6 a view in all, for a relative se below 3e-3 (printed): 512 gave 3.4e-3
    at worst, the view 26 degrees off the zenith over the thick conservative cloud"""
    rows = []
    nb, per_pixel = 16, 2048
    for g, omega, tau, mu0, albedo, tau_ray, _ in ORACLE_CASES:
        want = k16_answer(g, omega, tau, mu0, albedo, tau_ray)
        sc = slab(g, omega, tau, mu0, albedo, tau_ray, grid=True)
        sc = dataclasses.replace(sc, src_mtype=2, src_fsol=1.0, src_wlen=sref.WL, tmp1d=np.full(sc.zgrd.size, sref.COLD), view_method=1, view_sunlight=1)
        assert sc.nview == 12 and (sc.nz3, sc.ny, sc.nx) == (4, 16, 16)
        npix = sc.nview*sc.nxr*sc.nyr
        _, _, a = batches(solver, sc, nb, per_pixel*npix, 16)
        m = a.mean(axis=(2, 3))                                       # (nb, nview)
        mean, se = m.mean(axis=0), m.std(axis=0, ddof=1)/np.sqrt(nb)
        print('K16 g %g omega %g tau %g mu0 %g albedo %g tau_ray %g: relative se of the view means from %.2e to %.2e; largest relative gap %.2e'
              % (g, omega, tau, mu0, albedo, tau_ray, (se/mean).min(), (se/mean).max(), np.abs(mean/want['radiance']-1.0).max()))
        assert (se/mean).max() < 3.0e-3
        compare((g, omega, tau, mu0, albedo, tau_ray), mean, se, want['radiance'], rows)
    check_group(rows, 'backward views with sunlight, voxel grid')


# ---- 5: a 3-D cloud against the oracle's sum ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('qmax', [0.0, 0.533])
def test_cloud_against_the_oracles_forward_sum(solver, oracle, nthreads, qmax):
    """the checkerboard cloud at 3.75 um, omega = 0.9, the sun 40 degrees from the zenith, F = 10: the oracle has no source 2, so the reference
    is F x solar + thermal of its forward runs, 32 batches of 125000 photons each, summed batch by batch as tests/test_gpu_source_mix.py sums
    them; the criteria of tests/test_gpu_backward_views.py::test_scattering_against_the_oracles_forward_image"""
    F = 10.0
    sc = sref.scattering_sunlit(140.0, 30.0, F, qmax=qmax, omgp=0.9)
    th = dataclasses.replace(sc, src_mtype=3, src_fsol=None, view_method=0, view_sunlight=0)
    so = dataclasses.replace(th, src_mtype=1)
    runs, sol_share = [], []
    for b in range(32):
        rs = oracle.run(so, 125000, seed=2101, offset=b*125000, nthreads=nthreads)['rad'].astype(np.float64)
        rt = oracle.run(th, 125000, seed=2102, offset=b*125000, nthreads=nthreads)['rad'].astype(np.float64)
        runs.append(F*rs+rt); sol_share.append((F*rs).mean()/(F*rs+rt).mean())
    runs = np.array(runs)
    mf, sf = runs.mean(axis=0), runs.std(axis=0, ddof=1)/np.sqrt(32.0)
    solver.set_tuning(bwd_chunk=16)
    mb, sb, _ = batches(solver, sc, 16, 2000*72, 89)
    z = ((mb-mf)/np.sqrt(sb**2+sf**2)).ravel()
    M = z.size
    print('cloud, Src_qmax %g: %d pixels; solar share %.2f; se / value: backward %.4f, oracle sum %.4f (largest); max |z| %.2f, mean z %.3f (allowed %.3f)'
          % (qmax, M, np.mean(sol_share), (sb/mb).max(), (sf/mf).max(), np.abs(z).max(), z.mean(), 3.0/np.sqrt(M)))
    assert M == 72 and (sb/mb).max() < 0.02 and (sf/mf).max() < 0.02
    assert np.abs(z).max() < 4.5 and abs(z.mean()) < 3.0/np.sqrt(M), (np.abs(z).max(), z.mean())


# ---- 6: pixel errors ---------------------------------------------------------------------------------------------------------------------------

def test_pixel_errors_are_served(solver):
    """with mi3d_set_pixel_errors 1 the job runs the N,S build, its image is that of the run without, bit for bit, and se^2 is the variance of
    independent batch means: R = var(batch means) / mean(se^2) per pixel, |R - 1| <= 4 sqrt(2 / (M - 1)) + 0.1 with M = 16 batches under seeds
    of their own -- the criterion of tests/test_gpu_pixel_errors.py::test_se_squared_is_the_variance_of_independent_batch_means (its line
    `bound = 4.0*np.sqrt(2.0/(M-1))+0.1`), whose 0.1 allows for heavy tails"""
    sc = sref.scattering_sunlit(140.0, 30.0, 10.0, omgp=0.9)
    on = dataclasses.replace(sc, pixel_errors=1)
    npix = sc.nview*sc.nxr*sc.nyr
    M, n = 16, 1000
    N = n*npix
    solver.set_tuning(bwd_chunk=16)
    solver.load_scene(sc); solver.reset(); solver.run(N, seed=1000)
    plain = solver.radiance(N)
    assert solver.kernel_name() == SUN
    solver.load_scene(on)
    means, ses = [], []
    for b in range(M):
        solver.reset(); solver.run(N, seed=1000+b)
        means.append(solver.radiance(N)); ses.append(solver.radiance_se(N).astype(np.float64).ravel())
        assert solver.kernel_name() == SUN_ERR, solver.kernel_name()
    assert np.array_equal(means[0], plain)
    means, ses = np.array([m.astype(np.float64).ravel() for m in means]), np.array(ses)
    assert np.all(ses > 0.0) and np.all(np.isfinite(ses))
    R = means.var(axis=0, ddof=1)/(ses**2).mean(axis=0)
    bound = 4.0*np.sqrt(2.0/(M-1))+0.1
    print('pixel errors: R from %.3f to %.3f over %d pixels (allowed 1 +- %.3f); se / rad from %.2e to %.2e'
          % (R.min(), R.max(), npix, bound, (ses.mean(axis=0)/means.mean(axis=0)).min(), (ses.mean(axis=0)/means.mean(axis=0)).max()))
    assert np.all(np.abs(R-1.0) <= bound), R


# ---- 7: bookkeeping ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('chunk', [16, -1])
def test_raw_tallies_add_over_id_ranges(solver, chunk):
    """two id ranges against one.  Not np.array_equal: the same float64 scores are added by atomics whose order differs between one launch
    and two (and from run to run): sums of some 140 positive addends a pixel agree to 140 x 2^-53 = 1.6e-14, held here to 1e-12"""
    sc = sref.scattering_sunlit(140.0, 30.0, 10.0, qmax=0.533, omgp=0.9)
    npix = sc.nview*sc.nxr*sc.nyr
    N, n1 = 137*npix+21, 41*npix+9
    whole = _raw(solver, sc, [(0, N)], 67, chunk, SUN)
    parts = _raw(solver, sc, [(0, n1), (n1, N-n1)], 67, chunk, SUN)
    assert whole.min() > 0.0 and np.allclose(parts, whole, rtol=1.0e-12, atol=0.0), (parts/whole-1.0)


# ---- 8: refusals through the C-ABI -------------------------------------------------------------------------------------------------------------

def test_what_the_switch_does_not_serve_is_refused(solver):
    sc = dataclasses.replace(sref.scattering_sunlit(140.0, 30.0, 10.0), view_sunlight=0)      # (the switch is set by hand below)
    lsrt = dataclasses.replace(sc, sfc_mtype=4, sfc_param=np.array([0.1, 0.05, 0.02, 0, 0], dtype=np.float32))
    cams = dataclasses.replace(sc, view_method=0, rad_kind=1, view_the=[180.0], view_phi=[0.0], view_zloc=[500.0], nxr=2, nyr=2, cam_images=0)
    # (scene, view method, emission weights, view profiles, the refusal's word, is the refusal the switch's own?)
    cases = [(dataclasses.replace(sc, src_mtype=1), 1, 0, 0, 'Src_mtype=1', True),
             (dataclasses.replace(sc, src_mtype=3, src_fsol=None), 1, 0, 0, 'Src_mtype=3', True),
             (sc, 0, 0, 0, 'Rad_mvbwd=1', True),
             (cams, 1, 0, 0, 'Rad_mrkind=1', True),
             (sc, 1, 0, 1, 'view profiles', True),
             (sc, 1, 1, 0, 'emission weights', True),
             (dataclasses.replace(sc, src_the=90.2, src_qmax=0.533), 1, 0, 0, 'horizon', True),
             (dataclasses.replace(sc, target=TARGET_FLUX), 1, 0, 0, 'flux', False),
             (dataclasses.replace(sc, solver=1), 1, 0, 0, 'partial 3-D', False),
             (dataclasses.replace(sc, solver=2), 1, 0, 0, 'independent columns', False),
             (lsrt, 1, 0, 0, 'Lambertian', False)]
    lib = solver.lib
    for s, vm, wg, pf, word, own in cases:
        try:
            solver.load_scene(s)
        except OSError:
            pass                                             # (mi3d_prepare refuses the LSRT surface of a thermal job already)
        solver.set_view_method(vm); solver.set_emission_weights(wg); solver.set_view_profiles(pf); solver.set_view_sunlight(1)
        rc = lib.mi3d_run(solver._h, 1000, 1, 0)
        msg = lib.mi3d_last_error().decode()
        solver.set_emission_weights(0); solver.set_view_profiles(0)
        assert rc == -4 and word in msg, (word, rc, msg)
        assert not own or ('mi3d_set_view_sunlight 1' in msg and 'Rad_mvsun' in msg), (word, msg)
    assert lib.mi3d_set_view_sunlight(solver._h, 2) == -1 and lib.mi3d_set_view_sunlight(solver._h, -1) == -1
    for the in (90.0, 60.0):                                 # a sun on the horizon or from below: mi3d_set_source refuses it for every job
        with pytest.raises(OSError) as err:
            solver.load_scene(dataclasses.replace(sc, src_the=the))
        assert 'Src_the' in str(err.value)
    # the switch off: the mixed source is refused on the backward route in the words it always was
    solver.load_scene(sc); solver.set_view_sunlight(0)
    rc = lib.mi3d_run(solver._h, 1000, 1, 0)
    msg = lib.mi3d_last_error().decode()
    assert rc == -4 and 'solar+thermal' in msg and 'mi3d_set_view_method 1' in msg, msg
    # ... and on, it runs; off again on a thermal job, the plain build
    solver.set_view_sunlight(1); solver.reset(); solver.run(2000, seed=1)
    assert solver.kernel_name() == SUN and solver.radiance(2000).max() > 0.0
    solver.load_scene(sref.thermal_twin(sc)); solver.reset(); solver.run(2000, seed=1)
    assert solver.kernel_name() == PLAIN


# ---- 9: the drop-in ----------------------------------------------------------------------------------------------------------------------------

def test_dropin_files_against_fused_statistics(tmp_path):
    """mcarats_ng(source='solar+thermal', view_method='backward', view_sunlight=True) on the 12 x 10 x 10 synthetic cloud of
    tests/test_gpu_backward_views.py's drop-in test: the file route and the fused statistics under the same seeds, bit for bit; the key in
    the job file; bt above the thermal-only job's where the sun adds a fifth or more to the radiance"""
    import contextlib
    import copy
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(3750.0, atm, Ng=3)
    ab.coef['solar']['data'] = np.array([9.0, 10.0, 11.0])*1.0e-3          # W m-2 nm-1: about 10 W m-2 um-1, the size of the emission
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=3, target='radiance', surface_albedo=0.2, view_method='backward', Nrun=3, photons=6e4,
                  weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True,
                  solar_zenith_angle=40.0, solar_azimuth_angle=30.0, sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
        mix = dict(kw, source='solar+thermal', view_sunlight=True, abs_obj=ab)
        np.random.seed(7)                                    # (mcarats_ng shuffles the seeds over its jobs)
        files = mca.mcarats_ng(fdir=str(tmp_path/'files'), **mix)
        files = copy.copy(files); files.fused = None         # (a mixed job needs abs_obj for its irradiance: the file route is read from the files)
        name = get_runner().sol.kernel_name()
        np.random.seed(7)
        fused = mca.mcarats_ng(fdir=str(tmp_path/'fused'), keep_files=False, **mix)
        np.random.seed(7)
        thm = mca.mcarats_ng(fdir=str(tmp_path/'thm'), source='thermal', **kw)
    assert name == SUN and get_runner().sol.debug_backward_views(1, 0, 0)[3] == 0
    assert fused.fused is not None and files.fused is None
    nml = mca.mca_inp_read(files.fnames_inp[0][0])
    assert nml['Rad_mvsun'] == 1 and nml['Rad_mvbwd'] == 1 and nml['Rad_mrkind'] == 2 and nml['Src_mtype'] == 2
    assert 'Rad_mvsun' not in mca.mca_inp_read(thm.fnames_inp[0][0])
    assert [mca.mca_inp_read(f)['Wld_jseed'] for f in sum(files.fnames_inp, [])] == [mca.mca_inp_read(f)['Wld_jseed'] for f in sum(fused.fnames_inp, [])]
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=fused, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys()) and 'bt' in a
        for k in ('rad', 'bt'):
            assert a[k]['data'].shape == b[k]['data'].shape and a[k]['data'].shape[:3] == (12, 10, 2), (mode, k, a[k]['data'].shape)
            assert np.array_equal(a[k]['data'], b[k]['data']), (mode, k)
    b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    t = mca.mca_out_ng(mca_obj=thm, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    sunlit = b['rad']['data'] > 1.2*t['rad']['data']
    print('drop-in: %d of %d pixels with a solar share above a sixth; bt from %.1f to %.1f K, the thermal job\'s from %.1f to %.1f K'
          % (sunlit.sum(), sunlit.size, b['bt']['data'].min(), b['bt']['data'].max(), t['bt']['data'].min(), t['bt']['data'].max()))
    assert sunlit.sum() > sunlit.size//2 and np.all(b['bt']['data'][sunlit] > t['bt']['data'][sunlit])
