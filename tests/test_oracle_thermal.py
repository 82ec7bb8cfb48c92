"""
Pins the CPU oracle's thermal source (Src_mtype = 3) and its rectangular camera map (Rad_mpmap = 2, Rad_mrproj) on known answers,
before the GPU is held to it (tests/test_gpu_thermal_parity.py):
  * the CDF of the cells' emitted power against a numpy float64 restatement,
  * a non-scattering column over a grey surface: up and down flux at every level against the exact E3 sums, radiance from above
    and looking up (at the ground and inside a layer) against Schwarzschild's sums,
  * Kirchhoff: an isothermal scattering slab over a Lambert surface at the same temperature against K16's plane albedo,
  * a transparent atmosphere over a 2-D surface finer and coarser than the voxel grid: every pixel is its surface cells' emission,
  * a scene where nothing emits,
  * the rectangular map's pixel solid angles, and an isotropic radiance field seen as the same value in every pixel.
CPU only.
"""

import dataclasses

import numpy as np
import pytest
from scipy.special import expn

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE
from er3t_amd.thermal import planck
from tests import k16_adding_doubling as k16
from tests.test_gpu_thermal import column_1d
from tests.util import slab_scene, thermal_mixed_scene, thermal_powers_np

WL = 11.0
FLOOR = 3.0e-4


def obatches(oracle, scene, nb, nper, nthreads, seed=1):
    """nb batches of nper photons on consecutive id ranges: per-batch normalised radiance and flux"""
    rad, flux = [], []
    for b in range(nb):
        r = oracle.run(scene, nper, seed=seed, offset=b*nper, nthreads=nthreads)
        rad.append(r['rad']); flux.append(r['flux'])
    return np.array(rad), np.array(flux)


def zscore(x, want):
    """z of the batch mean of x (first axis: batches) against want, with a relative floor for float32 inputs"""
    m = x.mean(axis=0); se = x.std(axis=0, ddof=1)/np.sqrt(x.shape[0])
    return (m-want)/np.hypot(se, FLOOR*np.abs(want))


# ---------------------------------------------------------------------------------------------
def test_thermal_cdf_matches_a_numpy_restatement(oracle):
    for s in (thermal_mixed_scene(), column_1d(sfc_param=[0.3, 0, 0, 0, 0]),
              dataclasses.replace(thermal_mixed_scene(seed=3), iz3l=5, tmpa3d=None, tmps2d=None, abst=None)):
        cdf = oracle.thermal_cdf(s)
        want = np.cumsum(thermal_powers_np(s))
        assert cdf.shape == want.shape
        assert np.all(np.diff(cdf) >= 0.0) and cdf[-1] > 0.0
        assert np.max(np.abs(cdf-want)/want[-1]) < 1e-12, np.max(np.abs(cdf-want)/want[-1])
    with pytest.raises(ValueError):
        oracle.thermal_cdf(slab_scene())


def _column_sums(s, eps):
    """exact fluxes at every level and radiances of a non-scattering column over a grey Lambert surface (emissivity eps)"""
    t = s.tmp1d.astype(np.float64)
    B = planck(WL, 0.5*(t[:-1]+t[1:]))
    Bs = planck(WL, t[0])
    dtau = s.abs1d.astype(np.float32).astype(np.float64)*np.diff(s.zgrd)
    tl = np.concatenate([[0.0], np.cumsum(dtau)])            # optical depth of every level above the surface
    nz = dtau.size
    fdn = np.zeros(nz+1); fup = np.zeros(nz+1)
    for i in range(nz+1):
        for k in range(i, nz):                                # layers above level i
            fdn[i] += np.pi*B[k]*2.0*(expn(3, tl[k]-tl[i])-expn(3, tl[k+1]-tl[i]))
    fup0 = np.pi*eps*Bs + (1.0-eps)*fdn[0]
    for i in range(nz+1):
        fup[i] = fup0*2.0*expn(3, tl[i])
        for k in range(0, i):                                 # layers below level i
            fup[i] += np.pi*B[k]*2.0*(expn(3, tl[i]-tl[k+1])-expn(3, tl[i]-tl[k]))
    return B, Bs, dtau, tl, fdn, fup, fup0


def _down_radiance(B, s, tl, z, mu):
    """radiance looking up at height z (cosine mu of the line of sight): emission of everything above z"""
    zg = np.asarray(s.zgrd, dtype=np.float64)
    dtau = np.diff(tl)
    kap = dtau/np.diff(zg)
    tz = np.interp(z, zg, tl)
    I = 0.0
    for k in range(B.size):
        lo, hi = max(zg[k], z), zg[k+1]
        if hi <= lo:
            continue
        a = tl[k] + kap[k]*(lo-zg[k]) - tz                   # optical depth from z to the part's bottom and top
        b = tl[k+1] - tz
        I += B[k]*(np.exp(-a/mu)-np.exp(-b/mu))
    return I


def test_non_scattering_column_over_a_grey_surface(oracle, nthreads):
    """up and down flux at every level, radiance from above at mu 1 and 0.5, and up-looking sensors at the ground and at a height
    inside a layer (a partial layer in the sum): the exact sums of a non-scattering atmosphere over a Lambert surface of albedo 0.3"""
    alb = 0.3
    s = column_1d(sfc_param=[alb, 0, 0, 0, 0], view_the=[180.0, 120.0, 0.0, 0.0, 60.0], view_phi=[0.0]*5,
                  view_zloc=[1.0e6, 1.0e6, 0.0, 2500.0, 2500.0])
    rad, flux = obatches(oracle, s, 10, 200000, nthreads, seed=3)
    B, Bs, dtau, tl, fdn, fup, fup0 = _column_sums(s, 1.0-alb)
    assert np.all(flux[:, 0] == 0.0)                          # no direct beam
    zd = zscore(flux[:, 1, :-1, 0, 0], fdn[:-1])
    zu = zscore(flux[:, 2, :, 0, 0], fup)
    assert np.all(np.abs(zd) < 4.0), zd                       # (the top level's downward flux is 0 on both sides)
    assert np.all(flux[:, 1, -1] == 0.0) and fdn[-1] == 0.0
    assert np.all(np.abs(zu) < 4.0), zu
    assert abs(fup[0]-fup0) < 1e-12*fup0
    ru = rad[:, :, 0, 0]
    for iv, mu in enumerate((1.0, 0.5)):
        want = float(np.sum(B*(-np.expm1(-dtau/mu))*np.exp(-(tl[-1]-tl[1:])/mu))) + (fup0/np.pi)*np.exp(-tl[-1]/mu)
        assert abs(zscore(ru[:, iv], want)) < 4.0, (mu, ru[:, iv].mean(), want)
    for iv, z, mu in ((2, 0.0, 1.0), (3, 2500.0, 1.0), (4, 2500.0, 0.5)):
        want = _down_radiance(B, s, tl, z, mu)
        assert abs(zscore(ru[:, iv], want)) < 4.0, (z, mu, ru[:, iv].mean(), want)


def test_kirchhoff_isothermal_scattering_slab(oracle, nthreads):
    """isothermal HG cloud (tau 2, omega 0.9) over a Lambert surface at the same temperature: I_up(mu) = B (1 - r(mu)), r the plane
    albedo of K16 for incidence mu"""
    nz, dz, tau, g, omega, albedo, T = 4, 500.0, 2.0, 0.85, 0.9, 0.2, 280.0
    s = column_1d(nz=nz, dz=dz, target=TARGET_RADIANCE, abs1d=np.zeros(nz), ext1d=np.full(nz, tau/(nz*dz)), omg1d=np.full(nz, omega),
                  apf1d=np.full(nz, g), sfc_param=[albedo, 0, 0, 0, 0], tmp1d=np.full(nz+1, T),
                  view_the=[180.0, 120.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6])
    rad, _ = obatches(oracle, s, 8, 100000, nthreads, seed=7)
    for iv, mu in enumerate((1.0, 0.5)):
        r = k16.solve([(tau, omega, k16.hg_moments(g, 95))], mu, albedo=albedo)['albedo']
        want = planck(WL, T)*(1.0-r)
        assert abs(zscore(rad[:, iv, 0, 0], want)) < 4.0, (mu, rad[:, iv, 0, 0].mean(), want)


@pytest.mark.parametrize('nb', [8, 2])
def test_transparent_atmosphere_over_a_2d_surface(oracle, nthreads, nb):
    """nothing but a 2-D surface emits (nb x nb cells under 4 x 4 columns: finer and coarser): the nadir radiance of every pixel is
    the area-weighted eps B(Ts) of the surface cells under it, its upward flux at level 0 pi times that; the domain mean of the upward
    flux is the same at every level"""
    nx = 4
    rng = np.random.default_rng(nb)
    alb = rng.uniform(0.0, 0.5, (nb, nb)); tmps = rng.uniform(-15.0, 15.0, (nb, nb))
    psfc = np.zeros((5, nb, nb)); psfc[0] = alb
    s = column_1d(nz=3, nx=nx, ny=nx, abs1d=np.zeros(3), jsfc=np.ones((nb, nb)), psfc=psfc, tmps2d=tmps,
                  view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6])
    rad, flux = obatches(oracle, s, 8, 20000, nthreads, seed=11)
    e = (1.0-psfc[0].astype(np.float32))*planck(WL, s.tmp1d[0].astype(np.float64)+tmps.astype(np.float32))
    fine = np.kron(e, np.ones((nx, nx)))                      # both grids onto a common one of nx * nb cells a side
    want = fine.reshape(nx, nb, nx, nb).mean(axis=(1, 3))
    z = zscore(rad[:, 0], want)
    assert np.all(np.abs(z) < 4.0), z
    assert np.all(np.abs(zscore(flux[:, 2, 0], np.pi*want)) < 4.0)
    for lev in range(s.nz+1):
        assert abs(zscore(flux[:, 2, lev].mean(axis=(1, 2)), np.pi*want.mean())) < 4.0, lev
    assert np.all(flux[:, :2] == 0.0)


def test_nothing_emits(oracle, nthreads):
    """no absorption anywhere and a white surface: P_tot = 0, every tally exactly 0 and finite"""
    s = column_1d(abs1d=np.zeros(10), sfc_param=[1.0, 0, 0, 0, 0])
    assert oracle.thermal_cdf(s)[-1] == 0.0
    r = oracle.run(s, 1000, seed=1, nthreads=nthreads)
    assert np.all(r['rad'] == 0.0) and np.all(r['flux'] == 0.0)


def test_thermal_jobs_refuse_cameras_and_heating_rates(oracle):
    s = column_1d(target=TARGET_FLUX | 4)
    with pytest.raises(OSError):
        oracle.run(s, 10)
    cam = dataclasses.replace(column_1d(target=TARGET_RADIANCE, view_the=[0.0], view_phi=[0.0], view_zloc=[10.0]), rad_kind=1,
                              cam_xpos=[0.5], cam_ypos=[0.5], cam_psi=[0.0], cam_qmax=[180.0], cam_umax=[90.0], cam_vmax=[180.0],
                              cam_apsize=[0.05], cam_mpmap=2, cam_mrproj=1)
    with pytest.raises(OSError):
        oracle.run(cam, 10)


# ---------------------------------------------------------------------------------------------
def camera_scene(base, the, zloc, nxr, nyr, umax=90.0, vmax=180.0, mrproj=1, mpmap=2, phi=0.0, psi=0.0, xpos=0.5, ypos=0.5):
    return dataclasses.replace(base, target=TARGET_RADIANCE, rad_kind=1, view_the=[the], view_phi=[phi], view_zloc=[zloc],
                               cam_xpos=[xpos], cam_ypos=[ypos], cam_psi=[psi], cam_qmax=[180.0], cam_umax=[umax], cam_vmax=[vmax],
                               cam_apsize=[0.05], nxr=nxr, nyr=nyr, cam_mpmap=mpmap, cam_mrproj=mrproj)


@pytest.mark.parametrize('mrproj, hemi', [(0, 2.0*np.pi), (1, np.pi)])
def test_rectangular_pixels_tile_the_hemisphere(oracle, mrproj, hemi):
    s = camera_scene(slab_scene(), 0.0, 10.0, 9, 36, mrproj=mrproj)
    w = oracle.rect_pixel_w(s, 0)
    assert abs(w.sum()*s.nyr/hemi-1.0) < 1e-12
    t = np.radians(90.0)*np.arange(10)/9
    want = (np.cos(t[:-1])-np.cos(t[1:])) if mrproj == 0 else 0.5*(np.sin(t[1:])**2-np.sin(t[:-1])**2)
    assert np.allclose(w, want*2.0*np.pi/36, rtol=1e-13, atol=0.0)


@pytest.mark.parametrize('mrproj', [0, 1])
def test_rectangular_binning_keeps_every_contribution(oracle, nthreads, mrproj):
    """the same histories binned into 1 x 1 and 6 x 8 hemisphere pixels (looking up, and tilted): sum(value W) is one number"""
    base = slab_scene(tau=0.5, omega=0.9, apf=-1.0, albedo=0.3, nz=4, nx=2, ny=2, nz3=1, dx=20000.0, dy=20000.0, target=TARGET_RADIANCE)
    for the, phi, psi in ((0.0, 0.0, 0.0), (25.0, 60.0, 30.0)):
        one = oracle.run(camera_scene(base, the, 1.0, 1, 1, mrproj=mrproj, phi=phi, psi=psi), 20000, seed=5, nthreads=nthreads)['rad']
        sc = camera_scene(base, the, 1.0, 6, 8, mrproj=mrproj, phi=phi, psi=psi)
        img = oracle.run(sc, 20000, seed=5, nthreads=nthreads)['rad']
        w = oracle.rect_pixel_w(sc, 0)[None, :]
        assert np.count_nonzero(img) > 30
        a, b = (img[0]*w).sum(), one[0, 0, 0]*oracle.rect_pixel_w(camera_scene(base, the, 1.0, 1, 1, mrproj=mrproj), 0)[0]
        assert a > 0.0 and abs(a/b-1.0) < 1e-9, (the, a, b)


@pytest.mark.parametrize('mrproj', [0, 1])
def test_isotropic_field_is_flat_in_every_pixel(oracle, nthreads, mrproj):
    """the sun at zenith on a white Lambert plane under a vacuum: the reflected radiance is 1/pi in every upward direction, and
    every pixel of a down-looking rectangular image (6 x 8, theta up to 60) holds 1/pi for both weightings"""
    base = slab_scene(tau=0.0, omega=1.0, albedo=1.0, sza=0.0, nz=2, nx=1, ny=1, dx=2000.0, dy=2000.0, target=TARGET_RADIANCE)
    sc = camera_scene(base, 180.0, 200.0, 6, 8, umax=60.0, mrproj=mrproj)
    imgs = np.array([oracle.run(sc, 100000, seed=3, offset=b*100000, nthreads=nthreads)['rad'][0] for b in range(8)])
    z = zscore(imgs, np.full(imgs.shape[1:], 1.0/np.pi))
    assert np.all(np.abs(z) < 4.0), z
    assert abs(imgs.mean()*np.pi-1.0) < 0.01, imgs.mean()*np.pi
