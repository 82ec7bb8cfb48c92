"""
Thermal source (Src_mtype = 3) on the GPU against references that do not come from the oracle (which has no thermal source):
the Schwarzschild solution of a non-scattering atmosphere, Kirchhoff's law with K16's plane albedo (tests/k16_adding_doubling.py)
and with the solver's own solar albedo of the same 3-D scene, and the drop-in route through mcarats_ng + mca_out_ng.

Tolerances: 3 sigma of the batch statistics plus a relative floor of 3e-4 (float32 tallies and inputs).
"""

import dataclasses
import os

import numpy as np
import pytest
from scipy.special import expn

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE
from er3t_amd.thermal import planck
from tests import k16_adding_doubling as k16

WL = 11.0     # um
FLOOR = 3.0e-4


def batches(sol, scene, nb, nper, seed=1):
    """nb independent batches of nper photons: per-batch radiance and flux fields"""
    sol.load_scene(scene)
    rad, flux = [], []
    for b in range(nb):
        sol.reset()
        sol.run(nper, seed=seed, offset=b*nper)
        if scene.target & TARGET_RADIANCE:
            rad.append(sol.radiance(nper).astype(np.float64))
        if scene.target & TARGET_FLUX:
            flux.append(sol.flux(nper).astype(np.float64))
    return np.array(rad), np.array(flux)


def close(got, sig, want):
    return abs(got - want) <= 3.0*sig + FLOOR*abs(want)


def schwarzschild(B_lay, dtau, B_sfc, mu, eps=1.0):
    """radiance leaving the top of a non-scattering atmosphere at cosine mu; layers from the surface up"""
    tau_above = np.concatenate([np.cumsum(dtau[::-1])[::-1][1:], [0.0]])
    return float(np.sum(B_lay*(-np.expm1(-dtau/mu))*np.exp(-tau_above/mu)) + eps*B_sfc*np.exp(-dtau.sum()/mu))


def column_1d(nz=10, dz=1000.0, t_sfc=295.0, t_top=215.0, nx=1, ny=1, dx=1.0e4, target=TARGET_RADIANCE | TARGET_FLUX, **kw):
    zgrd = np.arange(nz+1)*dz
    absk = 1.0e-4*np.exp(-np.arange(nz)/3.0)          # 0.1 per km at the surface, falling off upwards
    tlev = np.linspace(t_sfc, t_top, nz+1)
    base = dict(zgrd=zgrd, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=nx, ny=ny, dx=dx, dy=dx,
                sfc_mtype=1, sfc_param=[0.0, 0, 0, 0, 0], target=target, view_the=[180.0, 120.0], view_phi=[0.0, 0.0],
                view_zloc=[1.0e6, 1.0e6], nxr=nx, nyr=ny, src_mtype=3, src_wlen=WL, tmp1d=tlev, src_the=180.0, src_qmax=0.0)
    base.update(kw)
    return Scene(**base)


@pytest.mark.gpu
def test_non_scattering_1d_matches_schwarzschild(solver):
    """nadir and 60 degree radiance, TOA upward and surface downward flux of a non-scattering column over a black surface"""
    s = column_1d()
    rad, flux = batches(solver, s, 16, 1000000, seed=3)
    assert solver.kernel_name().startswith('k_transport<') and 'thermal' in solver.kernel_name(), solver.kernel_name()
    t = s.tmp1d.astype(np.float64)
    B_lay = planck(WL, 0.5*(t[:-1]+t[1:]))
    dtau = s.abs1d.astype(np.float64)*np.diff(s.zgrd)
    B_s = planck(WL, t[0])
    for iv, mu in enumerate((1.0, 0.5)):
        want = schwarzschild(B_lay, dtau, B_s, mu)
        got = rad[:, iv].mean(axis=(1, 2))
        assert close(got.mean(), got.std(ddof=1)/np.sqrt(len(got)), want), (mu, got.mean(), want)
    tau_above = np.concatenate([np.cumsum(dtau[::-1])[::-1][1:], [0.0]])
    tau_below = np.concatenate([[0.0], np.cumsum(dtau)[:-1]])
    f_up = np.sum(np.pi*B_lay*2.0*(expn(3, tau_above)-expn(3, tau_above+dtau))) + np.pi*B_s*2.0*expn(3, dtau.sum())
    f_dn = np.sum(np.pi*B_lay*2.0*(expn(3, tau_below)-expn(3, tau_below+dtau)))
    up = flux[:, 2, -1].mean(axis=(1, 2)); dn = flux[:, 1, 0].mean(axis=(1, 2))
    assert close(up.mean(), up.std(ddof=1)/np.sqrt(len(up)), f_up), (up.mean(), f_up)
    assert close(dn.mean(), dn.std(ddof=1)/np.sqrt(len(dn)), f_dn), (dn.mean(), f_dn)
    assert np.all(flux[:, 0] == 0.0)          # no direct beam


@pytest.mark.gpu
def test_non_scattering_3d_every_pixel_is_its_own_column(solver):
    """block fields of voxel absorption and temperature anomaly over a 2-D surface with temperature anomalies: the nadir radiance of
    every pixel is its own column's Schwarzschild sum"""
    nz, nx, dz, dx = 6, 32, 1000.0, 500.0
    iz3l, nz3 = 2, 4
    yy, xx = np.meshgrid(np.arange(nx), np.arange(nx), indexing='ij')
    blk = ((xx//4 + yy//4) % 2).astype(np.float64)                      # 4 x 4 column checkerboard
    kz = np.arange(nz3)[:, None, None]
    ka = (0.2e-3 + 0.6e-3*blk[None]*(kz % 2 == 0)).astype(np.float32)  # absorbing constituent, omega = 0
    tmpa = (8.0*blk[None] - 4.0*(kz == 1)).astype(np.float32)
    tmps = (6.0*(1.0-blk) - 3.0*(xx % 2)).astype(np.float32)
    s0 = column_1d(nz=nz, dz=dz, nx=nx, ny=nx, dx=dx, target=TARGET_RADIANCE, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6])
    s = dataclasses.replace(s0, nz3=nz3, iz3l=iz3l, extp=ka[None], omgp=np.zeros((1, nz3, nx, nx)), apfp=np.zeros((1, nz3, nx, nx)),
                            jsfc=np.ones((nx, nx)), psfc=np.zeros((5, nx, nx)), tmpa3d=tmpa, tmps2d=tmps)
    nb = 48
    rad, _ = batches(solver, s, nb, 2000000, seed=5)
    t = s.tmp1d.astype(np.float64)
    tmean = 0.5*(t[:-1]+t[1:])
    z = np.zeros((nx, nx))
    for j in range(nx):
        for i in range(nx):
            kcol = s.abs1d.astype(np.float64).copy()
            tcol = tmean.copy()
            kcol[iz3l-1:iz3l-1+nz3] += ka[:, j, i]
            tcol[iz3l-1:iz3l-1+nz3] += tmpa[:, j, i]
            want = schwarzschild(planck(WL, tcol), kcol*dz, planck(WL, t[0]+tmps[j, i]), 1.0)
            got = rad[:, 0, j, i]
            sig = got.std(ddof=1)/np.sqrt(nb)
            z[j, i] = (got.mean()-want)/np.hypot(sig, FLOOR*want)
    assert np.mean(np.abs(z) <= 3.0) >= 0.99, z
    assert abs(z.mean()) <= 0.2, z.mean()


@pytest.mark.gpu
@pytest.mark.parametrize('mu', [1.0, 0.5])
def test_scattering_1d_kirchhoff_against_k16(solver, mu):
    """isothermal cloud layer (HG g 0.85, omega 0.9, tau 2) over a Lambert surface at the same temperature: I_up(mu) = B (1 - r(mu))
    with r K16's plane albedo for incidence mu"""
    nz, dz, tau, g, omega, albedo, T = 4, 500.0, 2.0, 0.85, 0.9, 0.2, 280.0
    s = column_1d(nz=nz, dz=dz, target=TARGET_RADIANCE, abs1d=np.zeros(nz), ext1d=np.full(nz, tau/(nz*dz)), omg1d=np.full(nz, omega),
                  apf1d=np.full(nz, g), sfc_param=[albedo, 0, 0, 0, 0], tmp1d=np.full(nz+1, T),
                  view_the=[180.0 - np.rad2deg(np.arccos(mu))], view_phi=[0.0], view_zloc=[1.0e6])
    nb = 16
    rad, _ = batches(solver, s, nb, 2000000, seed=7)
    r = k16.solve([(tau, omega, k16.hg_moments(g, 95))], mu, albedo=albedo)['albedo']
    want = planck(WL, T)*(1.0-r)
    got = rad[:, 0].mean(axis=(1, 2))
    assert close(got.mean(), got.std(ddof=1)/np.sqrt(nb), want), (mu, got.mean(), want, r)


@pytest.mark.gpu
def test_scattering_3d_kirchhoff_domain_mean(solver):
    """isothermal synthetic cloud field on 64 x 64 columns: domain-mean nadir radiance = B (1 - A), A the solver's own domain-mean
    TOA albedo of the same scene with the sun at zenith"""
    from er3t_amd.synth import les_scene
    T = 270.0
    s0 = les_scene(nx=64, ny=64, nz3=20)
    absk = np.full(s0.nz, 2.0e-5, dtype=np.float32)
    s1 = dataclasses.replace(s0, abs1d=absk, omgp=(s0.omgp*np.float32(0.97)), sfc_mtype=1, sfc_param=[0.1, 0, 0, 0, 0], jsfc=None, psfc=None,
                             src_the=180.0, src_qmax=0.0, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=64, nyr=64)
    nb = 12
    sol_s = dataclasses.replace(s1, target=TARGET_FLUX)
    _, flux = batches(solver, sol_s, nb, 2000000, seed=9)
    A = flux[:, 2, -1].mean(axis=(1, 2))
    th = dataclasses.replace(s1, target=TARGET_RADIANCE, src_mtype=3, src_wlen=WL, tmp1d=np.full(s0.nz+1, T))
    rad, _ = batches(solver, th, nb, 2000000, seed=10)
    got = rad[:, 0].mean(axis=(1, 2))
    B = planck(WL, T)
    want = B*(1.0-A.mean())
    sig = np.hypot(got.std(ddof=1), B*A.std(ddof=1))/np.sqrt(nb)
    assert close(got.mean(), sig, want), (got.mean(), want, A.mean())


@pytest.mark.gpu
def test_end_to_end_11um_through_mcarats_ng_and_mca_out_ng(tmp_path):
    """an 11 um window image of the synthetic cloud through the drop-in: the fused statistics equal the file route bit for bit,
    the brightness temperature lies within the scene's temperatures, and the general kernel serves the jobs with its thermal mark"""
    import contextlib
    import copy
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=4)
    cld = cld_synth(atm, nx=16, ny=12, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=4, target='radiance', surface_albedo=0.02, source='thermal',
                           fdir=str(tmp_path/'thermal'), Nrun=3, photons=4e5, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py',
                           overwrite=True, date=gin.DATE, quiet=True, abs_obj=ab, keep_files=True)
    name = get_runner().sol.kernel_name()
    assert name.startswith('k_transport<') and 'thermal' in name, name
    assert m.fused is not None and all(os.path.exists(f) for row in m.fnames_out for f in row)
    files = copy.copy(m); files.fused = None
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys())
        for k in ['rad', 'bt'] + (['rad_std'] if mode == 'mean' else []):
            assert np.array_equal(a[k]['data'], b[k]['data']), (mode, k)
    bt = a['bt']['data']
    tlev = atm.lev['temperature']['data']
    assert np.all(np.isfinite(bt)) and bt.min() >= tlev.min() and bt.max() <= tlev.max(), (bt.min(), bt.max())
