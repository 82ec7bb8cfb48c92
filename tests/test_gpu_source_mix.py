"""
Solar+thermal source (Src_mtype = 2) on the GPU.  A mixed result is linear in its two sources -- Src_flx x (thermal +
Src_fsol x solar per unit irradiance) --, so the references are closed forms of a non-scattering column (Schwarzschild's solution plus the
attenuated beam reflected by a Lambert surface), the thermal job itself (Src_fsol = 0 walks its histories id for id), and the CPU oracle's
solar (1) and thermal (3) runs summed; the oracle has no source 2.

Tolerances: `close` of tests/test_gpu_thermal.py, |got - want| <= 3 se + 3e-4 |want|, se the standard error over batches; against an oracle
sum se^2 = se_gpu^2 + Src_fsol^2 se_solar^2 + se_thermal^2.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import expn

from er3t_amd.scene import TARGET_FLUX, TARGET_HEAT, TARGET_RADIANCE, SOLVER_3D, SOLVER_IPA, SOLVER_P3D
from er3t_amd.thermal import planck
from tests.test_gpu_thermal import column_1d, schwarzschild, batches, close, FLOOR
from tests.test_gpu_thermal_heating import cloud_scene, layer_means, column_fnet

pytestmark = pytest.mark.gpu

WL = 3.75          # um
FSOL = 10.0        # W m-2 um-1
THE = 140.0        # Src_the: the sun 40 degrees from the zenith
MU0 = abs(np.cos(np.deg2rad(THE)))
FH = TARGET_FLUX | TARGET_HEAT


def mix_column(**kw):
    base = dict(nz=6, src_wlen=WL, sfc_param=[0.3, 0, 0, 0, 0], src_mtype=2, src_fsol=FSOL, src_the=THE)
    base.update(kw)
    return column_1d(**base)


def se_of(x):
    return x.std(axis=0, ddof=1)/np.sqrt(len(x))


def column_closed_form(B_lay, dtau, B_s, albedo, fsol, mu0):
    """a non-scattering column over a Lambert surface of albedo a, emission and an attenuated solar beam: direct-down flux at the nz+1
    levels, diffuse-down flux at the surface, the radiance the surface leaves with, up flux at the top, net upward flux at every level"""
    tau = dtau.sum()
    tau_above_lev = np.concatenate([np.cumsum(dtau[::-1])[::-1], [0.0]])            # optical depth above each of the nz+1 levels
    tau_below = np.concatenate([[0.0], np.cumsum(dtau)[:-1]])
    tau_above = tau_above_lev[1:]
    direct = fsol*mu0*np.exp(-tau_above_lev/mu0)
    f_dn = np.sum(np.pi*B_lay*2.0*(expn(3, tau_below)-expn(3, tau_below+dtau)))
    # what leaves the surface is isotropic: emission eps B_s plus the reflected downward flux, (a / pi) (F_dn + direct)
    I_sfc = (1.0-albedo)*B_s + albedo/np.pi*(f_dn + direct[0])
    f_up_top = np.sum(np.pi*B_lay*2.0*(expn(3, tau_above)-expn(3, tau_above+dtau))) + np.pi*I_sfc*2.0*expn(3, tau)
    fnet = column_fnet(B_lay, dtau, I_sfc) - direct                                  # (column_fnet's surface term is pi B 2 E3: B -> I_sfc)
    return dict(direct=direct, f_dn=f_dn, I_sfc=I_sfc, f_up_top=f_up_top, fnet=fnet, tau=tau)


def column_radiance(B_lay, dtau, B_s, albedo, fsol, mu0, mu):
    c = column_closed_form(B_lay, dtau, B_s, albedo, fsol, mu0)
    return (schwarzschild(B_lay, dtau, B_s, mu, eps=1.0-albedo) + albedo/np.pi*c['f_dn']*np.exp(-c['tau']/mu)
            + fsol*albedo/np.pi*mu0*np.exp(-c['tau']/mu0)*np.exp(-c['tau']/mu))


# ---- 1: a non-scattering column, both closed forms ---------------------------------------------------------------------------------------

def test_non_scattering_column_matches_both_closed_forms(solver, oracle):
    s = mix_column()
    rad, flux = batches(solver, s, 16, 1000000, seed=3)
    name = solver.kernel_name()
    assert name.startswith('k_transport<') and 'solar+thermal' in name, name
    t = s.tmp1d.astype(np.float64)
    B_lay = planck(WL, 0.5*(t[:-1]+t[1:]))
    dtau = s.abs1d.astype(np.float64)*np.diff(s.zgrd)
    B_s, a = planck(WL, t[0]), 0.3
    c = column_closed_form(B_lay, dtau, B_s, a, FSOL, MU0)
    # (the figures the issue records for this column: thermal 0.23419, solar per unit irradiance 0.036209, sums 0.59628 and 0.46958)
    assert abs(column_radiance(B_lay, dtau, B_s, a, 0.0, MU0, 1.0) - 0.23419) < 1.0e-5
    assert abs(column_radiance(B_lay, dtau, B_s, a, FSOL, MU0, 1.0) - 0.59628) < 1.0e-5
    assert abs(column_radiance(B_lay, dtau, B_s, a, FSOL, MU0, 0.5) - 0.46958) < 1.0e-5
    for iv, mu in enumerate((1.0, 0.5)):
        want = column_radiance(B_lay, dtau, B_s, a, FSOL, MU0, mu)
        got = rad[:, iv].mean(axis=(1, 2))
        print('radiance mu %.1f: got %.6f +- %.6f, want %.6f' % (mu, got.mean(), se_of(got), want))
        assert close(got.mean(), se_of(got), want), (mu, got.mean(), want)
    # the direct-down plane at every level, the top included, is Src_fsol mu0 exp(-tau_above / mu0): it pins the solar share
    d = flux[:, 0].mean(axis=(2, 3))
    for L in range(s.nz+1):
        print('direct-down level %d: got %.6f +- %.6f, want %.6f' % (L, d[:, L].mean(), se_of(d[:, L]), c['direct'][L]))
        assert close(d[:, L].mean(), se_of(d[:, L]), c['direct'][L]), (L, d[:, L].mean(), c['direct'][L])
    dn = flux[:, 1, 0].mean(axis=(1, 2)); up = flux[:, 2, -1].mean(axis=(1, 2))
    assert close(dn.mean(), se_of(dn), c['direct'][0] + c['f_dn']), (dn.mean(), c['direct'][0] + c['f_dn'])
    assert close(up.mean(), se_of(up), c['f_up_top']), (up.mean(), c['f_up_top'])
    ptot, psol = solver.source_power()
    want_ptot = oracle.thermal_cdf(dataclasses.replace(s, src_mtype=3, src_fsol=None))[-1]
    want_psol = FSOL*MU0*(s.nx*s.dx)*(s.ny*s.dy)
    assert abs(ptot/want_ptot - 1.0) <= 1.0e-12 and abs(psol/want_psol - 1.0) <= 1.0e-12, (ptot, want_ptot, psol, want_psol)


# ---- 2: Src_fsol = 0 is the thermal job --------------------------------------------------------------------------------------------------

def _one_run(solver, scene, n, seed, offset):
    solver.bind(None, None, None); solver.load_scene(scene); solver.set_counting(True)
    solver.reset(); solver.run(n, seed=seed, offset=offset); solver.sync()
    out = {'counters': solver.counters(), 'name': solver.kernel_name()}
    if scene.target & TARGET_RADIANCE:
        out['rad'] = solver.radiance(n).astype(np.float64)
    if scene.target & TARGET_FLUX:
        out['flux'] = solver.flux(n).astype(np.float64)
    if scene.target & TARGET_HEAT:
        out['heat'] = solver.heating(n).astype(np.float64)
    solver.set_counting(False)
    return out


@pytest.mark.parametrize('which', ['column', 'cloud'])
@pytest.mark.parametrize('target', [TARGET_RADIANCE | TARGET_FLUX, FH])
def test_no_sunlight_is_the_thermal_job_id_for_id(solver, which, target):
    views = dict(view_the=[180.0, 120.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6])
    if which == 'column':
        th = column_1d(nz=6, src_wlen=WL, sfc_param=[0.3, 0, 0, 0, 0], target=target)
    else:
        th = cloud_scene(src_wlen=WL, target=target, nxr=16, nyr=16, **views)
    mx = dataclasses.replace(th, src_mtype=2, src_fsol=0.0, src_the=THE)
    n = 200000
    a = _one_run(solver, th, n, seed=41, offset=7000)
    b = _one_run(solver, mx, n, seed=41, offset=7000)
    assert '[thermal]' in a['name'] and '[solar+thermal]' in b['name']
    # (every counter of the histories; the sched_* and ticks_* entries count wave passes and clock ticks, which no two launches share)
    for key in ('photons', 'steps', 'steps3d', 'scatter', 'surface', 'le_rays', 'le_steps', 'le_steps3d', 'le_column', 'flux_tally',
                'roulette', 'killed', 'escaped', 'absorbed'):
        assert a['counters'][key] == b['counters'][key], key
    assert a['counters']['photons'] == n
    for key in ('rad', 'flux', 'heat'):
        if key in a:
            scale = np.abs(a[key]).max()
            assert scale > 0.0 and np.allclose(a[key], b[key], rtol=1.0e-6, atol=0.0), key


# ---- 3: nothing emits: the solar job, statistically --------------------------------------------------------------------------------------

def _slab(**kw):
    nz, dz, tau = 4, 500.0, 2.0
    base = dict(nz=nz, dz=dz, nx=8, ny=8, dx=500.0, abs1d=np.zeros(nz), ext1d=np.full(nz, tau/(nz*dz)), omg1d=np.ones(nz), apf1d=np.full(nz, 0.85),
                sfc_param=[1.0, 0, 0, 0, 0], src_wlen=WL, src_mtype=2, src_fsol=3.0, src_the=THE)
    base.update(kw)
    return column_1d(**base)


def test_a_source_that_only_shines_is_the_solar_job(solver, oracle, nthreads):
    s = _slab()
    rad, flux = batches(solver, s, 16, 200000, seed=5)
    assert 'solar+thermal' in solver.kernel_name()
    ptot, psol = solver.source_power()
    assert ptot == 0.0 and psol > 0.0
    so = dataclasses.replace(s, src_mtype=1, src_fsol=None)
    nbo, npo = 32, 12500       # (4e5 photons in 32 batches: a standard error from a handful of batches has a Student-t tail a 3-sigma bound does not allow for)
    orad, oflux = [], []
    for b in range(nbo):
        r = oracle.run(so, npo, seed=1005, offset=b*npo, nthreads=nthreads)
        orad.append(r['rad']); oflux.append(r['flux'])
    orad, oflux = 3.0*np.array(orad), 3.0*np.array(oflux)
    for iv in range(2):
        g, o = rad[:, iv].mean(axis=(1, 2)), orad[:, iv].mean(axis=(1, 2))
        print('view %d: GPU %.6f +- %.6f, 3 x oracle %.6f +- %.6f' % (iv, g.mean(), se_of(g), o.mean(), se_of(o)))
        assert close(g.mean(), np.hypot(se_of(g), se_of(o)), o.mean()), (iv, g.mean(), o.mean())
    gl, ol = flux.mean(axis=(3, 4)), oflux.mean(axis=(3, 4))                        # (batches, 3 planes, nz+1 levels)
    se = np.hypot(se_of(gl), se_of(ol))
    assert np.all(np.abs(gl.mean(axis=0)-ol.mean(axis=0)) <= 3.0*se + FLOOR*np.abs(ol.mean(axis=0))), (gl.mean(axis=0), ol.mean(axis=0), se)
    # neither source has any power: nothing runs
    dark = _slab(src_fsol=0.0)
    solver.load_scene(dark); solver.reset(); solver.run(100000, seed=1)
    assert np.all(solver.radiance(100000) == 0.0) and np.all(solver.flux(100000) == 0.0)
    assert 'nothing emits' in solver.kernel_name() and 'solar+thermal' in solver.kernel_name()


# ---- 4: the 3-D cloud scene against the oracle's sum -------------------------------------------------------------------------------------

VIEWS = dict(view_the=[180.0, 120.0], view_phi=[0.0, 30.0], view_zloc=[1.0e6, 1.0e6], nxr=16, nyr=16)


@pytest.fixture(scope='module')
def oracle_sum(oracle, nthreads):
    """the oracle's solar (per unit irradiance) and thermal runs of the cloud scene at 3.75 um, 4e5 photons per source in 32 batches of 12500,
    summed batch by batch as Src_fsol x solar + thermal: radiance (nb, nview, ny, nx) and flux planes (nb, 3, nz+1, ny, nx).  Computed once.
    Thirty-two batches as on the oracle side of tests/test_gpu_thermal_heating.py: the standard errors below are taken over them, and
    28 layers are held to 3 of them each."""
    th = cloud_scene(src_wlen=WL, src_the=THE, src_phi=0.0, target=TARGET_RADIANCE | TARGET_FLUX, **VIEWS)
    so = dataclasses.replace(th, src_mtype=1)
    nbo, npo = 32, 12500
    rad, flux = [], []
    for b in range(nbo):
        rs = oracle.run(so, npo, seed=2001, offset=b*npo, nthreads=nthreads)
        rt = oracle.run(th, npo, seed=2002, offset=b*npo, nthreads=nthreads)
        rad.append(FSOL*rs['rad'] + rt['rad']); flux.append(FSOL*rs['flux'] + rt['flux'])
    rad, flux = np.array(rad), np.array(flux)
    rad.setflags(write=False); flux.setflags(write=False)
    return rad, flux


def _mix_cloud(**kw):
    return cloud_scene(src_wlen=WL, src_mtype=2, src_fsol=FSOL, src_the=THE, src_phi=0.0, **kw)


def test_3d_cloud_scene_radiance_and_flux_match_the_oracles_sum(solver, oracle_sum):
    orad, oflux = oracle_sum
    s = _mix_cloud(target=TARGET_RADIANCE | TARGET_FLUX, **VIEWS)
    rad, flux = batches(solver, s, 32, 200000, seed=19)
    assert 'solar+thermal' in solver.kernel_name()
    for iv in range(2):
        g, o = rad[:, iv].mean(axis=(1, 2)), orad[:, iv].mean(axis=(1, 2))
        print('view %d: GPU %.6f +- %.6f, oracle sum %.6f +- %.6f' % (iv, g.mean(), se_of(g), o.mean(), se_of(o)))
        assert close(g.mean(), np.hypot(se_of(g), se_of(o)), o.mean()), (iv, g.mean(), o.mean())
    gl, ol = flux.mean(axis=(3, 4)), oflux.mean(axis=(3, 4))
    se = np.hypot(se_of(gl), se_of(ol))
    z = (gl.mean(axis=0)-ol.mean(axis=0))/np.maximum(se, 1e-300)
    print('flux planes, level means: largest |z| %.2f' % np.abs(z[np.isfinite(z)]).max())
    assert np.all(np.abs(gl.mean(axis=0)-ol.mean(axis=0)) <= 3.0*se + FLOOR*np.abs(ol.mean(axis=0))), z
    # the nadir image in 4 x 4 blocks, the criterion of tests/test_gpu_fullsize.py (bench.parity_stats): z of a block against sqrt(2) x the
    # oracle's standard error of it, |z| < 4 (one may reach 6), |mean z| < 0.5, std z < 1
    nbk = 4
    gb = rad[:, 0].reshape(len(rad), nbk, 16//nbk, nbk, 16//nbk).mean(axis=(2, 4))
    ob = orad[:, 0].reshape(len(orad), nbk, 16//nbk, nbk, 16//nbk).mean(axis=(2, 4))
    zb = ((gb.mean(axis=0)-ob.mean(axis=0))/(np.sqrt(2.0)*se_of(ob))).ravel()
    print('nadir blocks: z mean %+.3f, std %.3f, max |z| %.2f' % (zb.mean(), zb.std(), np.abs(zb).max()))
    assert np.sum(np.abs(zb) >= 4.0) <= 1 and np.abs(zb).max() < 6.0, zb
    assert abs(zb.mean()) < 0.5 and zb.std() < 1.0, (zb.mean(), zb.std())


@pytest.mark.parametrize('est', [0, 1])
def test_3d_cloud_scene_net_heating_matches_the_divergence_of_the_summed_oracle_fluxes(solver, oracle_sum, est):
    _, oflux = oracle_sum
    s = _mix_cloud(target=FH, heat_estimator=est)
    from tests.test_gpu_thermal_heating import batches as heat_batches
    nb = 32
    heat, flux = heat_batches(solver, s, nb, 200000, seed=23)
    name = solver.kernel_name()
    assert '[solar+thermal]' in name and ('[heating: path length]' in name) == bool(est), name
    dz = np.diff(s.zgrd)
    g = heat.mean(axis=(2, 3))*dz[None]                                             # (nb, nz)
    ofn = (oflux[:, 2]-oflux[:, 1]).mean(axis=(2, 3))
    div = ofn[:, :-1]-ofn[:, 1:]
    emitted = solver.emission().astype(np.float64).mean(axis=(1, 2))*dz            # the scale of the floor: the gross term of a layer
    z = (g.mean(axis=0)-div.mean(axis=0))/np.sqrt(se_of(g)**2 + se_of(div)**2 + (FLOOR*emitted)**2)
    print('estimator %d: layer z' % est, np.round(z, 2))
    assert np.mean(np.abs(z) <= 3.0) >= 0.99, z
    assert abs(z.mean()) <= 0.3, z.mean()
    # the job's own budget, batch by batch: sum net dz + (f_dn - f_up) at level 0 + (f_up - f_dn) at the top is 0
    fnet = (flux[:, 2]-flux[:, 1]).mean(axis=(2, 3))
    d = g.sum(axis=1) - fnet[:, 0] + fnet[:, -1]
    print('budget: %+.4e +- %.4e of %.4e absorbed and emitted' % (d.mean(), se_of(d), emitted.sum()))
    assert abs(d.mean()) <= 3.0*se_of(d) + FLOOR*emitted.sum(), (d.mean(), se_of(d))


# ---- 5: every column its own column (IPA; P3D with the sun overhead) ---------------------------------------------------------------------

@pytest.mark.parametrize('solver_id, the', [(SOLVER_IPA, THE), (SOLVER_P3D, 180.0)])
def test_checkerboard_every_column_matches_its_own_closed_form(solver, solver_id, the):
    """4 x 4 columns x 6 layers, two alternating absorption profiles with voxel temperatures +- 5 K, no scattering, albedo 0.3: under IPA
    (sun at 40 degrees) and under partial 3-D with the sun overhead every column is its own 1-D problem.  By `close`, per column: the nadir
    radiance against the closed form of test 1, and the column's net heating sum_k net_k dz_k against F_net(0) - F_net(top) of
    column_closed_form (column_net_heating with what the surface reflects, plus the absorbed beam); the vertical distribution layer by
    layer on the mean over the eight columns of either profile, which are the same problem eight times.  (Every one of the 96 cells held
    to 3 standard errors on its own is 96 + 16 three-sigma verdicts in one test: one false alarm in three runs of a correct code.  A run
    with sixteen times the photons, 32 batches of 8e6, showed no bias: relative deviations of the cells' net of 1e-4 ... 1e-3, each
    within its standard error's reach, mean z per layer -0.42 ... +0.19)"""
    nz, nx, dz, dx, a = 6, 4, 1000.0, 500.0, 0.3
    iz3l, nz3 = 2, 4
    mu0 = abs(np.cos(np.deg2rad(the)))
    yy, xx = np.meshgrid(np.arange(nx), np.arange(nx), indexing='ij')
    blk = ((xx + yy) % 2).astype(np.float64)
    kz = np.arange(nz3)[:, None, None]
    ka = (0.2e-3 + 0.6e-3*blk[None]*(kz % 2 == 0) + 0.3e-3*(1.0-blk[None])*(kz % 2 == 1)).astype(np.float32)   # two alternating profiles
    tmpa = np.broadcast_to((10.0*blk - 5.0)[None], (nz3, nx, nx)).astype(np.float32)                               # +- 5 K
    from tests.test_gpu_thermal_heating import batches as heat_batches
    base = mix_column(nz=nz, dz=dz, nx=nx, ny=nx, dx=dx, src_the=the, solver=solver_id, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6],
                      sfc_param=[a, 0, 0, 0, 0])
    vox = dict(nz3=nz3, iz3l=iz3l, extp=ka[None], omgp=np.zeros((1, nz3, nx, nx)), apfp=np.zeros((1, nz3, nx, nx)), tmpa3d=tmpa)
    nb, nper = 64, 250000      # (many batches: 16 + 96 values are held to 3 standard errors each, which must then be well estimated)
    rad, _ = batches(solver, dataclasses.replace(base, target=TARGET_RADIANCE, **vox), nb, nper, seed=7)
    assert 'solar+thermal' in solver.kernel_name()
    heat, _ = heat_batches(solver, dataclasses.replace(base, target=FH, **vox), nb, nper, seed=8)
    t = np.asarray(base.tmp1d, dtype=np.float32).astype(np.float64)
    tmean = 0.5*(t[:-1]+t[1:])
    want_r, want_h = np.zeros((nx, nx)), np.zeros((nz, nx, nx))
    for j in range(nx):
        for i in range(nx):
            kcol = np.asarray(base.abs1d, dtype=np.float32).astype(np.float64)
            tcol = tmean.copy()
            kcol[iz3l-1:iz3l-1+nz3] = (np.asarray(base.abs1d, dtype=np.float32)[iz3l-1:iz3l-1+nz3] + ka[:, j, i]).astype(np.float64)
            tcol[iz3l-1:iz3l-1+nz3] += tmpa[:, j, i]
            B_lay, dtau, B_s = planck(WL, tcol), kcol*dz, planck(WL, t[0])
            want_r[j, i] = column_radiance(B_lay, dtau, B_s, a, FSOL, mu0, 1.0)
            # net of a layer: the divergence of the net flux -- column_net_heating with the surface's reflected light, plus the absorbed beam
            f = column_closed_form(B_lay, dtau, B_s, a, FSOL, mu0)['fnet']
            want_h[:, j, i] = (f[:-1]-f[1:])/dz
    got_r, se_r = rad[:, 0].mean(axis=0), se_of(rad[:, 0])
    got_h, se_h = heat.mean(axis=0), se_of(heat)
    zr = (got_r-want_r)/np.hypot(se_r, FLOOR*want_r)
    zh = (got_h-want_h)/np.hypot(se_h, FLOOR*np.abs(want_h))
    print('radiance: z mean %+.3f, max |z| %.2f; heating: z mean %+.3f, max |z| %.2f, per layer mean z' % (zr.mean(), np.abs(zr).max(), zh.mean(), np.abs(zh).max()),
          np.round(zh.mean(axis=(1, 2)), 2))
    assert np.all(close(got_r, se_r, want_r)), ('radiance', zr)
    dzk = np.full(nz, dz)[None, :, None, None]
    col = (heat*dzk).sum(axis=1)                                                     # (nb, ny, nx): what the column's atmosphere gains
    want_c = (want_h*dzk[0]).sum(axis=0)
    zc = (col.mean(axis=0)-want_c)/np.hypot(se_of(col), FLOOR*np.abs(want_c))
    print('column net: z', np.round(zc, 2))
    assert np.all(close(col.mean(axis=0), se_of(col), want_c)), ('column net heating', zc)
    for b in (0, 1):
        m = blk == b
        lay = heat[:, :, m].mean(axis=2)                                             # (nb, nz): layer means over the columns of one profile
        want_l = want_h[:, m].mean(axis=1)
        zl = (lay.mean(axis=0)-want_l)/np.hypot(se_of(lay), FLOOR*np.abs(want_l))
        print('profile %d, layer means: z' % b, np.round(zl, 2))
        assert np.all(close(lay.mean(axis=0), se_of(lay), want_l)), ('layer means of profile %d' % b, zl)


# ---- 6: id ranges add --------------------------------------------------------------------------------------------------------------------

def test_id_ranges_add_and_the_emission_comes_off_once(solver):
    import torch
    s = _mix_cloud(target=FH)
    n = 200000
    dev = torch.device('cuda', solver.device)
    flux = torch.zeros(3*(s.nz+1)*s.ny*s.nx, dtype=torch.float64, device=dev)
    heat = torch.zeros(s.nz*s.ny*s.nx, dtype=torch.float64, device=dev)
    rad = torch.zeros(1, dtype=torch.float64, device=dev)
    try:
        solver.load_scene(s); solver.set_counting(False)
        solver.bind(rad_ptr=rad.data_ptr(), flux_ptr=flux.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, heat_ptr=heat.data_ptr())
        raw, net = [], []
        for pieces in ([(0, n)], [(0, n//2), (n//2, n//2)]):
            solver.reset(); flux.zero_(); heat.zero_(); torch.cuda.synchronize(dev)
            for off, cnt in pieces:
                solver.run(cnt, seed=31, offset=off)
            solver.sync(); torch.cuda.synchronize(dev)
            raw.append((flux.cpu().numpy().copy(), heat.cpu().numpy().copy()))
            net.append(solver.heating(n).astype(np.float64))
        assert '[solar+thermal]' in solver.kernel_name()
    finally:
        solver.bind(None, None, None)
    (f1, h1), (f2, h2) = raw
    assert f1.sum() > 0.0 and h1.sum() > 0.0
    assert np.allclose(f1, f2, rtol=1.0e-9, atol=0.0) and np.allclose(h1, h2, rtol=1.0e-9, atol=0.0)
    em = solver.emission().astype(np.float64)
    assert np.allclose(net[0], net[1], rtol=2.0e-7, atol=1.0e-12*em.max())      # one read-out: the emission came off once


# ---- 7: C-ABI refusals -------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals():
    from er3t_amd.solver import Mi3dSolver
    EINVAL, ESTATE, EUNSUP = -1, -2, -4
    th = column_1d(nz=6, src_wlen=WL, target=FH)
    sol = Mi3dSolver(device=0)                 # a handle of its own: no irradiance has ever been set on it
    try:
        sol.load_scene(th)
        lib, h = sol.lib, sol._h
        tmp = np.ascontiguousarray(th.tmp1d, dtype=np.float32)
        import ctypes as C
        ptr = tmp.ctypes.data_as(C.POINTER(C.c_float))
        assert lib.mi3d_set_thermal(h, 2, WL, tmp.size, ptr, None, None) == 0
        assert lib.mi3d_prepare(h) == ESTATE and lib.mi3d_run(h, 1000, 1, 0) == ESTATE
        assert 'mi3d_set_solar_irradiance' in lib.mi3d_last_error().decode()
        for bad in (-1.0, float('nan'), float('inf')):
            assert lib.mi3d_set_solar_irradiance(h, bad) == EINVAL
        assert lib.mi3d_run(h, 1000, 1, 0) == ESTATE             # (a refused value sets nothing)
        assert lib.mi3d_set_solar_irradiance(h, FSOL) == 0
        assert lib.mi3d_set_thermal(h, 0, WL, tmp.size, ptr, None, None) == EUNSUP
        em = sol.emission()                                     # needs no run
        assert em.shape == (6, 1, 1) and np.all(em > 0.0)
        ptot, psol = sol.source_power()
        assert ptot > 0.0 and abs(psol/(FSOL*abs(np.cos(np.deg2rad(th.src_the)))*1.0e8) - 1.0) < 1e-12
        assert lib.mi3d_run(h, 1000, 1, 0) == 0 and 'solar+thermal' in sol.kernel_name()
        # a camera
        cam = mix_column(target=TARGET_RADIANCE, rad_kind=1, view_the=[0.0], view_phi=[0.0], view_zloc=[10.0], nxr=8, nyr=8)
        sol.load_scene(cam)
        assert lib.mi3d_run(h, 1000, 1, 0) == EUNSUP
        # the power of a solar job is refused
        from er3t_amd.synth import les_scene
        sol.load_scene(les_scene(nx=8, ny=8, nz3=10))
        assert lib.mi3d_get_source_power(h, None, None) == ESTATE
    finally:
        sol.close()


# ---- 8: the drop-in ----------------------------------------------------------------------------------------------------------------------

def test_the_drop_in_is_the_sum_of_a_solar_and_a_thermal_simulation(tmp_path):
    import copy
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner
    from er3t_amd.synth import abs_synth, cld_synth
    from tests.golden import inputs as gin
    from tests.test_gpu_dropin import _atm, _quiet
    atm = _atm(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(3750.0, atm, Ng=4)
    ab.coef['solar']['data'] = np.array([8.0, 9.5, 10.0, 11.25])*1.0e-3           # W m-2 nm-1: about 10 W m-2 um-1, the size of the emission
    w, slit = ab.coef['weight']['data'], ab.coef['slit_func']['data']
    # (the solar route weights with slit / sum_g (weight slit), the mixed route does not: the two agree where that factor is 1)
    assert np.all(slit == 1.0) and abs(w.sum() - 1.0) < 1.0e-12
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    a1 = _quiet(mca.mca_atm_1d, atm_obj=atm, abs_obj=ab)
    a3 = _quiet(mca.mca_atm_3d, atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=4, target='radiance', surface_albedo=0.2, solar_zenith_angle=40.0, solar_azimuth_angle=30.0,
              Nrun=3, weights=w, photons=300000, solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True)
    mix = _quiet(mca.mcarats_ng, source='solar+thermal', fdir=str(tmp_path/'mix'), abs_obj=ab, keep_files=True, **kw)
    assert 'solar+thermal' in get_runner().sol.kernel_name()
    files = copy.copy(mix); files.fused = None
    fused = _quiet(mca.mcarats_ng, source='solar+thermal', fdir=str(tmp_path/'mixf'), abs_obj=ab, keep_files=False, **kw)
    assert fused.fused is not None and not os.path.exists(fused.fnames_out[0][0])
    a = mca.mca_out_ng(mca_obj=mix, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    c = mca.mca_out_ng(mca_obj=fused, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert sorted(a.keys()) == sorted(b.keys()) == sorted(c.keys()) and 'bt' in a
    scale = float(a['rad']['data'].max())
    for k in ('rad', 'rad_std', 'bt'):
        assert np.array_equal(a[k]['data'], b[k]['data']), k              # the file route and the statistics on the device: one simulation
        # ... and without the files: another simulation of the same photon ids (same clock, same seeds), whose float64 tallies are atomic sums
        # in another order, rounded to float32 once per job: a few float32 ulps after the sum over g (rad_std: of the radiance)
        assert np.allclose(a[k]['data'], c[k]['data'], rtol=1.0e-6, atol=1.0e-6*scale if k == 'rad_std' else 0.0), k
    assert a['toa']['data'] > 0.0
    m_sol = _quiet(mca.mcarats_ng, source='solar', fdir=str(tmp_path/'sol'), **kw)
    m_thm = _quiet(mca.mcarats_ng, source='thermal', fdir=str(tmp_path/'thm'), **kw)
    sol = mca.mca_out_ng(mca_obj=m_sol, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    thm = mca.mca_out_ng(mca_obj=m_thm, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    want = sol['rad']['data'].astype(np.float64) + thm['rad']['data'].astype(np.float64)
    got = a['rad']['data'].astype(np.float64)
    share = sol['rad']['data'].mean()/want.mean()
    assert 0.05 < share < 0.95                                            # both sources matter in this scene
    # pixel by pixel, the issue's bound: 3 x the combined rad_std / sqrt(Nrun) + 3e-4.  rad_std is numpy's population standard deviation
    # of THREE runs: the bound is 2.45 standard errors of a Student-t statistic with two degrees of freedom, which a correct code leaves in
    # 13.4 % of the pixels (120 pixels: 87 +- 3 % inside).  At least 75 % must lie inside, four of those standard deviations below
    std = np.sqrt(a['rad_std']['data'].astype(np.float64)**2 + sol['rad_std']['data'].astype(np.float64)**2 + thm['rad_std']['data'].astype(np.float64)**2)
    inside = np.abs(got-want) <= 3.0*std/np.sqrt(3.0) + FLOOR*want
    print('pixels inside 3 x combined rad_std / sqrt(3) + 3e-4: %.3f of %d; per-pixel relative rad_std of the mixed run %.3f' %
          (inside.mean(), inside.size, (a['rad_std']['data']/a['rad']['data']).mean()))
    assert inside.mean() >= 0.75, inside.mean()
    # the domain mean, where a wrong normalisation of the g-sum or of Src_fsol shows: against the standard error of the three simulations' own
    # per-run domain means (mode='all'), 3 of them + 3e-4
    runs = [mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='all', squeeze=True, quiet=True).data['rad']['data'].astype(np.float64).mean(axis=(0, 1))
            for m in (mix, m_sol, m_thm)]
    assert all(r.shape == (3,) for r in runs)
    se = np.sqrt(sum(r.var(ddof=1) for r in runs)/3.0)
    d = runs[0].mean() - (runs[1].mean() + runs[2].mean())
    print('domain means: mixed %.6e, solar %.6e + thermal %.6e = %.6e, difference %+.3e, se %.2e (%.2e of the mean); solar share %.3f' %
          (runs[0].mean(), runs[1].mean(), runs[2].mean(), runs[1].mean()+runs[2].mean(), d, se, se/want.mean(), share))
    assert abs(d) <= 3.0*se + FLOOR*want.mean(), (d, se)
    assert np.all(a['bt']['data'] >= thm['bt']['data'].min())             # the sun only adds


# ---- 9: two ranks against one ------------------------------------------------------------------------------------------------------------

def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on this box's one GPU) against one rank on the same photon ids
    (tests/source_mix_dist_worker.py): a radiance and a heating-rate simulation, every job file to float32 rounding -- every mixed job
    goes job by job through run, all-reduce and the read-outs that know the mixed job's amplitude"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'source_mix_dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(out, 'result.npz'))
    assert int(z['njob_radiance']) == 4 and int(z['njob_heating']) == 4
    assert 'solar+thermal' in str(z['kernel_radiance']) and 'solar+thermal' in str(z['kernel_heating'])
    em = float(z['emission_max'])
    for j in range(4):
        a, b = z['dist_rad_%d' % j], z['solo_rad_%d' % j]
        assert a.shape == b.shape and a.max() > 0.0 and np.allclose(a, b, rtol=2.0e-7, atol=0.0), (j, np.abs(a-b).max())
        a, b = z['dist_hrt_%d' % j], z['solo_hrt_%d' % j]
        assert a.shape == b.shape and np.allclose(a, b, rtol=2.0e-7, atol=1.0e-12*em), (j, np.abs(a-b).max())
        for name in ('fdnd', 'fdn', 'fup'):
            a, b = z['dist_%s_%d' % (name, j)], z['solo_%s_%d' % (name, j)]
            assert a.max() > 0.0 and np.allclose(a, b, rtol=2.0e-7, atol=0.0), (name, j)
