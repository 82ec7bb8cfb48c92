"""
The path-length estimator of the heating rates (mi3d_set_heating_estimator 1, Scene.heat_estimator, Flx_mhest = 1) on the GPU: a closed
form, the oracle's collision estimator (which stays the independent answer), the energy budget, what the estimator is for (less noise in
optically thin layers), the routes (tally records, atomics, the general loop), the flux planes it must not touch, and the drop-in.

Statistics: nb independent batches of photon ids (by `offset`); se = batch standard deviation / sqrt(nb); a relative float32 floor of 3e-4.
Every figure a test asserts on is printed first (run with -s to see them).
"""

import dataclasses

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_HEAT
from er3t_amd.synth import les_scene
from tests.test_gpu_parity import gpu_run
from tests.util import slab_scene

pytestmark = pytest.mark.gpu

FLOOR = 3.0e-4


def heat_scene(**kw):
    """the scene of tests/test_gpu_parity.py::test_heating_rates_parity_and_energy_budget: 16 x 16 x 68, clouds, aerosol, gas absorption x 30"""
    sc = les_scene(nx=16, ny=16, nz3=50, target='flux', aerosol=True)
    sc.target = TARGET_FLUX | TARGET_HEAT
    sc.abs1d = sc.abs1d*30.0
    for k, v in kw.items():
        setattr(sc, k, v)
    return sc


def batches(sol, scene, nb, nper, seed=1):
    """nb independent batches of nper photons: per-batch heating and flux fields (nb, nz, ny, nx), (nb, 3, nz+1, ny, nx)"""
    sol.bind(None, None, None)
    sol.load_scene(scene)
    sol.set_counting(False)
    heat, flux = [], []
    for b in range(nb):
        sol.reset()
        sol.run(nper, seed=seed, offset=b*nper)
        sol.sync()
        heat.append(sol.heating(nper).astype(np.float64))
        flux.append(sol.flux(nper).astype(np.float64))
    return np.array(heat), np.array(flux)


def total_extinction(sc):
    """(nz, ny, nx) total extinction of every cell, as the solver adds it up: 1-D constituents and gas, 3-D constituents and absorber"""
    bt = np.tile((np.asarray(sc.ext1d, dtype=np.float64).sum(axis=0) + np.asarray(sc.abs1d, dtype=np.float64))[:, None, None], (1, sc.ny, sc.nx))
    if sc.nz3 > 0:
        k0 = sc.iz3l - 1
        bt[k0:k0+sc.nz3] += np.asarray(sc.extp, dtype=np.float64).sum(axis=0)
        if sc.abst is not None:
            bt[k0:k0+sc.nz3] += np.asarray(sc.abst, dtype=np.float64)
    return bt


def thin_layers(sc, limit=0.05):
    """layers whose optical thickness beta_t dz is at most `limit` in every column"""
    tau = (total_extinction(sc)*np.diff(sc.zgrd)[:, None, None]).reshape(sc.nz, -1).max(axis=1)
    return np.where(tau <= limit)[0]


def walked_layers(sc):
    """layers the photon loops walk voxel by voxel: the total extinction varies horizontally"""
    return np.where(total_extinction(sc).reshape(sc.nz, -1).std(axis=1) > 0.0)[0]


def is_path_flux_loop(name):
    return name.startswith('k_transport_flux<') and name.split('>')[0].count(',') == 3      # (k_transport_flux<count, p3d, mix, 1>)


# ---- 4: closed form --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout, sza', [('1d', 30.0), ('1d', 60.0), ('3d', 30.0), ('3d', 60.0), ('walk', 0.0)])
def test_non_scattering_slab_matches_beer_law_layer_by_layer(solver, layout, sza):
    """A non-scattering absorbing slab over a black surface (K17's first case): heat_k dz_k = mu0 (exp(-tau_top / mu0) - exp(-tau_bot / mu0)),
    tau from the top, per layer within 3 se + floor (ten layers per case: 0.03 false alarms expected).  '1d': 1-D layers; '3d': the lower
    five layers carried by a 3-D region (horizontally uniform: crossed level by level); 'walk' (beyond what the issue asks): a checkerboard
    absorber in the 3-D region under an overhead sun -- the voxel walk's records, every column its own slab."""
    nz, ztop, abs_tau = 10, 4000.0, 1.0
    kw = dict(tau=0.0, abs_tau=abs_tau, albedo=0.0, sza=sza, nz=nz, ztop=ztop, target=TARGET_FLUX | TARGET_HEAT)
    if layout == '1d':
        sc = slab_scene(**kw)
    else:
        sc = slab_scene(nx=4, ny=4, nz3=5, **kw)
    kabs = np.tile(np.full(nz, abs_tau/ztop)[:, None, None], (1, sc.ny, sc.nx))
    if layout == 'walk':
        yy, xx = np.meshgrid(np.arange(sc.ny), np.arange(sc.nx), indexing='ij')
        abst = np.tile((((xx+yy) % 2)*2.0*abs_tau/ztop)[None], (5, 1, 1)).astype(np.float32)
        sc = dataclasses.replace(sc, abst=abst)
        kabs[:5] += abst
    sc.heat_estimator = 1
    nb = 16
    heat, _ = batches(solver, sc, nb, 200000, seed=5)
    assert is_path_flux_loop(solver.kernel_name()), solver.kernel_name()
    if layout == 'walk':
        assert len(walked_layers(sc)) == 5
    dz = np.diff(sc.zgrd)
    mu0 = np.cos(np.radians(sza))
    dtau = kabs*dz[:, None, None]
    tau_top = np.concatenate([np.cumsum(dtau[::-1], axis=0)[::-1][1:], np.zeros((1, sc.ny, sc.nx))])     # above every layer
    want = (mu0*(np.exp(-tau_top/mu0) - np.exp(-(tau_top+dtau)/mu0))).mean(axis=(1, 2))
    got_b = heat.mean(axis=(2, 3))*dz
    got, se = got_b.mean(axis=0), got_b.std(axis=0, ddof=1)/np.sqrt(nb)
    print(layout, sza, 'z per layer:', np.round((got-want)/np.hypot(se, FLOOR*want), 2), 'relative se:', np.round(se/want, 5))
    assert np.all(np.abs(got-want) <= 3.0*se + FLOOR*want), (got, want, se)


# ---- 5: the oracle's collision estimator -----------------------------------------------------------------------------------------------

def _layer_z(hg, ho, nb):
    gm, om = hg.mean(axis=(0, 2, 3)), ho.mean(axis=(0, 2, 3))
    se_g = hg.mean(axis=(2, 3)).std(axis=0, ddof=1)/np.sqrt(nb)
    se_o = ho.mean(axis=(2, 3)).std(axis=0, ddof=1)/np.sqrt(nb)
    return gm, om, (gm-om)/np.sqrt(se_g**2 + se_o**2)


def test_parity_with_the_oracles_collision_estimator(solver, oracle, nthreads):
    """Estimator 1 on the GPU against the oracle's collision estimator, two unbiased estimators of one quantity, batch for batch on the
    same photon ids.  Layer means: z = (gpu - oracle) / sqrt(se_g^2 + se_o^2) within |z| < 4, |mean z| < 0.5, std z < 1.4; column total within
    3e-3.  Cell by cell in the voxel-walked layers: at least 0.99 of the cells within |z| <= 3, |mean z| <= 0.2.  32 batches of 250 000 photons:
    the oracle's cells of those layers then hold (mean / se)^2 = 1.1e4 on average (124 in the thinnest aerosol layer), and the oracle against
    its own second seed gives a share of 0.9972, mean z 0.011 (measured on the CPU before this test was run)."""
    sc = heat_scene()
    nb, nper = 32, 250000
    ho = np.stack([oracle.run(sc, nper, seed=7, offset=b*nper, nthreads=nthreads)['heat'] for b in range(nb)])
    sc.heat_estimator = 1
    hg, _ = batches(solver, sc, nb, nper, seed=7)
    assert is_path_flux_loop(solver.kernel_name()), solver.kernel_name()
    gm, om, z = _layer_z(hg, ho, nb)
    dz = np.diff(sc.zgrd)
    tot = (gm*dz).sum()/(om*dz).sum() - 1.0
    print('layer z: mean %.3f std %.3f max |z| %.2f; column total off by %.2e' % (z.mean(), z.std(), np.abs(z).max(), tot))
    assert om.max() > 0.0 and np.all(np.abs(z) < 4.0) and abs(z.mean()) < 0.5 and z.std() < 1.4, (z.mean(), z.std(), np.abs(z).max())
    assert abs(tot) < 3e-3, tot
    kw = walked_layers(sc)
    assert len(kw) >= 20
    cg, co = hg[:, kw], ho[:, kw]
    se2 = cg.var(axis=0, ddof=1)/nb + co.var(axis=0, ddof=1)/nb
    assert np.all(se2 > 0.0) and (co.mean(axis=0)**2/(co.var(axis=0, ddof=1)/nb)).mean() >= 100.0
    zc = (cg.mean(axis=0) - co.mean(axis=0))/np.sqrt(se2)
    print('cells of the walked layers: share |z| <= 3 %.4f, mean z %.3f, std %.3f' % (np.mean(np.abs(zc) <= 3.0), zc.mean(), zc.std()))
    assert np.mean(np.abs(zc) <= 3.0) >= 0.99, np.mean(np.abs(zc) <= 3.0)
    assert abs(zc.mean()) <= 0.2, zc.mean()


@pytest.mark.parametrize('mode', [1, 2], ids=['partial3d', 'ipa'])
def test_parity_with_the_oracle_under_the_other_solvers(solver, oracle, nthreads, mode):
    """the same by layer means under the partial 3-D solver and the independent-column approximation (the photon's column is the cell)"""
    sc = heat_scene(solver=mode)
    nb, nper = 16, 50000
    ho = np.stack([oracle.run(sc, nper, seed=9, offset=b*nper, nthreads=nthreads)['heat'] for b in range(nb)])
    sc.heat_estimator = 1
    hg, _ = batches(solver, sc, nb, nper, seed=9)
    assert is_path_flux_loop(solver.kernel_name()), solver.kernel_name()
    gm, om, z = _layer_z(hg, ho, nb)
    dz = np.diff(sc.zgrd)
    tot = (gm*dz).sum()/(om*dz).sum() - 1.0
    print('solver %d layer z: mean %.3f std %.3f max |z| %.2f; column total off by %.2e' % (mode, z.mean(), z.std(), np.abs(z).max(), tot))
    assert np.all(np.abs(z) < 4.0) and abs(z.mean()) < 0.5 and z.std() < 1.4, (z.mean(), z.std(), np.abs(z).max())
    assert abs(tot) < 3e-3, tot


# ---- 6: the budget ---------------------------------------------------------------------------------------------------------------------

def test_energy_budget_closes_in_expectation(solver):
    """Without roulette (wmin 0, albedo 0.3): d_b = sum_k heat_k dz_k - [(F_down - F_up)_top - (F_down - F_up)_surface], domain means, batch by
    batch.  Under the collision estimator d closes history by history (2e-5 of the beam, K17); under the path-length estimator only its
    expectation does: |mean d| <= 3 se(d) + 2e-5 mu0.  Layer by layer: heat_k dz_k against the divergence of the same job's net flux, z from the
    batch differences, within |z| < 4, |mean z| < 0.5, std z < 1.4."""
    sc = heat_scene(wmin=0.0, heat_estimator=1)
    sc.sfc_param[0] = 0.3
    nb = 32
    heat, flux = batches(solver, sc, nb, 100000, seed=3)
    assert is_path_flux_loop(solver.kernel_name()), solver.kernel_name()
    dz = np.diff(sc.zgrd)
    f = flux.mean(axis=(3, 4))                               # (nb, 3, nz+1)
    net = f[:, 1] - f[:, 2]                                  # net downward flux at every level
    hk = heat.mean(axis=(2, 3))*dz                           # (nb, nz)
    d = hk.sum(axis=1) - (net[:, -1] - net[:, 0])
    print('budget: mean d %.3e, se %.3e, absorbed %.4f of mu0 %.4f' % (d.mean(), d.std(ddof=1)/np.sqrt(nb), hk.sum(axis=1).mean(), sc.mu0))
    assert hk.sum(axis=1).mean() > 0.02*sc.mu0
    assert abs(d.mean()) <= 3.0*d.std(ddof=1)/np.sqrt(nb) + 2e-5*sc.mu0, (d.mean(), d.std(ddof=1)/np.sqrt(nb))
    dl = hk - (net[:, 1:] - net[:, :-1])                     # (nb, nz): what the layer absorbs less what the fluxes say it does
    z = dl.mean(axis=0)/(dl.std(axis=0, ddof=1)/np.sqrt(nb))
    print('layers against the flux divergence: z mean %.3f std %.3f max |z| %.2f' % (z.mean(), z.std(), np.abs(z).max()))
    print('z per layer:', np.round(z, 2))
    assert np.all(np.abs(z) < 4.0) and abs(z.mean()) < 0.5 and z.std() < 1.4, (z.mean(), z.std(), np.abs(z).max())


# ---- 7: what it is for -----------------------------------------------------------------------------------------------------------------

def test_thin_layers_get_less_than_half_the_noise(solver):
    """Same scene, same photon ids, both estimators: in every layer with beta_t dz <= 0.05 (domain maximum) the batch se of the layer mean
    under the path-length estimator is at most half of that under the collision estimator.  (se ratio ~ sqrt(tau_t c), c = O(1) from the
    spread of slant paths: 0.22 sqrt(c) at tau_t = 0.05; 0.5 leaves a factor of two.  32 batches: a ratio of two sample standard
    deviations is known to 18 %.)"""
    sc = heat_scene()
    thin = thin_layers(sc)
    assert len(thin) >= 5
    nb, nper = 32, 100000
    se = []
    for est in (0, 1):
        sc.heat_estimator = est
        heat, _ = batches(solver, sc, nb, nper, seed=21)
        assert is_path_flux_loop(solver.kernel_name()) == bool(est), solver.kernel_name()
        se.append(heat.mean(axis=(2, 3)).std(axis=0, ddof=1)/np.sqrt(nb))
    ratio = se[1]/se[0]
    tau = (total_extinction(sc)*np.diff(sc.zgrd)[:, None, None]).reshape(sc.nz, -1).max(axis=1)
    print('se(path) / se(collision) per layer [layer: tau_max, ratio]:', ' '.join('%d: %.4f, %.3f;' % (k, tau[k], ratio[k]) for k in range(sc.nz)))
    assert np.all(se[0][thin] > 0.0) and np.all(ratio[thin] <= 0.5), ratio[thin]


# ---- 8: routes -------------------------------------------------------------------------------------------------------------------------

def test_record_atomic_and_general_routes_agree(solver):
    """Estimator 1: tally records (sorted and summed after the launch) against an atomic per record -- same histories, same records: the
    counters equal, the heating rates to the order of the float64 sums; the lean flux loop against the general loop, another float32
    program: layer sums within 5e-3 (the bounds of test_gpu_parity.py::test_flux_tally_routes_agree, its absolute term scaled to the
    largest layer sum as there: 1e-3 of sums of order 200)"""
    sc = heat_scene(heat_estimator=1)
    n = 300000
    try:
        ref = gpu_run(solver, sc, n, seed=11)
        name = solver.kernel_name()
        assert is_path_flux_loop(name) and 'k_tl_scatter' in name, name
        solver.set_tuning(tally_lists=0)
        atom = gpu_run(solver, sc, n, seed=11)
        name = solver.kernel_name()
        assert is_path_flux_loop(name) and 'k_tl_scatter' not in name, name
        solver.set_tuning(tally_lists=1)
        solver.set_kernel(general=True)
        gen = gpu_run(solver, sc, n, seed=11)
        name = solver.kernel_name()
        assert name.startswith('k_transport<') and 'path length' in name, name
    finally:
        solver.set_tuning(tally_lists=1)
        solver.set_kernel()
    assert atom['counters']['flux_tally'] == ref['counters']['flux_tally']
    assert ref['heat'].max() > 0.0
    assert np.allclose(atom['heat'], ref['heat'], rtol=1e-6, atol=1e-9*ref['heat'].max())
    assert np.allclose(atom['flux'], ref['flux'], rtol=1e-6, atol=1e-9)
    gs, rs = gen['heat'].sum(axis=(1, 2)), ref['heat'].sum(axis=(1, 2))
    print('general / lean layer sums - 1:', np.round(gs/rs - 1.0, 5))
    assert np.allclose(gs, rs, rtol=5e-3, atol=5e-6*rs.max())


@pytest.mark.parametrize('nx', [128, 481])
def test_records_equal_atomics_beyond_256_bins(solver, nx):
    """as tests/test_gpu_fullsize.py::test_tally_records_equal_an_atomic_per_crossing_beyond_256_bins builds them: the 128 x 128 x 69 grid with
    heating cells (279 bins) and 480 x 480 x 100 with them (the workgroups' compact histogram, which under estimator 1 covers the heating
    cells of every layer), estimator 1: records twice and atomics once, every cell equal to the float32 precision of the output"""
    from bench import make_scene
    from er3t_amd.synth import z_levels_config4
    if nx == 128:
        sc = make_scene('les128_flux')
    else:
        sc = les_scene(nx=480, ny=480, nz3=100, levels=z_levels_config4(), z_top=1.6, seed=20251004, target='flux')
    sc.target = TARGET_FLUX | TARGET_HEAT
    sc.abs1d = sc.abs1d*30.0 + 2.0e-5
    sc.heat_estimator = 1
    n = 10000000
    solver.bind(None, None, None); solver.load_scene(sc); solver.set_counting(False)
    out = []
    try:
        for lists in (1, 1, 0):
            solver.set_tuning(tally_lists=lists)
            solver.reset(); solver.run(n, seed=7); solver.sync()
            name = solver.kernel_name()
            assert is_path_flux_loop(name) and ('k_tl_scatter' in name) == bool(lists), name
            out.append((solver.flux(n).astype(np.float64), solver.heating(n).astype(np.float64)))
    finally:
        solver.set_tuning(tally_lists=1)
    assert out[2][1].max() > 0.0
    for f, hh in out[:2]:
        assert np.abs(f-out[2][0]).max() <= 2e-6*out[2][0].max() and np.abs(hh-out[2][1]).max() <= 2e-6*out[2][1].max()


# ---- 9: the flux planes ----------------------------------------------------------------------------------------------------------------

def test_flux_planes_do_not_depend_on_the_estimator(solver):
    """the estimator draws no random number and touches no weight: the three flux planes of a job are what they are under the other one,
    to the order of their float64 sums"""
    sc = heat_scene()
    n = 400000
    a = gpu_run(solver, sc, n, seed=13)
    assert not is_path_flux_loop(solver.kernel_name())
    sc.heat_estimator = 1
    b = gpu_run(solver, sc, n, seed=13)
    assert is_path_flux_loop(solver.kernel_name())
    for key in ('photons', 'scatter', 'surface', 'escaped', 'absorbed', 'flux_tally'):
        assert a['counters'][key] == b['counters'][key], key
    assert np.allclose(a['flux'], b['flux'], rtol=1e-9, atol=0.0)
    assert not np.array_equal(a['heat'], b['heat'])


def test_the_setter_refuses_anything_but_0_and_1(solver):
    with pytest.raises(OSError):
        solver.set_heating_estimator(2)
    solver.set_heating_estimator(0)


# ---- 10: the drop-in -------------------------------------------------------------------------------------------------------------------

def test_heating_estimator_through_the_dropin(tmp_path):
    """mcarats_ng(target='heating rate', heating_estimator='path', Nrun=3) + mca_out_ng: the same variable as under the default, layer
    means within 4 x the larger heating_rate_std / sqrt(3) + floor (the layer's mean of the std field), named for its estimator, and
    with a smaller heating_rate_std in the layers that are optically thin (beta_t dz <= 0.05 in every column and every g)"""
    import er3t_amd.rtm.mca as mca
    from er3t_amd.synth import abs_synth, cld_synth
    from tests.golden import inputs as gin
    from tests.test_gpu_dropin import _atm, _quiet
    atm = _atm(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(650.0, atm, Ng=4)
    ab.coef['abso_coef']['data'] = ab.coef['abso_coef']['data']*40.0
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    a1 = _quiet(mca.mca_atm_1d, atm_obj=atm, abs_obj=ab)
    a3 = _quiet(mca.mca_atm_3d, atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
    out, tau = {}, None
    for est in ('collision', 'path'):
        m = _quiet(mca.mcarats_ng, atm_1ds=[a1], atm_3ds=[a3], Ng=4, target='heating rate', surface_albedo=0.2, solar_zenith_angle=40.0,
                   solar_azimuth_angle=30.0, fdir=str(tmp_path/est), Nrun=3, weights=ab.coef['weight']['data'], photons=400000,
                   solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True, heating_estimator=est)
        assert ('Flx_mhest' in mca.mca_inp_read(m.fnames_inp[2][3])) == (est == 'path')
        out[est] = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
        if tau is None:
            import os
            taus = []
            for fname in m.fnames_inp[0]:
                sc = Scene.from_nml(mca.mca_inp_read(fname), os.path.dirname(fname), solver=0)
                taus.append((total_extinction(sc)*np.diff(sc.zgrd)[:, None, None]).reshape(sc.nz, -1).max(axis=1))
            tau = np.max(taus, axis=0)
    assert 'path-length estimator' in out['path']['heating_rate']['name'] and 'path' not in out['collision']['heating_rate']['name']
    assert out['path']['heating_rate']['units'] == out['collision']['heating_rate']['units']
    h0, h1 = out['collision']['heating_rate']['data'].mean(axis=(0, 1)), out['path']['heating_rate']['data'].mean(axis=(0, 1))
    s0, s1 = out['collision']['heating_rate_std']['data'].mean(axis=(0, 1)), out['path']['heating_rate_std']['data'].mean(axis=(0, 1))
    thin = np.where(tau <= 0.05)[0]
    print('layer means path / collision - 1:', np.round(h1/h0 - 1.0, 4))
    print('layer mean of heating_rate_std, path / collision:', np.round(s1/s0, 3), 'thin layers:', thin)
    assert h0.shape == h1.shape and h0.min() > 0.0
    assert np.all(np.abs(h1-h0) <= 4.0*np.maximum(s0, s1)/np.sqrt(3.0) + FLOOR*h0), (h1, h0)
    assert len(thin) >= 5 and np.all(s1[thin] < s0[thin]), (s1[thin]/s0[thin])
