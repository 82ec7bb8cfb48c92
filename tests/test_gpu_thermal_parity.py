"""
The thermal source (Src_mtype = 3) and the rectangular camera map (Rad_mpmap = 2, Rad_mrproj) on the GPU against the CPU oracle,
which follows the same Philox stream per photon id (oracle/mi3d_oracle.c, pinned by tests/test_oracle_thermal.py):
  * the source's CDF (k_thermal_power, k_scan_chunk / _top / _add) exactly, at cell counts on both sides of the scan's block and
    top-level edges, and against the oracle's cell powers on a scene with every kind of emitting cell,
  * single histories of every thermal build, batch parity on the LES scene, id-range additivity, random corner scenes,
  * multi-pixel rectangular camera images of the cloud scene, as check_radiance holds every solar image.
Tolerances are those of tests/test_gpu_parity.py unless stated.
"""

import dataclasses
import re

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE, SOLVER_3D, SOLVER_P3D, SOLVER_IPA
from er3t_amd.synth import les_scene
from tests.test_gpu_parity import gpu_run, oracle_batches, check_counters, check_radiance
from tests.test_gpu_radiometer import cameras
from tests.test_gpu_thermal import column_1d
from tests.util import thermal_mixed_scene, thermal_powers_np

pytestmark = pytest.mark.gpu

WL = 11.0


def marched(sc, column_le=True):
    """whether a radiance job of sc marches local-estimate rays: every view that is not nadir from above the atmosphere, or all"""
    if not sc.target & TARGET_RADIANCE:
        return False
    return (not column_le) or any(abs(t-180.0) > 1e-9 or z < sc.zgrd[-1] for t, z in zip(sc.view_the, sc.view_zloc))


def assert_thermal_build(solver, march, flux, p3d):
    name = solver.kernel_name()
    assert re.fullmatch(r'k_transport<\d,%d,%d,%d> \[thermal\]' % (int(march), int(flux), int(p3d)), name), name


def thermal_les(nx=16, ny=16, nz3=50, tmpa=True, **kw):
    """the LES cloud scene as a thermal scene: 11 um, gas absorption in every layer, cloud droplets absorbing 3 % of what they
    extinguish (ka / beta >= 1e-3 in every emitting cell), a lapse-rate profile, voxel anomalies, a grey Lambert surface"""
    s0 = les_scene(nx=nx, ny=ny, nz3=nz3, **kw)
    rng = np.random.default_rng(7)
    nz = s0.nz
    return dataclasses.replace(s0, abs1d=np.full(nz, 2.0e-5, dtype=np.float32), omgp=(s0.omgp*np.float32(0.97)),
                               sfc_mtype=1, sfc_param=[0.1, 0, 0, 0, 0], jsfc=None, psfc=None,
                               src_mtype=3, src_wlen=WL, tmp1d=np.linspace(292.0, 210.0, nz+1),
                               tmpa3d=(rng.uniform(-4.0, 4.0, (s0.nz3, s0.ny, s0.nx)) if tmpa else None))


# ---------------------------------------------------------------------------------------------
def _scan_scene(ncell, seed):
    """a grid of exactly ncell thermal cells whose float32 records hold ka exactly: one absorbing 3-D constituent (omega = 0), no
    other extinction; log-normal absorption (zero in a fifth of the voxels), voxel and surface temperature anomalies, a 2-D surface
    of random albedo filling the count up"""
    nx = ny = 16 if ncell < 5000 else 256
    cols = nx*ny
    nz3 = (ncell-2)//(cols+1)
    nz = nz3+1
    nsfc = ncell - cols*nz3 - nz
    assert nz3 >= 1 and nsfc >= 1
    rng = np.random.default_rng(seed)
    shape = (nz3, ny, nx)
    ka = (1.0e-4*rng.lognormal(0.0, 2.0, shape)*(rng.random(shape) > 0.2)).astype(np.float32)
    psfc = np.zeros((5, 1, nsfc)); psfc[0] = rng.uniform(0.0, 0.9, (1, nsfc))
    return Scene(zgrd=np.arange(nz+1)*200.0, ext1d=np.zeros((1, nz)), omg1d=np.zeros((1, nz)), apf1d=np.zeros((1, nz)), abs1d=np.zeros(nz),
                 nx=nx, ny=ny, dx=100.0, dy=100.0, nz3=nz3, iz3l=1, extp=ka[None], omgp=np.zeros((1,)+shape), apfp=np.zeros((1,)+shape),
                 sfc_mtype=1, sfc_param=[0.0, 0, 0, 0, 0], jsfc=np.ones((1, nsfc)), psfc=psfc, target=TARGET_RADIANCE,
                 view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=1, nyr=1, src_mtype=3, src_wlen=WL,
                 tmp1d=np.linspace(290.0, 250.0, nz+1), tmpa3d=rng.uniform(-20.0, 20.0, shape), tmps2d=rng.uniform(-20.0, 20.0, (1, nsfc)),
                 src_the=180.0, src_qmax=0.0)


@pytest.mark.parametrize('ncell', [2047, 2048, 2049, 2048*1024, 2048*1024+1, 3*2**21+5])
def test_thermal_cdf_is_exact_across_the_scan_edges(solver, ncell):
    """the device CDF against a numpy float64 cumsum of the same cells' powers: a dropped block offset or a lost carry of k_scan_top
    moves an element by at least one cell's power (~1e-7 P_tot at these sizes)"""
    s = _scan_scene(ncell, ncell)
    solver.load_scene(s)
    pw = thermal_powers_np(s)
    assert pw.size == ncell and np.count_nonzero(pw) > 0.5*ncell
    ptot, cdf = solver.debug_thermal(ncell)
    want = np.cumsum(pw)
    assert ptot == cdf[-1]
    err = np.abs(cdf-want)
    assert err.max() <= 1e-10*want[-1], (err.max()/want[-1], int(err.argmax()))
    d = np.diff(np.concatenate([[0.0], cdf]))
    assert np.all(np.abs(d-pw) <= 1e-8*pw + 1e-13*want[-1]), int(np.argmax(np.abs(d-pw)-1e-8*pw))


def test_thermal_cdf_matches_the_oracle_cell_by_cell(solver, oracle):
    """every kind of emitting cell (voxels of two constituents + gas, 1-D layers with scattering, a 2-D surface coarser than the
    voxel grid): powers within 1e-6 of 4 pi beta B V (float32 beta - ks on the device, ka in double in the oracle)"""
    s = thermal_mixed_scene()
    solver.load_scene(s)
    ocdf = oracle.thermal_cdf(s)
    ptot, cdf = solver.debug_thermal(ocdf.size)
    scale = thermal_powers_np(dataclasses.replace(s, omg1d=np.zeros_like(s.omg1d), omgp=np.zeros_like(s.omgp),
                                                  psfc=np.zeros_like(s.psfc)))       # 4 pi beta B V; pi B A for the surface
    dg = np.diff(np.concatenate([[0.0], cdf])); do = np.diff(np.concatenate([[0.0], ocdf]))
    assert np.all(np.abs(dg-do) <= 1e-6*scale + 1e-13*ocdf[-1]), np.max(np.abs(dg-do)/scale)
    assert abs(ptot/ocdf[-1]-1.0) < 1e-6


def test_debug_thermal_refuses_a_solar_job(solver):
    solver.load_scene(les_scene(nx=8, ny=8, nz3=10))
    with pytest.raises(OSError):
        solver.debug_thermal(10)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['1d', 'voxels', 'sfc2d', 'marched', 'flux', 'flux+marched', 'p3d', 'tables', 'up_looking'])
def test_thermal_single_histories_follow_the_oracle(solver, oracle, variant):
    """one photon id at a time, every thermal build: at least 85 % of the histories have identical event counts (a launch that
    read its random numbers in another order would leave almost none)"""
    column_le = variant not in ('marched', 'flux+marched')
    if variant == '1d':
        sc = column_1d(nz=10, target=TARGET_RADIANCE, ext1d=np.full(10, 2.0e-4), omg1d=np.full(10, 0.8), apf1d=np.full(10, 0.7),
                       sfc_param=[0.2, 0, 0, 0, 0])
    elif variant == 'sfc2d':
        sc = thermal_mixed_scene(target=TARGET_RADIANCE)
    elif variant == 'tables':
        sc = thermal_les(mie=True)
    elif variant == 'p3d':
        sc = thermal_les(solver=SOLVER_P3D, vza=(0.0, 26.1), vaa=(0.0, 180.0))
    elif variant == 'up_looking':
        sc = thermal_les(vza=(180.0, 130.0, 0.0), vaa=(0.0, 250.0, 0.0))
        sc.view_zloc = [0.0, 900.0, 705000.0]
    elif not column_le:
        sc = thermal_les(vza=(0.0, 40.0), vaa=(0.0, 120.0))
    else:
        sc = thermal_les()
    if variant.startswith('flux'):
        sc.target = TARGET_FLUX | TARGET_RADIANCE
    keys = ('scatter', 'surface', 'roulette', 'killed', 'escaped', 'absorbed')
    solver.bind(None, None, None)
    solver.load_scene(sc, column_le=column_le)
    solver.set_counting(True)
    same, nph = 0, 96
    for i in range(nph):
        solver.reset(); solver.run(1, seed=5, offset=i); solver.sync()
        g = solver.counters()
        o = oracle.run(sc, 1, seed=5, offset=i, nthreads=1)['counters']
        assert g['photons'] == 1 and g['killed']+g['escaped']+g['absorbed'] == 1
        same += all(g[k] == o[k] for k in keys)
    assert same >= 0.85*nph, (variant, same, nph)
    assert_thermal_build(solver, march=marched(sc, column_le), flux=variant.startswith('flux'), p3d=(variant == 'p3d'))


@pytest.mark.parametrize('case', ['nadir_column', 'three_views', 'up_looking', 'p3d', 'ipa', 'flux'])
def test_thermal_parity_les(solver, oracle, nthreads, case):
    """batch parity on the same photon ids (16 oracle batches of 20 000): counters, images (check_radiance) and, for flux, all three
    planes at every level -- the direct plane exactly 0 on both sides"""
    kw = {}
    column_le = True
    if case == 'three_views':
        kw.update(vza=(0.0, 45.6, 60.0), vaa=(0.0, 30.0, 200.0))
    if case == 'up_looking':
        kw.update(vza=(180.0, 150.0, 130.0, 0.0), vaa=(0.0, 60.0, 250.0, 0.0))
    if case == 'p3d':
        kw.update(solver=SOLVER_P3D, vza=(0.0, 26.1), vaa=(0.0, 180.0))
    if case == 'ipa':
        kw.update(solver=SOLVER_IPA, vza=(0.0, 26.1), vaa=(0.0, 180.0))
    if case == 'flux':
        kw.update(target='flux')
    sc = thermal_les(**kw)
    if case == 'up_looking':
        sc.view_zloc = [0.0, 0.0, 900.0, 705000.0]
    nb, nper = 16, 20000
    o = oracle_batches(oracle, sc, nb, nper, 7, nthreads)
    g = gpu_run(solver, sc, nb*nper, seed=7, column_le=column_le)
    assert_thermal_build(solver, march=marched(sc, column_le), flux=(case == 'flux'), p3d=(case == 'p3d'))
    # (check_counters holds the GPU's flux tallies below the oracle's: a solar job adds its direct beam above the 3-D region
    #  analytically.  A thermal job has none and both sides tally every crossing: the counts agree both ways)
    gf, of = g['counters']['flux_tally'], o['counters']['flux_tally']
    assert abs(gf-of) <= 1e-3*of, (gf, of)
    check_counters(dict(g['counters'], flux_tally=min(gf, of)), o['counters'])
    if case != 'flux':
        check_radiance(g, o, zstd_max={'ipa': 0.05, 'p3d': 0.3}.get(case, 0.8))
        assert np.all(g['rad'].mean(axis=(1, 2)) > 0.0)
        return
    assert np.all(g['flux'][0] == 0.0) and np.all(o['flux'][0] == 0.0)
    gm = g['flux'].mean(axis=(2, 3)); om = o['flux'].mean(axis=(2, 3)); se = o['flux_mean_se']
    for p in (1, 2):
        lev = om[p] > 0.0
        assert np.all(np.abs(gm[p]-om[p])[lev] < 2.0*np.sqrt(2.0)*se[p][lev] + 2e-4*om[p][lev]), (p, np.abs(gm[p]-om[p]).max())
        sep = np.maximum(o['flux_se'][p], 1e-12)
        z = (g['flux'][p]-o['flux'][p])/(np.sqrt(2.0)*sep)
        z = z[(o['flux'][p] > 0) & (o['flux_se'][p] > 0)]
        assert np.mean(np.abs(z) > 3.0) < 0.05 and abs(z.mean()) < 0.5, (p, np.mean(np.abs(z) > 3.0), z.mean())


def test_thermal_id_ranges_add_up(solver):
    """tallies of ids [0, N) equal those of [0, N/2) plus [N/2, N): the thermal launch runs in id order and sharding relies on it"""
    sc = thermal_les(vza=(0.0, 40.0), vaa=(0.0, 120.0))
    sc.target = TARGET_FLUX | TARGET_RADIANCE
    n = 400000
    g = gpu_run(solver, sc, n, seed=31)
    solver.reset()
    solver.run(n//2, seed=31, offset=0); solver.run(n-n//2, seed=31, offset=n//2); solver.sync()
    rad = solver.radiance(n).astype(np.float64); flux = solver.flux(n).astype(np.float64)
    c2 = solver.counters()
    for k in ('photons', 'scatter', 'surface', 'le_rays', 'roulette', 'killed', 'escaped', 'absorbed', 'flux_tally'):
        assert c2[k] == g['counters'][k], k
    assert np.allclose(rad, g['rad'], rtol=1e-5, atol=1e-6*np.abs(g['rad']).max())
    assert np.allclose(flux, g['flux'], rtol=1e-5, atol=1e-6*np.abs(g['flux']).max())


def _random_thermal_scene(rng, i):
    """corners: nz3 = 1, nx = 1, the 3-D region at the top or the bottom, layers with no absorption, grey and black surfaces"""
    nz = int(rng.integers(2, 7))
    nz3 = 1 if i % 3 == 0 else int(rng.integers(1, nz+1))
    iz3l = int(rng.choice([1, nz-nz3+1]))
    nx = 1 if i % 4 == 1 else int(rng.integers(1, 6))
    ny = int(rng.integers(1, 6))
    dz = float(rng.choice([50.0, 500.0]))
    zgrd = np.arange(nz+1)*dz
    ext1d = rng.choice([0.0, 2e-4, 2e-3], size=(1, nz))
    abs1d = rng.choice([0.0, 1e-4, 1e-3], size=nz)
    shape = (nz3, ny, nx)
    extp = (rng.choice([0.0, 1e-3, 2e-2], size=shape)*rng.uniform(0.5, 2.0, shape)).astype(np.float32)[None]
    omgp = rng.choice([0.0, 0.5, 0.95], size=(1,)+shape).astype(np.float32)
    nv = int(rng.integers(1, 3))
    vza = rng.choice([0.0, 30.0, 150.0, 180.0], size=nv)
    sc = Scene(zgrd=zgrd, ext1d=ext1d, omg1d=rng.choice([0.5, 0.9], size=(1, nz)), apf1d=np.full((1, nz), 0.5), abs1d=abs1d,
               nx=nx, ny=ny, dx=200.0, dy=300.0, nz3=nz3, iz3l=iz3l, extp=extp, omgp=omgp, apfp=np.full((1,)+shape, 0.8, dtype=np.float32),
               sfc_mtype=1, sfc_param=[float(rng.choice([0.0, 0.4])), 0, 0, 0, 0],
               target=int(rng.choice([TARGET_FLUX, TARGET_RADIANCE, TARGET_FLUX | TARGET_RADIANCE])),
               view_the=list(180.0-vza), view_phi=[0.0]*nv, view_zloc=list(rng.choice([1.0e6, 0.0, 0.5*dz], size=nv)), nxr=nx, nyr=ny,
               src_mtype=3, src_wlen=WL, tmp1d=rng.uniform(220.0, 300.0, nz+1), tmpa3d=rng.uniform(-5.0, 5.0, shape),
               src_the=180.0, src_qmax=0.0, solver=int(rng.choice([0, 1, 2])))
    return sc


def test_random_thermal_corner_scenes_end_and_follow_the_oracle(solver, oracle, nthreads):
    rng = np.random.default_rng(20261016)
    n = 40000
    for i in range(24):
        sc = _random_thermal_scene(rng, i)
        g = gpu_run(solver, sc, n, seed=200+i)
        c = g['counters']
        o = oracle.run(sc, n, seed=200+i, nthreads=nthreads)
        oc = o['counters']
        if oc['photons'] == 0:                    # nothing emits: both sides leave every tally 0
            assert all(np.all(g[k] == 0.0) for k in ('rad', 'flux') if k in g), i
            continue
        assert c['photons'] == n and c['killed']+c['escaped']+c['absorbed'] == n, (i, c)
        assert 'thermal' in solver.kernel_name()
        for k in ('scatter', 'surface', 'escaped'):
            assert abs(c[k]-oc[k]) <= 0.03*max(oc[k], 1) + 60, (i, k, c[k], oc[k])
        if sc.target & TARGET_RADIANCE:
            assert np.all(np.isfinite(g['rad']))
            gm, om = g['rad'].mean(axis=(1, 2)), o['rad'].mean(axis=(1, 2))
            assert np.all(np.abs(gm-om) <= 0.08*np.abs(om) + 2e-3*np.abs(om).max()), (i, gm, om)
        if sc.target & TARGET_FLUX:
            assert np.all(np.isfinite(g['flux'])) and np.all(g['flux'][0] == 0.0)
            gm, om = g['flux'].mean(axis=(2, 3)), o['flux'].mean(axis=(2, 3))
            assert np.all(np.abs(gm-om) <= 0.03*np.abs(om) + 2e-3*np.abs(om).max()), (i, np.abs(gm-om).max())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [dict(the=0.0, zloc=0.0, umax=90.0, vmax=180.0, mrproj=1),       # irradiance sensor on the ground, wrap
                                  dict(the=0.0, zloc=0.0, umax=80.0, vmax=150.0, mrproj=0),       # a narrower map, actinic weighting
                                  dict(the=155.0, zloc=3000.0, umax=80.0, vmax=180.0, mrproj=0, phi=60.0, psi=30.0),   # tilted axis
                                  dict(the=180.0, zloc=3000.0, umax=90.0, vmax=180.0, mrproj=1)])  # looking down from above the cloud
def test_rectangular_camera_images_against_the_oracle(solver, oracle, nthreads, case):
    """6 x 8 rectangular images of the cloud scene on the same photon ids: image means and per-pixel z-scores (check_radiance)"""
    sc = cameras(les_scene(nx=16, ny=16, nz3=50, surface_albedo=0.1), case['the'], case['zloc'], xpos=0.4, ypos=0.55, nxr=6, nyr=8,
                 umax=case['umax'], vmax=case['vmax'], mrproj=case['mrproj'], apsize=30.0, phi=case.get('phi', 0.0), psi=case.get('psi', 0.0))
    sc.cam_images = 0
    nb, nper = 16, 20000
    o = oracle_batches(oracle, sc, nb, nper, 23, nthreads)
    g = gpu_run(solver, sc, nb*nper, seed=23)
    check_counters(g['counters'], o['counters'])
    assert np.all(o['rad'][0] > 0.0)          # (every pixel lit: a pixel the oracle never reached has no sigma to hold the GPU to)
    check_radiance(g, o)
