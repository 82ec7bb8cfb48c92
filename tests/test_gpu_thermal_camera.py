"""
Cameras and point radiometers of thermal jobs (Src_mtype = 3, Rad_mrkind = 1) on the GPU.  The oracle refuses the
combination, so the tests rest on closed forms (an isothermal scene glows at B(T)), on an independent float64 line integral
(tests/thermal_camera_ref.py) and on the oracle's flux planes, which it does serve for thermal jobs.

Every statistical comparison: batches of the same job over disjoint photon-id ranges, allowance 4 batch standard errors of the quantity
compared plus the bounds derived in the test from the geometry; each such test also asserts that its own 4 se is below 5 % of the value
expected (a lost cosine, pi for 4 pi, mu0 for P_tot / (Lx Ly) are all >= 10 % in these scenes).

Truncation.  dz: the vertical distance from the sensor to the far boundary it looks at, N = cam_images.  Every line of sight with
tan(theta) <= t_c = (N + 1/2) min(Lx, Ly) / dz is served completely and a truncated one loses at most its whole value: the estimate is
never high and low by at most cos^2(theta_c) = 1 / (1 + t_c^2) of a hemispheric irradiance, cos(theta_c) of an actinic flux.

Sensors sit in the middle of a layer with no extinction: the local estimate carries 1 / r^2, and events in a medium around the sensor
would make the batch standard error heavy-tailed (bounded by the Rad_apsize clamp only).
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE
from er3t_amd.thermal import planck, brightness_temperature
from tests import thermal_camera_ref as ref

pytestmark = pytest.mark.gpu

WL = 11.0     # um


def cameras(base, the, zloc, xpos=0.5, ypos=0.5, mpmap=2, mrproj=1, nxr=1, nyr=1, umax=90.0, vmax=180.0, qmax=180.0, apsize=0.05,
            phi=0.0, psi=0.0, images=-1):
    the = list(np.atleast_1d(np.asarray(the, dtype=float)))
    n = len(the)
    per = lambda v: list(np.resize(np.atleast_1d(np.asarray(v, dtype=float)), n))
    return dataclasses.replace(base, target=TARGET_RADIANCE, rad_kind=1, view_the=the, view_phi=per(phi), view_zloc=per(zloc),
                               cam_xpos=per(xpos), cam_ypos=per(ypos), cam_psi=per(psi), cam_qmax=per(qmax), cam_umax=per(umax),
                               cam_vmax=per(vmax), cam_apsize=per(apsize), nxr=nxr, nyr=nyr, cam_mpmap=mpmap, cam_mrproj=mrproj,
                               cam_images=images)


def batches(sol, scene, nb, nper, seed):
    """nb batches over disjoint photon-id ranges: mean image and standard error of that mean, (nview, nyr, nxr)"""
    sol.load_scene(scene)
    out = []
    for b in range(nb):
        sol.reset()
        sol.run(nper, seed=seed, offset=b*nper)
        out.append(sol.radiance(nper).astype(np.float64))
    a = np.array(out)
    return a.mean(axis=0), a.std(axis=0, ddof=1)/np.sqrt(nb)


def t_crit(scene, nimg, dz):
    return (nimg+0.5)*min(scene.nx*scene.dx, scene.ny*scene.dy)/dz


# ---- 1: an isothermal scene glows at B(T) in every direction ------------------------------------------------------------------------------

ZS_ISO = 350.0
TAU_TOP = 8.0      # of the opaque layer on top of the isothermal scene: what it lets in from cold space is below exp(-TAU_TOP) of B


def iso_scene(T=285.0, n=8, dx=250.0, tlev=None):
    """seven layers of 100 m: an absorbing 1-D layer (tau 0.5) over the surface; a 3-D region of five layers, a checkerboard of scattering,
    partly absorbing cloud (omega 0.7, g 0.85, tau 2 per cloudy cell) in four of them and NO extinction in the middle one (the gap the
    sensors sit in, z = 300 ... 400 m); an opaque absorbing 1-D layer on top (TAU_TOP: the sky is as warm as the scene).  Everything at T."""
    nz, dz = 7, 100.0
    absk = np.zeros(nz); absk[0] = 0.005; absk[-1] = TAU_TOP/dz
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    ext = np.zeros((1, 5, n, n), dtype=np.float32)
    for k3 in (0, 1, 3, 4):
        ext[0, k3] = 0.02*((xx+yy+k3) % 2)
    tl = np.full(nz+1, T) if tlev is None else np.asarray(tlev, dtype=np.float64)
    return Scene(zgrd=np.arange(nz+1)*dz, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=n, ny=n, dx=dx, dy=dx,
                 nz3=5, iz3l=2, extp=ext, omgp=np.full_like(ext, 0.7), apfp=np.full_like(ext, 0.85), sfc_mtype=1, sfc_param=[0.3, 0, 0, 0, 0],
                 target=TARGET_RADIANCE, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=n, nyr=n, src_mtype=3, src_wlen=WL,
                 tmp1d=tl, src_the=180.0, src_qmax=0.0)


def test_isothermal_scene_glows_at_planck(solver):
    """up- and down-looking irradiance and actinic sensors off-centre in the gap read pi B and 2 pi B; a polar image reads B in every
    pixel that lies inside theta_c.  Holds src_amp, 1 / W, 1 / r^2, the emission of volume and surface, the scattering events of a
    thermal photon and the enumeration of the images."""
    T, N = 285.0, 2
    B = float(planck(WL, T))
    base = iso_scene(T)
    ztoa = float(base.zgrd[-1])
    for mrproj, k, low in ((1, np.pi, lambda tc: 1.0/(1.0+tc*tc)), (0, 2.0*np.pi, lambda tc: 1.0/np.sqrt(1.0+tc*tc))):
        sc = cameras(base, [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mrproj=mrproj, images=N)
        m, e = batches(solver, sc, 16, 10000000, 31+mrproj)
        name = solver.kernel_name()
        assert name.endswith('+ k_rays') and '[thermal]' in name, name
        assert np.all(solver.camera_direct() == 0.0)
        for iv, dz in ((0, ztoa-ZS_ISO), (1, ZS_ISO)):
            tc = t_crit(sc, N, dz)
            assert tc >= 14.0
            f, se4, want = k*m[iv, 0, 0], 4.0*k*e[iv, 0, 0], k*B
            print('isothermal: mrproj %d view %d: %.5f, expected %.5f, 4 se %.5f, truncation bound %.5f' % (mrproj, iv, f, want, se4, low(tc)*want))
            assert se4 < 0.05*want, (mrproj, iv, se4, want)
            leak = np.exp(-TAU_TOP)*want if iv == 0 else 0.0
            assert -(se4+low(tc)*want+leak) <= f-want <= se4, (mrproj, iv, f, want, se4)
    # a polar image of 4 x 4 pixels over the hemisphere: pixel (j, i) spans 45 degrees of U and of V
    n = 4
    sc = cameras(base, [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=n, nyr=n, umax=180.0, vmax=180.0, images=N)
    m, e = batches(solver, sc, 16, 60000000, 37)
    assert solver.kernel_name().endswith('+ k_rays')
    edge = np.maximum(np.abs(np.arange(n)/n-0.5), np.abs((np.arange(n)+1.0)/n-0.5))*180.0      # the far edge of every pixel column / row [deg]
    far = np.hypot(edge[None, :], edge[:, None])                                               # ... the far corner's angle off the axis
    for iv, dz in ((0, ztoa-ZS_ISO), (1, ZS_ISO)):
        inside = far <= np.degrees(np.arctan(t_crit(sc, N, dz)))
        assert inside.sum() == 4
        print('isothermal: polar image %d / B:\n%s\n4 se / B:\n%s' % (iv, np.round(m[iv]/B, 4), np.round(4.0*e[iv]/B, 4)))
        assert np.all(4.0*e[iv][inside] < 0.05*B)
        leak = np.exp(-TAU_TOP)*B if iv == 0 else 0.0
        assert np.all((m[iv]-B)[inside] <= 4.0*e[iv][inside]) and np.all((B-m[iv])[inside] <= 4.0*e[iv][inside]+leak), (iv, (m[iv]/B)[inside], (4.0*e[iv]/B)[inside])


# ---- 2: a non-scattering 3-D scene against a line integral, cam_images 0, 1 and 2 ----------------------------------------------------------

def absorbing_scene():
    """six layers of 200 m: an empty one over the surface (the sensor on the ground sits in its middle), three layers of an absorbing
    checkerboard (omega = 0; tau 0.24 per cloudy cell and layer, 0.04 per clear one: thin enough that the far images matter) with voxel
    temperature anomalies, an empty gap (the sensor above the cloud), an absorbing 1-D layer; a lapse rate; a warm surface of emissivity 0.9"""
    nz, dz, n, dx = 6, 200.0, 8, 250.0
    absk = np.zeros(nz); absk[-1] = 0.0003
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    ext = np.zeros((1, 3, n, n), dtype=np.float32)
    tmpa = np.zeros((3, n, n), dtype=np.float32)
    for k3 in range(3):
        blk = ((xx//2+yy//2+k3) % 2)
        ext[0, k3] = 0.0002+0.0010*blk
        tmpa[k3] = -3.0*blk
    tlev = np.array([300.0, 291.0, 289.0, 287.0, 285.0, 283.0, 281.0])
    return Scene(zgrd=np.arange(nz+1)*dz, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=n, ny=n, dx=dx, dy=dx,
                 nz3=3, iz3l=2, extp=ext, omgp=np.zeros_like(ext), apfp=np.zeros_like(ext), tmpa3d=tmpa, sfc_mtype=1, sfc_param=[0.1, 0, 0, 0, 0],
                 target=TARGET_RADIANCE, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=n, nyr=n, src_mtype=3, src_wlen=WL,
                 tmp1d=tlev, src_the=180.0, src_qmax=0.0)


def absorbing_cameras(images):
    """view 0 looks down from the gap above the cloud, view 1 up from the ground: 2 rings x 3 sectors out to 87 degrees off the axis"""
    return cameras(absorbing_scene(), [180.0, 0.0], [900.0, 100.0], xpos=[0.3, 0.7], ypos=[0.6, 0.2], mpmap=2, mrproj=0, nxr=2, nyr=3,
                   umax=87.0, vmax=180.0, images=images)


@pytest.fixture(scope='module')
def line_integrals():
    """the reference images for cam_images 0, 1, 2 and the quadrature's error: the change under doubling the sub-directions of a pixel
    (and, with them, the quadrature of the irradiance the surface reflects)"""
    out = {}
    coarse, fine = ref.surface_reflection(absorbing_scene(), 16, 6, 12), ref.surface_reflection(absorbing_scene(), 32, 12, 24)
    for N in (0, 1, 2):
        sc = absorbing_cameras(N)
        a = np.array([ref.rect_image(sc, iv, N, 16, coarse) for iv in range(2)])
        b = np.array([ref.rect_image(sc, iv, N, 32, fine) for iv in range(2)])
        out[N] = (b, np.abs(b-a))
    return out


@pytest.mark.parametrize('images, general', [(0, False), (1, False), (2, False), (0, True)])
def test_absorbing_scene_against_the_line_integral(solver, line_integrals, images, general):
    """every pixel against ITS OWN truncated integral: this holds the image box itself; cam_images = 0 on the fallback route too"""
    want, qerr = line_integrals[images]
    if images > 0:         # (the box matters: the outer ring of a wider box sees more)
        assert np.all(want[:, :, 1] > line_integrals[images-1][0][:, :, 1]*1.01)
    sc = absorbing_cameras(images)
    try:
        solver.set_kernel(general=general)
        m, e = batches(solver, sc, 8, 500000, 41+images)
        name = solver.kernel_name()
    finally:
        solver.set_kernel()
    assert name.startswith('k_transport<') and '[thermal]' in name and name.endswith('+ k_rays') != general, name
    print('absorbing scene, cam_images %d (%s):\n got / want\n%s\n 4 se / want\n%s\n quadrature / want\n%s'
          % (images, name, np.round(m/want, 4), np.round(4.0*e/want, 4), np.round(qerr/want, 5)))
    assert np.all(4.0*e+qerr < 0.05*want), ((4.0*e+qerr)/want)
    assert np.all(np.abs(m-want) <= 4.0*e+qerr), ((m-want)/want, (4.0*e+qerr)/want)


# ---- 3: scattering, against the oracle's flux planes ----------------------------------------------------------------------------------------

def scattering_slab(target):
    """a horizontally uniform scattering and absorbing slab with a lapse rate and an empty gap layer at mid-height (the lowest layer is
    carried by a 2 x 2 voxel grid holding the same medium); 40 km wide"""
    nz, dz, n, dx = 5, 800.0, 2, 20000.0
    ext = np.full(nz, 2.5e-4); ext[2] = 0.0
    ext1 = ext.copy(); ext1[0] = 0.0
    v = np.full((1, 1, n, n), ext[0], dtype=np.float32)
    return Scene(zgrd=np.arange(nz+1)*dz, ext1d=ext1, omg1d=np.full(nz, 0.6), apf1d=np.full(nz, 0.7), abs1d=np.zeros(nz), nx=n, ny=n, dx=dx, dy=dx,
                 nz3=1, iz3l=1, extp=v, omgp=np.full_like(v, 0.6), apfp=np.full_like(v, 0.7), sfc_mtype=1, sfc_param=[0.2, 0, 0, 0, 0],
                 target=target, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=n, nyr=n, src_mtype=3, src_wlen=WL,
                 tmp1d=np.linspace(295.0, 265.0, nz+1), src_the=180.0, src_qmax=0.0)


def test_scattering_slab_against_the_oracles_flux_planes(solver, oracle, nthreads):
    """an up- and a down-looking irradiance sensor in the gap against the oracle's domain-mean f_down and f_up at the gap's interfaces"""
    N, zs, nb, nper = 2, 2000.0, 8, 400000
    fl = []
    fs = scattering_slab(TARGET_FLUX)
    for b in range(nb):
        f = oracle.run(fs, nper, seed=53, offset=b*nper, nthreads=nthreads)['flux'].astype(np.float64)
        fl.append([f[1, 2:4].mean(), f[2, 2:4].mean()])          # (no extinction in the gap: the two interfaces carry the same flux)
    fl = np.array(fl)
    fo, fe = fl.mean(axis=0), fl.std(axis=0, ddof=1)/np.sqrt(nb)
    sc = cameras(scattering_slab(TARGET_RADIANCE), [0.0, 180.0], zs, xpos=0.3, ypos=0.6, mrproj=1, images=N)
    m, e = batches(solver, sc, nb, nper, 59)
    assert solver.kernel_name().endswith('+ k_rays'), solver.kernel_name()
    Bmax = float(planck(WL, 295.0))
    for iv, dz in ((0, float(sc.zgrd[-1])-zs), (1, zs)):
        tc = t_crit(sc, N, dz)
        f, se4, low = np.pi*m[iv, 0, 0], 4.0*np.hypot(np.pi*e[iv, 0, 0], fe[iv]), np.pi*Bmax/(1.0+tc*tc)
        print('slab: view %d: sensor %.5f, oracle %.5f, 4 se %.5f, truncation bound %.5f' % (iv, f, fo[iv], se4, low))
        assert se4 < 0.05*fo[iv]
        assert -(se4+low) <= f-fo[iv] <= se4, (iv, f, fo[iv], se4, low)


# ---- 4: two routes, same photon ids ---------------------------------------------------------------------------------------------------------

def test_ray_kernel_route_against_the_general_loop(solver):
    """cam_images = 0: the event-writing loop + k_rays against the general loop with the rays in the photons' lanes, same photon ids"""
    sc = cameras(iso_scene(tlev=np.linspace(295.0, 274.0, 8)), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=8, nyr=8,
                 umax=180.0, vmax=180.0, images=0)
    nph = 400000
    res = {}
    solver.set_counting(True)
    try:
        for general in (False, True):
            solver.set_kernel(general=general)
            solver.load_scene(sc); solver.reset(); solver.run(nph, seed=61)
            res[general] = (solver.radiance(nph).astype(np.float64), solver.counters(), solver.kernel_name())
    finally:
        solver.set_kernel(); solver.set_counting(False)
    (ra, ca, na), (rb, cb, nb_) = res[False], res[True]
    assert na.endswith('+ k_rays') and '[thermal]' in na and nb_.startswith('k_transport<') and not nb_.endswith('k_rays'), (na, nb_)
    for key in ('photons', 'scatter', 'surface', 'roulette', 'killed', 'escaped', 'absorbed'):
        assert ca[key] == cb[key] and (ca[key] > 0 or key == 'escaped'), (key, ca[key], cb[key])
    assert ca['photons'] == nph
    for iv in range(2):
        assert ra[iv].mean() > 0.0 and abs(ra[iv].mean()-rb[iv].mean()) < 5.0e-3*rb[iv].mean(), (iv, ra[iv].mean(), rb[iv].mean())


# ---- 5: raw tallies and the C-ABI surface ---------------------------------------------------------------------------------------------------

def test_raw_tallies_add_and_refusals(solver, capfd):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mrproj=1, images=1)
    n1, n2 = 30000, 50000
    solver.load_scene(sc); solver.reset()
    solver.run(n1+n2, seed=67)
    whole = solver.radiance(n1+n2).astype(np.float64)
    solver.reset()
    solver.run(n1, seed=67); solver.run(n2, seed=67, offset=n1)
    parts = solver.radiance(n1+n2).astype(np.float64)
    assert whole.min() > 0.0 and np.allclose(parts, whole, rtol=1.0e-5, atol=0.0), (parts, whole)
    assert np.all(solver.camera_direct() == 0.0)
    # a third 3-D constituent: the lean limits do not hold -- the general loop serves the nearest image, and says so
    e3 = np.concatenate([sc.extp, 0.1*sc.extp, 0.1*sc.extp]); o3 = np.concatenate([sc.omgp]*3); a3 = np.concatenate([sc.apfp]*3)
    three = dataclasses.replace(sc, extp=e3, omgp=o3, apfp=a3, cam_images=-1)
    from er3t_amd.solver import Mi3dSolver
    sol = Mi3dSolver(device=0)               # (a handle of its own: the warning is given once per handle)
    try:
        capfd.readouterr()
        sol.load_scene(three); sol.reset(); sol.run(20000, seed=3)
        assert sol.kernel_name().startswith('k_transport<') and '[thermal]' in sol.kernel_name() and sol.radiance(20000).max() > 0.0
        assert 'NEAREST periodic image' in capfd.readouterr().err
        sol.load_scene(dataclasses.replace(three, cam_images=2)); sol.reset()
        assert sol.lib.mi3d_run(sol._h, 20000, 3, 0) == -4 and 'cam_images=2' in sol.lib.mi3d_last_error().decode()
        # solar+thermal with a camera: refused as before
        mix = dataclasses.replace(sc, src_mtype=2, src_fsol=5.0, src_the=150.0)
        sol.load_scene(mix); sol.reset()
        assert sol.lib.mi3d_run(sol._h, 1000, 1, 0) == -4 and 'Src_mtype=2' in sol.lib.mi3d_last_error().decode()
    finally:
        sol.close()


# ---- 6: the drop-in -------------------------------------------------------------------------------------------------------------------------

def _dropin(tmp_path, name, **kw):
    import contextlib
    import copy
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=3)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=3, target='radiance', surface_albedo=0.05, source='thermal',
                           fdir=str(tmp_path/name), Nrun=3, photons=2e5, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py',
                           overwrite=True, date=gin.DATE, quiet=True, abs_obj=ab, keep_files=True, **kw)
    assert m.fused is not None and all(os.path.exists(f) for row in m.fnames_out for f in row)
    files = copy.copy(m); files.fused = None
    return mca, m, files, ab, atm


def test_dropin_allsky_and_irradiance_sensors(tmp_path):
    """mcarats_ng + mca_out_ng for a thermal all-sky image and four irradiance sensors: files and fused statistics agree, as
    tests/test_gpu_camera_routes.py holds the solar ones"""
    from er3t_amd.rtm.mca.mca_exe import get_runner
    mca, m, files, ab, atm = _dropin(tmp_path, 'allsky', sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0)
    name = get_runner().sol.kernel_name()
    assert name.endswith('+ k_rays') and '[thermal]' in name, name
    assert mca.mca_inp_read(m.fnames_inp[0][0])['Rad_nimg'] == 2
    a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert sorted(a.keys()) == sorted(b.keys()) and 'bt' in a
    for k in ('rad', 'rad_std', 'bt'):
        assert a[k]['data'].shape == b[k]['data'].shape == (500, 500) and np.array_equal(a[k]['data'], b[k]['data']), k
    t = np.asarray(atm.lev['temperature']['data'], dtype=np.float64)
    # (the sky seen from the ground at 11 um is no warmer than the warmest air: the mean over the middle of the image -- single pixels are noise)
    mid = float(a['rad']['data'].astype(np.float64)[100:400, 100:400].mean())
    assert mid > 0.0 and brightness_temperature(WL, mid*1.0e3) < t.max(), (mid, t.max())
    assert len(mca.mca_out_raw(m.fnames_out[0][0]).data) == 1
    mca, m, files, ab, atm = _dropin(tmp_path, 'irr', sensor_type='irradiance', sensor_xpos=[0.1, 0.35, 0.6, 0.85], sensor_ypos=0.5,
                                     sensor_altitude=[10.0, 10.0, 10.0, 5000.0], sensor_zenith_angle=[0.0, 0.0, 20.0, 180.0], camera_images=1)
    assert mca.mca_inp_read(m.fnames_inp[0][0])['Rad_nimg'] == 1
    raw = mca.mca_out_raw(m.fnames_out[0][0])
    assert [v['name'].split()[0] for v in raw.data] == ['rad', 'rdir'] and np.all(raw.data[1]['data'] == 0.0)
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys())
        for k in ('f', 'f_diffuse', 'f_direct'):
            x, y = a[k]['data'], b[k]['data']
            assert x.shape == y.shape and x.shape[0] == 4, (mode, k)
            assert np.allclose(x, y, rtol=2e-5, atol=0.0), (mode, k, x, y)
        assert np.all(a['f_direct']['data'] == 0.0) and np.all(b['f_direct']['data'] == 0.0)
        assert np.array_equal(a['f']['data'], a['f_diffuse']['data'])
    f = b['f']['data'][:, 0]
    # pyrgeometers on the ground read less than pi B of the warmest air (their mean: a sensor inside absorbing air has heavy-tailed noise)
    assert np.all(f > 0.0) and f[:3].mean()*1.0e3 < np.pi*planck(WL, t.max())


def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on this box's one GPU) against one rank on the same photon ids: thermal
    irradiance sensors go job by job on the file route, and through the fused route (tests/thermal_camera_dist_worker.py)"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'thermal_camera_dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(out, 'result.npz'))
    a, b = z['job_dist_rad'], z['job_solo_rad']
    assert a.shape == b.shape == (4,) and a.min() > 0.0 and np.allclose(a, b, rtol=2e-3, atol=0.0), (a, b)
    assert np.all(z['job_dist_rdir'] == 0.0) and np.all(z['job_solo_rdir'] == 0.0)
    for v in ('f', 'f_diffuse'):
        a, b = z['file_'+v], z['fused_'+v]
        assert a.shape == b.shape == (4,) and np.allclose(a, b, rtol=0.1, atol=0.0), (v, a, b)                    # different seeds
    assert np.all(z['file_f_direct'] == 0.0) and np.all(z['fused_f_direct'] == 0.0)
    assert bool(z['batched_refused'])
