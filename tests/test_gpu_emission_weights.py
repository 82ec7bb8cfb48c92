"""
Per-cell emission weights of the backward route (mi3d_set_emission_weights 1, Rad_mwgt = 1) on the GPU, on the 8 x 8 scenes
of tests/test_gpu_backward.py.  The tests are identities, not statistics: a pixel's reading is exactly linear in the cells' Planck
radiances, R_p = Src_flx sum_c K[p][c] B_c, and K does not depend on any temperature.

The identity's bound, 5 x 2^-24 of the reading: all terms are >= 0; the kernel rounds (w B) em twice in float32 where the weights route
rounds w em once (3 x 2^-24 per term), and either read-out rounds once to float32 (2 x 2^-24); measured: 3.8e-8 ... 6.5e-8 of the reading.
Per cell against the float64 march (test 3): the tolerance is 4 x the largest gap of a float32 numpy restatement, measured on the CPU in
the test: 1.29e-8 of sum K_ref on these 2000 lines, the kernel's own largest gap 1.65e-8.  Every test asserts the kernel's name and
that no history was capped, and leaves the session's solver as it found it: switch off, method 'forward', buffers unbound.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import emission_weights_ref as wref
from tests import thermal_camera_ref as ref
from tests.test_gpu_backward import ZS_ISO, TAU_TOP, cameras, iso_scene, absorbing_scene

pytestmark = pytest.mark.gpu

U24 = 2.0**-24
NAME_W, NAME_0 = 'k_backward<0,W> [thermal]', 'k_backward<0> [thermal]'


@pytest.fixture(autouse=True)
def as_found(solver):
    yield
    solver.set_emission_weights(False)
    solver.set_camera_method('forward')
    solver.bind(None, None, None)
    solver.set_tuning(batch_log2=30, wgt_stage=1)


def flat(d):
    """the three parts of emission_weights() side by side in tally order: (npix, ncell) float64, and planck (ncell,)"""
    n = d['layers'].shape[0]
    k = np.concatenate([d['voxels'].reshape(n, -1), d['layers'], d['surface'].reshape(n, -1)], axis=1).astype(np.float64)
    p = d['planck']
    return k, np.concatenate([p['voxels'].ravel(), p['layers'].ravel(), p['surface'].ravel()]).astype(np.float64)


def run(sol, sc, N, seed, on=True, offset=0):
    """the job's reading (npix,) float64 and, with the switch on, K (npix, ncell) and planck (ncell,)"""
    sol.load_scene(dataclasses.replace(sc, cam_weights=1 if on else 0)); sol.reset()
    sol.run(N, seed=seed, offset=offset)
    rad = sol.radiance(N).astype(np.float64).ravel()
    assert sol.kernel_name() == (NAME_W if on else NAME_0), sol.kernel_name()
    assert sol.debug_backward(seed, 0, 0)[2] == 0                    # no history was capped
    if not on:
        return rad
    k, b = flat(sol.emission_weights(N))
    return rad, k, b


def with_surface2d(sc, nb, seed=3):
    rng = np.random.default_rng(seed)
    psfc = np.zeros((5, nb, nb), dtype=np.float32)
    psfc[0] = rng.uniform(0.05, 0.4, (nb, nb))
    return dataclasses.replace(sc, jsfc=np.ones((nb, nb)), psfc=psfc, tmps2d=rng.uniform(-4.0, 6.0, (nb, nb)).astype(np.float32))


def four_sensors(base):
    """tests/test_gpu_backward.py: down from the gap above the cloud, up from the ground, up and down from INSIDE an absorbing voxel"""
    return cameras(base, [180.0, 0.0, 30.0, 150.0], [900.0, 100.0, 500.0, 500.0], xpos=[0.3, 0.7, 0.45, 0.45], ypos=[0.6, 0.2, 0.3, 0.3],
                   mpmap=2, mrproj=0, nxr=2, nyr=3, umax=87.0, vmax=180.0, phi=[0.0, 0.0, 70.0, 70.0])


def identity(what, sc, rad, k, b):
    back = sc.src_flx*(k @ b)
    gap = np.abs(rad-back)/np.where(rad > 0.0, rad, 1.0)
    print('%s: %d pixels, %d cells; largest |R - Src_flx sum K B| / R = %.3e (allowed %.3e)' % (what, k.shape[0], k.shape[1], gap.max(), 5.0*U24))
    assert rad.max() > 0.0 and np.all(np.abs(rad-back) <= 5.0*U24*rad), (what, gap.max(), np.argmax(gap))


# ---- 1: the identity -------------------------------------------------------------------------------------------------------------------------

def test_reading_is_the_weights_times_planck(solver):
    sc = four_sensors(absorbing_scene(0.1))
    assert sc.extp[0, 1, int(0.3*8), int(0.45*8)] > 0.001             # the third and fourth sensor stand in an absorbing voxel
    rad, k, b = run(solver, sc, 24*4000, 11)
    identity('absorbing scene', sc, rad, k, b)
    # (the nadir sensor, view 0, sees the surface in every pixel; the zenith sensor, view 1, only by reflection -- nothing scatters)
    assert np.all(rad > 0.0) and np.all(k[:, :sc.nx*sc.ny*sc.nz3].sum(axis=1) > 0.0) and np.all(k[:6, -1] > 0.0)
    nvox = sc.nx*sc.ny*sc.nz3
    assert np.all(k[:, nvox+sc.iz3l-1:nvox+sc.iz3l-1+sc.nz3] == 0.0)  # layers inside the 3-D region carry nothing: their voxels do
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=4, nyr=4, umax=180.0, vmax=180.0)
    rad, k, b = run(solver, sc, 32*3000, 13)
    identity('scattering scene (albedo 0.3)', sc, rad, k, b)
    sc = four_sensors(with_surface2d(absorbing_scene(0.1), 2))
    rad, k, b = run(solver, sc, 24*4000, 17)
    identity('2 x 2 surface with Sfc_tmps2d', sc, rad, k, b)
    assert k.shape[1] == nvox+sc.nz+4 and np.all(k[:6, -4:].sum(axis=1) > 0.0) and len(set(b[-4:])) == 4


# ---- 2: other temperatures, same histories ---------------------------------------------------------------------------------------------------

def test_other_temperatures_same_histories(solver):
    A = four_sensors(with_surface2d(absorbing_scene(0.1), 2))
    rng = np.random.default_rng(5)
    B = dataclasses.replace(A, tmp1d=np.asarray(A.tmp1d)+rng.uniform(-6.0, 6.0, A.nz+1), tmpa3d=rng.uniform(-5.0, 5.0, A.tmpa3d.shape).astype(np.float32),
                            tmps2d=rng.uniform(-8.0, 8.0, (2, 2)).astype(np.float32))
    N, seed = 24*4000, 19
    rad_a, k_a, b_a = run(solver, A, N, seed)
    rad_b = run(solver, B, N, seed, on=False)
    _, k_b, b_b = run(solver, B, N, seed)
    emits = b_a > 0.0                                                  # (the layers inside the 3-D region hold no Planck radiance: their voxels do)
    assert np.array_equal(emits, b_b > 0.0) and np.abs(b_b[emits]/b_a[emits]-1.0).max() > 0.01 and np.abs(rad_b/rad_a-1.0).max() > 0.01
    back = A.src_flx*(k_a @ b_b)
    gap = np.abs(rad_b-back)/rad_b
    print('re-evaluation: largest |R_B - Src_flx sum K_A B_B| / R_B = %.3e (allowed %.3e)' % (gap.max(), 5.0*U24))
    assert np.all(np.abs(rad_b-back) <= 5.0*U24*rad_b), gap.max()
    # K does not depend on temperature: the raw float64 tallies agree to 1e-12 (sums in another order), their float32 read-outs to the last place
    assert np.allclose(k_b, k_a, rtol=2.0**-23, atol=0.0)
    import torch
    npix, nvox, nz, nsfc = solver.weights_shape()
    raws = []
    for s in (A, B):
        buf = torch.zeros(npix*(nvox+nz+nsfc), dtype=torch.float64, device='cuda:0')
        solver.bind(None, None, None, wgt_ptr=buf.data_ptr())
        solver.load_scene(dataclasses.replace(s, cam_weights=1)); solver.reset(); solver.run(N, seed=seed); solver.sync()
        raws.append(buf.cpu().numpy().copy())
        solver.bind(None, None, None)
    assert raws[0].max() > 0.0 and np.allclose(raws[1], raws[0], rtol=1.0e-12, atol=0.0)


# ---- 3: against float64, per cell --------------------------------------------------------------------------------------------------------------

def _weights32(sc, org, dirs, ncell):
    """the kernel's per-cell terms restated in float32 (the walk of tests/test_gpu_backward._march32): w (1 - exp(-ka l)) per cell step with
    float32 ka, weights and pieces, summed per cell in float64; non-scattering scenes over a black surface"""
    f = np.float32
    ka, _, eps, _ = ref.cells(sc)
    ka = ka.astype(f)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    dzl = np.diff(zg).astype(f)
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, f(sc.dx), f(sc.dy)
    k3lo, k3hi = sc.iz3l-1, sc.iz3l-1+sc.nz3
    nvox = nx*ny*sc.nz3
    out = np.zeros(ncell)
    for o, u in zip(np.asarray(org, dtype=f), np.asarray(dirs, dtype=f)):
        k = int(np.clip(np.searchsorted(zg, float(o[2]), side='right')-1, 0, nz-1))
        if float(o[2]) == zg[k] and u[2] < 0 and k > 0:
            k -= 1
        cx, cy = np.floor(o[0]/dx), np.floor(o[1]/dy)
        px, py, pz = f(o[0]-cx*dx), f(o[1]-cy*dy), f(o[2]-f(zg[k]))
        ix, iy = int(cx) % nx, int(cy) % ny
        ax, ay, az = f(1)/max(abs(u[0]), f(1e-20)), f(1)/max(abs(u[1]), f(1e-20)), f(1)/max(abs(u[2]), f(1e-20))
        sx, sy = f(dx*ax), f(dy*ay)
        tx = f((dx-px if u[0] > 0 else px)*ax); ty = f((dy-py if u[1] > 0 else py)*ay); tz = f((dzl[k]-pz if u[2] > 0 else pz)*az)
        w = f(1)
        while True:
            in3d = k3lo <= k < k3hi
            ds = min(tx, ty, tz) if in3d else tz
            a = f(ka[k, iy, ix]*ds)
            e = np.exp(-a, dtype=f)
            em = f(-np.expm1(-a, dtype=f))
            out[((k-k3lo)*ny+iy)*nx+ix if in3d else nvox+k] += float(f(w*em))
            w = f(w*e)
            hz = (not in3d) or (tz <= tx and tz <= ty)
            hx = (not hz) and tx <= ty
            tx, ty, tz = f(tx-ds), f(ty-ds), f(tz-ds)
            if not in3d:
                if tx < 0:
                    nc = np.floor(-tx/sx)+1; tx = f(tx+f(nc)*sx); ix = int(ix+(nc if u[0] > 0 else -nc)) % nx
                if ty < 0:
                    nc = np.floor(-ty/sy)+1; ty = f(ty+f(nc)*sy); iy = int(iy+(nc if u[1] > 0 else -nc)) % ny
            if w < 1e-7:
                break
            if hz:
                k += 1 if u[2] > 0 else -1
                if k >= nz:
                    break
                if k < 0:
                    out[nvox+nz] += float(f(w*f(eps)))
                    break
                tz = f(dzl[k]*az)
            elif hx:
                tx = sx; ix = (ix+(1 if u[0] > 0 else -1)) % nx
            else:
                ty = sy; iy = (iy+(1 if u[1] > 0 else -1)) % ny
    return out/len(dirs)


def test_weights_against_the_float64_march_per_cell(solver):
    """a one-pixel sensor INSIDE an absorbing voxel of the scene that never scatters, over a black surface: a history is its line of sight"""
    sc = cameras(absorbing_scene(0.0), [150.0], [500.0], xpos=0.45, ypos=0.3, mpmap=2, mrproj=0, nxr=1, nyr=1, umax=87.0, vmax=180.0, phi=70.0)
    n, seed = 2000, 23
    rad, k, b = run(solver, sc, n, seed)
    d, score, capped = solver.debug_backward(seed, 0, n)
    assert capped == 0
    org = np.array([float(np.float32(sc.cam_xpos[0]*sc.nx*sc.dx)), float(np.float32(sc.cam_ypos[0]*sc.ny*sc.dy)), float(sc.view_zloc[0])])
    k64 = wref.line_weights(sc, org, d.astype(np.float64)).mean(axis=0)
    k32 = _weights32(sc, np.broadcast_to(org, (n, 3)), d, k64.size)
    tot = k64.sum()
    gap32 = np.abs(k32-k64).max()/tot
    gap = np.abs(k[0]-k64)/tot
    print('per cell: %d lines, %d cells, sum K_ref %.6f; float32 restatement: largest |dK_c| / sum K_ref %.3e; the kernel: %.3e (allowed %.3e)'
          % (n, k64.size, tot, gap32, gap.max(), 4.0*gap32))
    assert 0.5 < tot <= 1.0 and 1.0e-9 < gap32 < 1.0e-5 and (k64 > 0.0).sum() > 50
    assert np.all(gap <= 4.0*gap32), (gap.max(), gap32, np.argmax(gap))
    assert np.allclose(b, wref.planck_cells(sc), rtol=2.0*U24, atol=0.0)        # float64 Planck radiances rounded once


# ---- 4: sum rule ---------------------------------------------------------------------------------------------------------------------------------

def test_weights_of_a_closed_scene_sum_to_one(solver):
    """under an opaque lid and with the roulette off a history's weight ends in some cell: sum_c K[p][c] = 1 - (what the lid lets out)"""
    sc = cameras(dataclasses.replace(iso_scene(), wmin=0.0), [0.0, 180.0, 0.0, 180.0], [ZS_ISO, ZS_ISO, 250.0, 250.0],
                 xpos=[0.3, 0.3, 0.3125, 0.3125], ypos=[0.6, 0.6, 0.5625, 0.5625], mrproj=1)
    rad, k, b = run(solver, sc, 4*20000, 29)
    miss = 1.0-k.sum(axis=1)
    print('sum rule: 1 - sum_c K[p][c] = %s (allowed %.3e ... %.3e)' % (miss, -5.0*U24, np.exp(-TAU_TOP)+1.0e-6))
    assert np.all(miss >= -5.0*U24) and np.all(miss <= np.exp(-TAU_TOP)+1.0e-6), miss


# ---- 5: switch off means the parent ----------------------------------------------------------------------------------------------------------

def test_switch_off_is_the_route_without_weights(solver):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=4, nyr=4, umax=180.0, vmax=180.0)
    N, seed = 40000, 31
    off = run(solver, sc, N, seed, on=False)
    _, s_off, _ = solver.debug_backward(seed, 0, 4096)
    on, k, b = run(solver, sc, N, seed)
    _, s_on, _ = solver.debug_backward(seed, 0, 4096)
    assert off.max() > 0.0 and np.allclose(on, off, rtol=2.0e-7, atol=0.0), np.abs(on/np.where(off > 0, off, 1.0)-1.0).max()
    assert s_off.max() > 0.0 and np.array_equal(s_on, s_off)           # single histories ignore the switch: bit for bit
    again = run(solver, sc, N, seed, on=False)
    assert np.array_equal(again, off)


# ---- 6: bookkeeping ------------------------------------------------------------------------------------------------------------------------------

def _raw(solver, sc, runs, seed, **tuning):
    """raw K_raw (npix, ncell) float64 through a bound buffer after the runs [(n, offset)]; whether the launch staged its layer part in LDS"""
    import torch
    solver.load_scene(dataclasses.replace(sc, cam_weights=1))
    npix, nvox, nz, nsfc = solver.weights_shape()
    buf = torch.zeros(npix*(nvox+nz+nsfc), dtype=torch.float64, device='cuda:0')
    try:
        solver.set_tuning(**tuning)
        solver.bind(None, None, None, wgt_ptr=buf.data_ptr())
        solver.reset()
        for n, off in runs:
            solver.run(n, seed=seed, offset=off)
        solver.sync()
        assert solver.kernel_name() == NAME_W and solver.debug_backward(seed, 0, 0)[2] == 0
        return buf.cpu().numpy().reshape(npix, -1).copy(), solver.lib.mi3d_debug_weights_staged(solver._h)
    finally:
        solver.bind(None, None, None)
        solver.set_tuning(batch_log2=30, wgt_stage=1)


def test_every_row_is_divided_by_its_own_count(solver):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, nxr=5, nyr=1, umax=80.0, mrproj=0)      # ten pixels
    N, seed = 7003, 37
    raw, _ = _raw(solver, sc, [(N, 0)], seed)
    solver.load_scene(dataclasses.replace(sc, cam_weights=1)); solver.reset(); solver.run(N, seed=seed)
    k, _ = flat(solver.emission_weights(N))
    cnt = N//10+(np.arange(10) < N % 10)
    assert sorted(set(cnt)) == [700, 701] and raw.min() >= 0.0 and np.all(raw.sum(axis=1) > 0.0)
    assert np.array_equal(k, (raw/cnt[:, None]).astype(np.float32).astype(np.float64))
    solver.reset(); solver.run(4, seed=seed)
    k, _ = flat(solver.emission_weights(4))
    assert np.all(k[:4].sum(axis=1) > 0.5) and np.all(k[4:] == 0.0) and np.all(np.isfinite(k))
    assert solver.kernel_name() == NAME_W and solver.debug_backward(seed, 0, 0)[2] == 0


def test_raw_weights_add_over_id_ranges_and_launch_sizes(solver):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=3, nyr=3, umax=180.0, vmax=180.0)
    N, n1, seed = 50003, 20011, 41
    whole, _ = _raw(solver, sc, [(N, 0)], seed)
    parts, _ = _raw(solver, sc, [(n1, 0), (N-n1, n1)], seed)
    small, _ = _raw(solver, sc, [(N, 0)], seed, batch_log2=12)
    assert whole.max() > 0.0 and (whole > 0.0).sum() > 500
    assert np.allclose(parts, whole, rtol=1.0e-12, atol=0.0) and np.allclose(small, whole, rtol=1.0e-12, atol=0.0)


@pytest.mark.parametrize('shape', ['two one-pixel sensors, uniform surface', '2 x 4 x 4 pixels, 8 x 8 surface', '2 x 8 x 8 pixels, 8 x 8 surface'])
def test_lds_staging_against_global_atomics(solver, shape):
    """the layer and surface part summed per workgroup in LDS against global atomics.  The staging limit is 32 KB of dynamic LDS: the first
    two shapes lie below it (16 B and 18 KB of staged sums), the third, 128 pixels x 71 layer and surface cells x 8 B = 73 KB, above"""
    if shape.startswith('two'):
        sc, want = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6), 1
    else:
        n = 4 if '4 x 4' in shape else 8
        sc = cameras(with_surface2d(iso_scene(), 8), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=n, nyr=n, umax=180.0, vmax=180.0)
        want = 1 if n == 4 else 0
    N, seed = 60000, 43
    auto, staged = _raw(solver, sc, [(N, 0)], seed)
    glob, staged0 = _raw(solver, sc, [(N, 0)], seed, wgt_stage=0)
    assert staged == want and staged0 == 0, (shape, staged, staged0)
    nvox = sc.nx*sc.ny*sc.nz3
    assert auto[:, nvox:nvox+sc.nz].max() > 0.0 and np.all(auto[:, nvox+sc.nz:].sum(axis=0) > 0.0)      # layers and every surface cell took part
    assert np.allclose(auto, glob, rtol=1.0e-12, atol=0.0)


# ---- 8: the drop-in ------------------------------------------------------------------------------------------------------------------------------

def _reduced_identity(what, d, Ng, Nrun):
    """f / solid angle = sum_c emission_weight_c emission_planck_c for the reduced fields.  Float32 reduction steps between the jobs' own
    identities and these fields: the product with the g factor (1), the sum over g (Ng - 1), the mean over runs (Nrun - 1 sums, 1 division),
    the product with the solid angle (1), the weights' own rounding to float32 (1): Ng + Nrun + 2 steps, 5 x 2^-24 each"""
    steps = Ng+Nrun+2
    f = d['f']['data'].astype(np.float64)/float(np.float32(np.pi))
    back = sum((d['emission_weight'+s]['data'].astype(np.float64)*d['emission_planck'+s]['data'].astype(np.float64)[..., None])
               .reshape(-1, f.size).sum(axis=0) for s in ('', '_layers', '_surface'))
    gap = np.abs(back/f-1.0)
    print('%s: %d float32 reduction steps; largest |sum weight planck / rad - 1| = %.3e (allowed %.3e)' % (what, steps, gap.max(), 5.0*U24*steps))
    assert f.min() > 0.0 and np.all(gap <= 5.0*U24*steps), (what, gap)


def test_dropin_files_against_fused(tmp_path):
    import contextlib
    import copy
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner, weights_fname
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=3)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    kw = dict(Ng=3, target='radiance', surface_albedo=0.05, source='thermal', camera_method='backward', Nrun=3, photons=6e4,
              weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True, abs_obj=ab, keep_files=True,
              sensor_type='irradiance', sensor_xpos=[0.1, 0.35, 0.6, 0.85], sensor_ypos=0.5, sensor_altitude=[10.0, 700.0, 10.0, 5000.0],
              sensor_zenith_angle=[0.0, 0.0, 20.0, 180.0])
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], fdir=str(tmp_path/'wgt'), emission_weights=True, **kw)
        plain = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], fdir=str(tmp_path/'plain'), **kw)
    sol = get_runner().sol
    try:
        assert sol.kernel_name() == NAME_0 and sol.debug_backward(1, 0, 0)[2] == 0           # (the job that ran last: without weights)
        nml = mca.mca_inp_read(m.fnames_inp[0][0])
        assert nml['Rad_mwgt'] == 1 and 'Rad_mwgt' not in mca.mca_inp_read(plain.fnames_inp[0][0])
        # one extra file per job, only with the key; out.bin and .ctl list what they listed
        assert all(os.path.exists(weights_fname(f)) for row in m.fnames_out for f in row)
        assert not any(os.path.exists(weights_fname(f)) for row in plain.fnames_out for f in row)
        assert [v['name'].split()[0] for v in mca.mca_out_raw(m.fnames_out[0][0]).data] == ['rad', 'rdir']
        assert os.path.getsize(m.fnames_out[0][0]) == os.path.getsize(plain.fnames_out[0][0])
        assert sorted(f for f in os.listdir(str(tmp_path/'wgt')) if not f.endswith('.wgt.bin')) == sorted(os.listdir(str(tmp_path/'plain')))
        files = copy.copy(m); files.fused = None
        for mode in ('mean', 'all'):
            a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
            b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
            assert sorted(a.keys()) == sorted(b.keys()) and 'emission_weight' in a and 'emission_planck_surface' in a
            for k in a:
                if k.startswith('emission_'):
                    assert a[k]['data'].shape == b[k]['data'].shape and np.array_equal(a[k]['data'], b[k]['data']), (mode, k)
            if mode == 'mean':
                assert a['emission_weight']['data'].shape == (12, 10, 10, 4) and a['emission_weight_surface']['data'].shape == (1, 1, 4)
                assert a['emission_weight']['data'].max() > 0.0 and a['emission_weight_std']['data'].max() > 0.0
                _reduced_identity('fused route', a, 3, 3)
                _reduced_identity('file route', b, 3, 3)
        assert 'emission_weight' not in mca.mca_out_ng(mca_obj=plain, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    finally:
        sol.set_emission_weights(False); sol.set_camera_method('forward')


def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on the one GPU) against one rank on the same ids: the shards of [0, N) add to the
    job's raw weights, and the read-out divides by the job's counts (tests/emission_weights_dist_worker.py)"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'emission_weights_dist_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(str(tmp_path), 'result.npz'))
    assert str(z['kernel']) == NAME_W and int(z['capped']) == 0
    a, b = z['job_dist_wgt'].astype(np.float64), z['job_solo_wgt'].astype(np.float64)
    assert a.shape == b.shape == (4, 12*10*10+28+1) and b.max() > 0.0 and np.allclose(a, b, rtol=2.0e-7, atol=0.0), np.abs(a-b).max()
    assert np.array_equal(z['job_dist_planck'], z['job_solo_planck'])
    rad = z['job_solo_rad'].astype(np.float64)
    assert np.all(np.abs(b @ z['job_solo_planck'].astype(np.float64)-rad) <= 5.0*U24*rad)
    for tag in ('file', 'fused'):
        d = {'f': {'data': z[tag+'_f']}}
        for s in ('', '_layers', '_surface'):
            d['emission_weight'+s] = {'data': z[tag+'_weight'+s]}; d['emission_planck'+s] = {'data': z[tag+'_planck'+s]}
        _reduced_identity('two ranks, %s route' % tag, d, 2, 2)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refusals(solver):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6)
    solver.load_scene(dataclasses.replace(sc, cam_method=0))
    solver.set_emission_weights(True)
    rc = solver.lib.mi3d_run(solver._h, 1000, 1, 0)
    msg = solver.lib.mi3d_last_error().decode()
    assert rc == -4 and 'mi3d_set_emission_weights' in msg, (rc, msg)
    with pytest.raises(ValueError):
        dataclasses.replace(sc, cam_method=0, cam_weights=1)
    # what the backward route refuses is still refused, with the same words (tests/test_gpu_backward.py)
    lsrt = dataclasses.replace(sc, sfc_mtype=4, sfc_param=np.array([0.1, 0.05, 0.02, 0, 0], dtype=np.float32))
    cases = [(dataclasses.replace(sc, src_mtype=1, cam_method=0), 'solar'),
             (dataclasses.replace(sc, src_mtype=2, src_fsol=5.0, src_the=150.0, cam_method=0), 'solar+thermal'),
             (dataclasses.replace(sc, solver=2), 'independent columns'),
             (dataclasses.replace(sc, solver=1), 'partial 3-D'),
             (lsrt, 'Lambertian')]
    for s, word in cases:
        try:
            solver.load_scene(s)
        except OSError:
            pass
        solver.set_camera_method('backward')
        solver.set_emission_weights(True)
        rc = solver.lib.mi3d_run(solver._h, 1000, 1, 0)
        msg = solver.lib.mi3d_last_error().decode()
        # (mi3d_prepare refuses the LSRT surface of a thermal job before the route is asked)
        assert rc == -4 and word in msg and (s is lsrt or msg.startswith('backward Monte Carlo (mi3d_set_camera_method 1) does not serve')), (word, rc, msg)
    # npix x ncell over 2^31: a large polar image on the tiny grid; refused before the tally is made
    big = cameras(iso_scene(), [0.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=2900, nyr=2900, umax=180.0, vmax=180.0)
    solver.load_scene(dataclasses.replace(big, cam_weights=1))
    rc = solver.lib.mi3d_run(solver._h, 1000, 1, 0)
    msg = solver.lib.mi3d_last_error().decode()
    assert rc == -4 and str(2900*2900) in msg and str(8*8*5+7+1) in msg, (rc, msg)
    solver.load_scene(dataclasses.replace(sc, cam_weights=1)); solver.reset(); solver.run(1000, seed=1)
    assert solver.kernel_name() == NAME_W and solver.radiance(1000).min() > 0.0 and solver.debug_backward(1, 0, 0)[2] == 0
