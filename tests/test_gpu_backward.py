"""
Backward Monte Carlo for the cameras and point radiometers of thermal jobs (mi3d_set_camera_method 1, Rad_mbwd = 1) on
the GPU.  The scenes are the 8 x 8 grids of tests/test_gpu_thermal_camera.py, rebuilt here; the references are the closed form of an
isothermal scene, the float64 line integral of tests/thermal_camera_ref.py, the oracle's flux planes and the forward route.

Every statistical comparison: 16 batches over disjoint id ranges whose size is a multiple of npix, allowance 4 batch standard errors
plus the bounds derived in the test; each asserts that its 4 se is below 5 % of the value expected (the two comparisons with the forward
route assert it of the backward reading: at the 2e6 histories a test may take, the forward route's own 4 se is 3 % on the absorbing scene
and 9 % on the slab with tables).  Every test asserts the kernel's name and that no history was capped.

Single histories (test 2): the tolerance is 4 x the largest relative gap between a float32 restatement of the kernel's sum (numpy, the
incremental walk, float32 weights and pieces) and the float64 march over the same lines, measured on the CPU in the test: 4.5e-7
on these 2016 lines, i.e. an allowance of 1.8e-6; the kernel's own largest gap was 3.6e-7.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE
from er3t_amd.thermal import planck
from tests import thermal_camera_ref as ref

pytestmark = pytest.mark.gpu

WL = 11.0
ZS_ISO = 350.0
TAU_TOP = 8.0


def cameras(base, the, zloc, xpos=0.5, ypos=0.5, mpmap=2, mrproj=1, nxr=1, nyr=1, umax=90.0, vmax=180.0, qmax=180.0, phi=0.0, psi=0.0,
            method=1, images=-1):
    the = list(np.atleast_1d(np.asarray(the, dtype=float)))
    n = len(the)
    per = lambda v: list(np.resize(np.atleast_1d(np.asarray(v, dtype=float)), n))
    return dataclasses.replace(base, target=TARGET_RADIANCE, rad_kind=1, view_the=the, view_phi=per(phi), view_zloc=per(zloc),
                               cam_xpos=per(xpos), cam_ypos=per(ypos), cam_psi=per(psi), cam_qmax=per(qmax), cam_umax=per(umax),
                               cam_vmax=per(vmax), cam_apsize=per(0.05), nxr=nxr, nyr=nyr, cam_mpmap=mpmap, cam_mrproj=mrproj,
                               cam_method=method, cam_images=images)


def iso_scene(T=285.0, n=8, dx=250.0):
    """tests/test_gpu_thermal_camera.py: an absorbing 1-D layer, five 3-D layers with a checkerboard of scattering, partly absorbing cloud
    in four of them and an empty gap (300 ... 400 m), an opaque 1-D layer on top; everything at T; surface albedo 0.3"""
    nz, dz = 7, 100.0
    absk = np.zeros(nz); absk[0] = 0.005; absk[-1] = TAU_TOP/dz
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    ext = np.zeros((1, 5, n, n), dtype=np.float32)
    for k3 in (0, 1, 3, 4):
        ext[0, k3] = 0.02*((xx+yy+k3) % 2)
    return Scene(zgrd=np.arange(nz+1)*dz, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=n, ny=n, dx=dx, dy=dx,
                 nz3=5, iz3l=2, extp=ext, omgp=np.full_like(ext, 0.7), apfp=np.full_like(ext, 0.85), sfc_mtype=1, sfc_param=[0.3, 0, 0, 0, 0],
                 target=TARGET_RADIANCE, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=n, nyr=n, src_mtype=3, src_wlen=WL,
                 tmp1d=np.full(nz+1, T), src_the=180.0, src_qmax=0.0)


def absorbing_scene(albedo=0.1):
    """tests/test_gpu_thermal_camera.py: an empty layer over the surface, three layers of an absorbing checkerboard with voxel temperature
    anomalies, an empty gap, an absorbing 1-D layer; a lapse rate; a warm surface"""
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
                 nz3=3, iz3l=2, extp=ext, omgp=np.zeros_like(ext), apfp=np.zeros_like(ext), tmpa3d=tmpa, sfc_mtype=1, sfc_param=[albedo, 0, 0, 0, 0],
                 target=TARGET_RADIANCE, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=n, nyr=n, src_mtype=3, src_wlen=WL,
                 tmp1d=tlev, src_the=180.0, src_qmax=0.0)


def scattering_slab(target, tables=False):
    """tests/test_gpu_thermal_camera.py: a horizontally uniform scattering and absorbing slab with a lapse rate and an empty gap layer at
    mid-height, the lowest layer carried by 2 x 2 voxels.  tables: the medium's phase function tabulated (Henyey-Greenstein g = 0.7 on a
    one-degree grid) and a thin Rayleigh constituent beside it in the 1-D layers"""
    nz, dz, n, dx = 5, 800.0, 2, 20000.0
    ext = np.full(nz, 2.5e-4); ext[2] = 0.0
    ext1 = ext.copy(); ext1[0] = 0.0
    v = np.full((1, 1, n, n), ext[0], dtype=np.float32)
    kw = dict(ext1d=ext1, omg1d=np.full(nz, 0.6), apf1d=np.full(nz, 0.7), apfp=np.full_like(v, 0.7))
    if tables:
        ang = np.arange(181.0)
        g = 0.7
        pha = (1.0-g*g)/(1.0+g*g-2.0*g*np.cos(np.radians(ang)))**1.5
        ray = np.full(nz, 2.0e-5); ray[2] = 0.0
        kw = dict(ext1d=np.stack([ext1, ray]), omg1d=np.stack([np.full(nz, 0.6), np.ones(nz)]), apf1d=np.stack([np.full(nz, 1.0), np.full(nz, -1.0)]),
                  apfp=np.full_like(v, 1.0), ang=ang, pha=pha[None])
    return Scene(zgrd=np.arange(nz+1)*dz, abs1d=np.zeros(nz), nx=n, ny=n, dx=dx, dy=dx, nz3=1, iz3l=1, extp=v, omgp=np.full_like(v, 0.6),
                 sfc_mtype=1, sfc_param=[0.2, 0, 0, 0, 0], target=target, view_the=[180.0], view_phi=[0.0], view_zloc=[1.0e6], nxr=n, nyr=n,
                 src_mtype=3, src_wlen=WL, tmp1d=np.linspace(295.0, 265.0, nz+1), src_the=180.0, src_qmax=0.0, **kw)


def batches(sol, scene, nb, nper, seed, name='k_backward<0> [thermal]'):
    """nb batches over disjoint id ranges: mean image and standard error of that mean, (nview, nyr, nxr)"""
    sol.load_scene(scene)
    out = []
    for b in range(nb):
        sol.reset()
        sol.run(nper, seed=seed, offset=b*nper)
        out.append(sol.radiance(nper).astype(np.float64))
        if name is not None:
            assert sol.kernel_name() == name, sol.kernel_name()
            assert sol.debug_backward(seed, 0, 0)[2] == 0          # no history was capped
    a = np.array(out)
    return a.mean(axis=0), a.std(axis=0, ddof=1)/np.sqrt(nb)


@pytest.fixture(autouse=True)
def forward_again(solver):
    yield
    solver.set_camera_method('forward')


# ---- 1: directions ----------------------------------------------------------------------------------------------------------------------------

def _camera_angles(sc, d, pix):
    """theta, phi of the directions d (n, 3) in the axes of the camera each belongs to (float64, from the scene's angles)"""
    iv = pix//(sc.nxr*sc.nyr)
    th, ph = np.zeros(len(d)), np.zeros(len(d))
    for v in range(sc.nview):
        X, Y, Z = ref.camera_axes(sc.view_the[v], sc.view_phi[v], sc.cam_psi[v])
        m = iv == v
        x, y, z = d[m] @ X, d[m] @ Y, d[m] @ Z
        th[m] = np.arctan2(np.hypot(x, y), z); ph[m] = np.arctan2(y, x)
    return th, ph


EDGE = 1.0e-5      # pixels: a float32 direction (2^-24 per component) sits this close to where float64 would put it, with room to spare


@pytest.mark.parametrize('mpmap, mrproj', [(2, 0), (2, 1), (1, 0)])
def test_directions_lie_in_their_pixels_with_the_pixels_weight(solver, mpmap, mrproj):
    if mpmap == 2:
        sc = cameras(absorbing_scene(0.0), [180.0, 30.0], [900.0, 100.0], xpos=[0.3, 0.7], ypos=[0.6, 0.2], mpmap=2, mrproj=mrproj, nxr=2, nyr=3,
                     umax=87.0, vmax=180.0, phi=[0.0, 40.0], psi=[0.0, 25.0])
    else:
        sc = cameras(absorbing_scene(0.0), [180.0, 30.0], [900.0, 100.0], xpos=[0.3, 0.7], ypos=[0.6, 0.2], mpmap=1, mrproj=0, nxr=4, nyr=4,
                     umax=180.0, vmax=180.0, phi=[0.0, 40.0], psi=[0.0, 25.0])
    npix = sc.nview*sc.nxr*sc.nyr
    n_p = 2000
    n = npix*n_p
    solver.load_scene(sc); solver.reset()
    d, score, capped = solver.debug_backward(71, 0, n)
    assert capped == 0 and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=3e-7)
    pix = np.arange(n) % npix
    jr, ir = (pix % (sc.nxr*sc.nyr))//sc.nxr, pix % sc.nxr
    th, ph = _camera_angles(sc, d.astype(np.float64), pix)
    umax, vmax = np.radians(sc.cam_umax[0]), np.radians(sc.cam_vmax[0])
    if mpmap == 2:
        fu = th/(umax/sc.nxr)-ir                                      # position inside the pixel, [0, 1]
        fv = (ph+vmax)/(2.0*vmax/sc.nyr)-jr
        fv = fv-sc.nyr*np.round((fv-0.5)/sc.nyr)                      # (phi = -pi and +pi are the same direction)
        t0, t1 = ir*umax/sc.nxr, (ir+1)*umax/sc.nxr
        if mrproj == 1:
            a, b, x = np.sin(t0)**2, np.sin(t1)**2, np.sin(th)**2
        else:
            a, b, x = np.cos(t0), np.cos(t1), np.cos(th)
        uni = [((x-a)/(b-a), 'cos / sin^2 theta'), (fv, 'phi')]
    else:
        U, V = th*np.cos(ph), th*np.sin(ph)
        fu = U/(umax/sc.nxr)+0.5*sc.nxr-ir
        fv = V/(vmax/sc.nyr)+0.5*sc.nyr-jr
        uni = [(fu, 'U'), (fv, 'V')]
        inside = np.cos(th) >= np.cos(np.radians(0.5*sc.cam_qmax[0]))-1e-6
        assert np.all(score[~inside] == 0.0) and np.all(score[np.cos(th) >= 1e-3] > 0.0) and (~inside).sum() > n//10
    assert np.all((fu >= -EDGE) & (fu <= 1.0+EDGE)) and np.all((fv >= -EDGE) & (fv <= 1.0+EDGE)), (fu.min(), fu.max(), fv.min(), fv.max())
    tol = 5.0/np.sqrt(12.0*n_p)                                       # of a unit interval
    for x, what in uni:
        means = np.array([x[pix == p].mean() for p in range(npix)])
        print('directions: map %d, weighting %d, %s: largest offset of a pixel mean from the middle %.4f (allowed %.4f)' % (mpmap, mrproj, what, np.abs(means-0.5).max(), tol))
        assert np.all(np.abs(means-0.5) <= tol), (what, means)


# ---- 2: single histories against the line integral -------------------------------------------------------------------------------------------

def _march32(sc, org, dirs):
    """the kernel's sum restated in float32: the incremental walk on (tx, ty, tz), one piece w B (1 - exp(-ka l)) per cell with float32
    ka, B, weights and pieces, the score summed in float64; non-scattering scenes over a black surface, 3-D layers and 1-D layers"""
    f = np.float32
    ka, B, eps, Bs = ref.cells(sc)
    ka, B = ka.astype(f), B.astype(f)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    dzl = np.diff(zg).astype(f)
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, f(sc.dx), f(sc.dy)
    k3lo, k3hi = sc.iz3l-1, sc.iz3l-1+sc.nz3
    out = np.zeros(len(dirs))
    for i, (o, u) in enumerate(zip(np.asarray(org, dtype=f), np.asarray(dirs, dtype=f))):
        k = int(np.clip(np.searchsorted(zg, float(o[2]), side='right')-1, 0, nz-1))
        if float(o[2]) == zg[k] and u[2] < 0 and k > 0:
            k -= 1
        cx, cy = np.floor(o[0]/dx), np.floor(o[1]/dy)
        px, py, pz = f(o[0]-cx*dx), f(o[1]-cy*dy), f(o[2]-f(zg[k]))
        ix, iy = int(cx) % nx, int(cy) % ny
        ax, ay, az = f(1)/max(abs(u[0]), f(1e-20)), f(1)/max(abs(u[1]), f(1e-20)), f(1)/max(abs(u[2]), f(1e-20))
        sx, sy = f(dx*ax), f(dy*ay)
        tx = f((dx-px if u[0] > 0 else px)*ax); ty = f((dy-py if u[1] > 0 else py)*ay); tz = f((dzl[k]-pz if u[2] > 0 else pz)*az)
        w, s = f(1), 0.0
        while True:
            in3d = k3lo <= k < k3hi
            ds = min(tx, ty, tz) if in3d else tz
            a = f(ka[k, iy, ix]*ds)
            e = np.exp(-a, dtype=f)
            em = f(-np.expm1(-a, dtype=f))
            s += float(f(f(w*B[k, iy, ix])*em))
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
                    s += float(f(f(w*f(eps))*f(Bs)))
                    break
                tz = f(dzl[k]*az)
            elif hx:
                tx = sx; ix = (ix+(1 if u[0] > 0 else -1)) % nx
            else:
                ty = sy; iy = (iy+(1 if u[1] > 0 else -1)) % ny
        out[i] = s
    return out


def test_single_histories_against_the_line_integral(solver):
    """a scene that never scatters over a black surface: a history IS its line integral.  Four sensors: down from the gap above the cloud, up
    from the ground, and up and down from INSIDE an absorbing voxel (z = 500 m: the forward route cannot be tested there)"""
    sc = cameras(absorbing_scene(0.0), [180.0, 0.0, 30.0, 150.0], [900.0, 100.0, 500.0, 500.0], xpos=[0.3, 0.7, 0.45, 0.45], ypos=[0.6, 0.2, 0.3, 0.3],
                 mpmap=2, mrproj=0, nxr=2, nyr=3, umax=87.0, vmax=180.0, phi=[0.0, 0.0, 70.0, 70.0])
    assert sc.extp[0, 1, int(0.3*8), int(0.45*8)] > 0.001          # the third and fourth sensor stand in a cloudy voxel
    npix, n = 24, 24*84
    solver.load_scene(sc); solver.reset()
    d, score, capped = solver.debug_backward(73, 0, n)
    assert capped == 0
    pix = np.arange(n) % npix
    iv = pix//6
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    org = np.array([[float(np.float32(sc.cam_xpos[v]*Lx)), float(np.float32(sc.cam_ypos[v]*Ly)), float(sc.view_zloc[v])] for v in iv])
    want = ref.march(sc, org, d.astype(np.float64), nimg=None)
    r32 = _march32(sc, org, d)
    gap32 = np.abs(r32/want-1.0).max()
    gap = np.abs(score/want-1.0)
    print('single histories: %d lines; float32 restatement: largest relative gap to the float64 march %.3e; the kernel: %.3e (allowed %.3e)'
          % (n, gap32, gap.max(), 4.0*gap32))
    assert want.min() > 0.0 and 1.0e-7 < gap32 < 1.0e-4              # (a float32 sum of a few dozen pieces)
    assert np.all(gap <= 4.0*gap32), (gap.max(), gap32, np.argmax(gap))
    for v in range(4):                                                # every sensor took part
        assert (iv == v).sum() == n//4 and np.all(score[iv == v] > 0.0)


# ---- 3: an isothermal scene glows at B(T) ----------------------------------------------------------------------------------------------------

def test_isothermal_scene_glows_at_planck(solver):
    """irradiance and actinic sensors, up- and down-looking, in the gap and INSIDE a cloudy, partly absorbing cell, read pi B and 2 pi B; every
    pixel of a 4 x 4 polar image inside the cone reads B.  The whole cyclic domain is seen: no truncation term; what the opaque top lets in
    from cold space, exp(-TAU_TOP), on the low side"""
    T = 285.0
    B = float(planck(WL, T))
    base = iso_scene(T)
    assert base.extp[0, 1, 4, 2] > 0.0                                 # cell (ix 2, iy 4) of the layer 200 ... 300 m is cloudy
    the, zs = [0.0, 180.0, 0.0, 180.0], [ZS_ISO, ZS_ISO, 250.0, 250.0]
    xs, ys = [0.3, 0.3, 0.3125, 0.3125], [0.6, 0.6, 0.5625, 0.5625]
    for mrproj, k in ((1, np.pi), (0, 2.0*np.pi)):
        sc = cameras(base, the, zs, xpos=xs, ypos=ys, mrproj=mrproj)
        m, e = batches(solver, sc, 16, 4*2000, 31+mrproj)
        assert np.all(solver.camera_direct() == 0.0)
        for iv in range(4):
            f, se4, want = k*m[iv, 0, 0], 4.0*k*e[iv, 0, 0], k*B
            print('isothermal: mrproj %d view %d: %.6f, expected %.6f, 4 se %.6f (%.2e of it)' % (mrproj, iv, f, want, se4, se4/want))
            assert se4 < 0.05*want
            assert -(se4+np.exp(-TAU_TOP)*want) <= f-want <= se4, (mrproj, iv, f, want, se4)
    n = 4
    sc = cameras(base, [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=n, nyr=n, umax=180.0, vmax=180.0)
    m, e = batches(solver, sc, 16, 32*1000, 37)
    edge = np.maximum(np.abs(np.arange(n)/n-0.5), np.abs((np.arange(n)+1.0)/n-0.5))*180.0
    inside = np.hypot(edge[None, :], edge[:, None]) <= 90.0            # the pixel's far corner lies inside the cone (qmax 180)
    assert inside.sum() == 4
    for iv in range(2):
        print('isothermal: polar image %d / B:\n%s\n4 se / B:\n%s' % (iv, np.round(m[iv]/B, 5), np.round(4.0*e[iv]/B, 5)))
        assert np.all(4.0*e[iv][inside] < 0.05*B)
        assert np.all((m[iv]-B)[inside] <= 4.0*e[iv][inside]) and np.all((B-m[iv])[inside] <= 4.0*e[iv][inside]+np.exp(-TAU_TOP)*B), (iv, m[iv]/B)
        assert np.all(m[iv] <= B*(1.0+1e-6)+4.0*e[iv])               # (pixels that straddle the cone hold less)


# ---- 4: a grey surface, against the line integral and the forward route ------------------------------------------------------------------------

def test_grey_surface_against_the_line_integral_and_the_forward_route(solver):
    base = absorbing_scene(0.1)
    kw = dict(xpos=[0.3, 0.7], ypos=[0.6, 0.2], mpmap=2, mrproj=0, nxr=2, nyr=3, umax=87.0, vmax=180.0)
    sc = cameras(base, [180.0, 0.0], [900.0, 100.0], **kw)
    coarse, fine = ref.surface_reflection(base, 16, 6, 12), ref.surface_reflection(base, 32, 12, 24)
    a = np.array([ref.rect_image(sc, iv, None, 16, coarse) for iv in range(2)])
    want = np.array([ref.rect_image(sc, iv, None, 32, fine) for iv in range(2)])
    qerr = np.abs(want-a)                                              # the quadrature's own error: the change under doubling
    m, e = batches(solver, sc, 16, 12*2000, 43)
    print('grey surface: backward / line integral\n%s\n4 se / want\n%s\nquadrature / want\n%s' % (np.round(m/want, 5), np.round(4.0*e/want, 5), np.round(qerr/want, 6)))
    assert np.all(4.0*e+qerr < 0.05*want)
    assert np.all(np.abs(m-want) <= 4.0*e+qerr), ((m-want)/want, (4.0*e+qerr)/want)
    # the forward route sees the domain out to two rings of images: never more than all of it
    fwd = cameras(base, [180.0, 0.0], [900.0, 100.0], method=0, images=2, **kw)
    mf, ef = batches(solver, fwd, 8, 150000, 47, name=None)
    assert solver.kernel_name().endswith('+ k_rays') and '[thermal]' in solver.kernel_name()
    print('grey surface: forward (cam_images 2) / backward\n%s\n4 se of both / backward\n%s' % (np.round(mf/m, 4), np.round(4.0*(ef+e)/m, 4)))
    assert np.all(mf-m <= 4.0*ef+4.0*e), ((mf-m)/m, (4.0*ef+4.0*e)/m)


# ---- 5: scattering, against the oracle's flux planes and the forward route -------------------------------------------------------------------

def test_scattering_slab_against_the_oracles_flux_planes(solver, oracle, nthreads):
    """an up- and a down-looking backward irradiance sensor in the gap against the oracle's domain-mean f_down and f_up at the gap's interfaces"""
    zs, nb, nper = 2000.0, 8, 400000
    fl = []
    fs = scattering_slab(TARGET_FLUX)
    for b in range(nb):
        f = oracle.run(fs, nper, seed=53, offset=b*nper, nthreads=nthreads)['flux'].astype(np.float64)
        fl.append([f[1, 2:4].mean(), f[2, 2:4].mean()])
    fl = np.array(fl)
    fo, fe = fl.mean(axis=0), fl.std(axis=0, ddof=1)/np.sqrt(nb)
    sc = cameras(scattering_slab(TARGET_RADIANCE), [0.0, 180.0], zs, xpos=0.3, ypos=0.6, mrproj=1)
    m, e = batches(solver, sc, 16, 2*20000, 59)
    for iv in range(2):
        f, se4 = np.pi*m[iv, 0, 0], 4.0*np.hypot(np.pi*e[iv, 0, 0], fe[iv])
        print('slab: view %d: backward sensor %.5f (se %.5f), oracle %.5f (se %.5f), 4 se of both %.5f' % (iv, f, np.pi*e[iv, 0, 0], fo[iv], fe[iv], se4))
        assert se4 < 0.05*fo[iv]
        assert abs(f-fo[iv]) <= se4, (iv, f, fo[iv], se4)


def test_tabulated_phase_function_and_rayleigh_against_the_forward_route(solver):
    """the slab with its phase function tabulated and a Rayleigh constituent in the 1-D layers: backward against forward (cam_images 2), 4 se
    of both in quadrature; the forward route is never high and low by at most 1 / (1 + t_c^2) of pi B_max.  (1.8e6 forward photons: its 4 se
    is 9 % of the reading and decides what the comparison can see; the backward reading's own 4 se is asserted below 5 %)"""
    N, zs = 2, 2000.0
    base = scattering_slab(TARGET_RADIANCE, tables=True)
    sc = cameras(base, [0.0, 180.0], zs, xpos=0.3, ypos=0.6, mrproj=1)
    m, e = batches(solver, sc, 16, 2*2500, 61)
    solver.set_counting(True)
    try:
        solver.load_scene(sc); solver.reset(); solver.run(20000, seed=5)
        cnt = solver.counters()
        assert solver.kernel_name() == 'k_backward<1> [thermal]'
    finally:
        solver.set_counting(False)
    # (a vertical line from the gap to either boundary crosses a scattering optical depth of 0.24: more than 1 - exp(-0.24) = 0.21 scatterings a history)
    assert cnt['photons'] == 20000 and cnt['scatter'] > 4000 and cnt['surface'] > 1000 and cnt['steps'] > cnt['steps3d'] > 0, cnt
    fwd = cameras(base, [0.0, 180.0], zs, xpos=0.3, ypos=0.6, mrproj=1, method=0, images=N)
    mf, ef = batches(solver, fwd, 8, 225000, 67, name=None)
    assert solver.kernel_name().endswith('+ k_rays'), solver.kernel_name()
    Bmax = float(planck(WL, 295.0))
    for iv, dz in ((0, float(sc.zgrd[-1])-zs), (1, zs)):
        tc = (N+0.5)*min(sc.nx*sc.dx, sc.ny*sc.dy)/dz
        b, f, se4, low = np.pi*m[iv, 0, 0], np.pi*mf[iv, 0, 0], 4.0*np.pi*np.hypot(e[iv, 0, 0], ef[iv, 0, 0]), np.pi*Bmax/(1.0+tc*tc)
        print('tables: view %d: backward %.5f (4 se %.5f), forward %.5f, 4 se of both %.5f, truncation bound %.5f' % (iv, b, 4.0*np.pi*e[iv, 0, 0], f, se4, low))
        assert 4.0*np.pi*e[iv, 0, 0] < 0.05*b
        assert -(se4+low) <= f-b <= se4, (iv, f, b, se4, low)


# ---- 6: bookkeeping ------------------------------------------------------------------------------------------------------------------------------

def test_raw_tallies_add_over_id_ranges(solver):
    import torch
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=3, nyr=3, umax=180.0, vmax=180.0)
    buf = torch.zeros(18, dtype=torch.float64, device='cuda:0')
    N, n1 = 50003, 20011
    try:
        solver.bind(buf.data_ptr(), None, None)
        solver.load_scene(sc); solver.reset()
        solver.run(N, seed=67); solver.sync()
        whole = buf.cpu().numpy().copy()
        solver.reset()
        solver.run(n1, seed=67); solver.run(N-n1, seed=67, offset=n1); solver.sync()
        parts = buf.cpu().numpy().copy()
        assert solver.kernel_name() == 'k_backward<0> [thermal]' and solver.debug_backward(67, 0, 0)[2] == 0
    finally:
        solver.bind(None, None, None)
    assert whole.min() > 0.0 and np.allclose(parts, whole, rtol=1.0e-12, atol=0.0), (parts/whole-1.0)


def test_every_pixel_is_divided_by_its_own_count(solver):
    """N no multiple of npix, and smaller than npix: the isothermal scene still reads B in every pixel that holds a history, 0 elsewhere"""
    T = 285.0
    B = float(planck(WL, T))
    sc = cameras(iso_scene(T), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, nxr=5, nyr=1, umax=80.0, mrproj=0)      # ten pixels
    nper = 10*700+3
    solver.load_scene(sc)
    out = []
    for b in range(16):
        solver.reset(); solver.run(nper, seed=71+b)       # (ids [0, nper) under another seed: the ids of a job cover [0, N))
        out.append(solver.radiance(nper).astype(np.float64))
        assert solver.debug_backward(1, 0, 0)[2] == 0
    a = np.array(out)
    m, e = a.mean(axis=0), a.std(axis=0, ddof=1)/4.0
    print('exact counts: image / B %s, 4 se / B %s' % (np.round(m.ravel()/B, 5), np.round(4.0*e.ravel()/B, 5)))
    assert np.all(4.0*e < 0.05*B) and np.all(m-B <= 4.0*e) and np.all(B-m <= 4.0*e+np.exp(-TAU_TOP)*B), (m/B, 4.0*e/B)
    solver.reset(); solver.run(4, seed=3)
    r = solver.radiance(4).ravel()
    assert np.all(np.abs(r[:4]/B-1.0) < 0.5) and np.all(r[4:] == 0.0) and np.all(np.isfinite(r)), r


def test_same_ids_same_image_at_two_launch_sizes(solver):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=4, nyr=4, umax=180.0, vmax=180.0)
    N = 40000
    res = []
    try:
        for lg in (30, 12):
            solver.set_tuning(batch_log2=lg)
            solver.load_scene(sc); solver.reset(); solver.run(N, seed=79, offset=1000)
            res.append(solver.radiance(N).astype(np.float64))
            assert solver.kernel_name() == 'k_backward<0> [thermal]' and solver.debug_backward(79, 0, 0)[2] == 0
    finally:
        solver.set_tuning(batch_log2=30)
    assert res[0].max() > 0.0 and np.allclose(res[0], res[1], rtol=2.0e-7, atol=0.0)      # (float32 read-out of sums in another order)


def test_what_the_route_does_not_serve_is_refused(solver):
    sc = cameras(iso_scene(), [0.0, 180.0], ZS_ISO, xpos=0.3, ypos=0.6)
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
            pass                                             # (mi3d_prepare refuses the LSRT surface of a thermal job already)
        solver.set_camera_method('backward')
        rc = solver.lib.mi3d_run(solver._h, 1000, 1, 0)
        msg = solver.lib.mi3d_last_error().decode()
        assert rc == -4 and word in msg, (word, rc, msg)
    below = dataclasses.replace(sc, view_zloc=[0.0, 350.0])
    solver.load_scene(below)
    assert solver.lib.mi3d_run(solver._h, 1000, 1, 0) == -1 and 'surface' in solver.lib.mi3d_last_error().decode()
    solver.load_scene(sc); solver.reset(); solver.run(1000, seed=1)
    assert solver.kernel_name() == 'k_backward<0> [thermal]' and solver.radiance(1000).min() > 0.0


# ---- the drop-in -------------------------------------------------------------------------------------------------------------------------------

def test_dropin_files_against_fused_statistics(tmp_path):
    import contextlib
    import copy
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
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=3, target='radiance', surface_albedo=0.05, source='thermal', camera_method='backward',
                           fdir=str(tmp_path/'irr'), Nrun=3, photons=6e4, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py',
                           overwrite=True, date=gin.DATE, quiet=True, abs_obj=ab, keep_files=True, sensor_type='irradiance',
                           sensor_xpos=[0.1, 0.35, 0.6, 0.85], sensor_ypos=0.5, sensor_altitude=[10.0, 700.0, 10.0, 5000.0],
                           sensor_zenith_angle=[0.0, 0.0, 20.0, 180.0])
    sol = get_runner().sol
    assert sol.kernel_name() == 'k_backward<0> [thermal]' and sol.debug_backward(1, 0, 0)[2] == 0
    nml = mca.mca_inp_read(m.fnames_inp[0][0])
    assert nml['Rad_mbwd'] == 1 and 'Rad_nimg' not in nml
    files = copy.copy(m); files.fused = None
    raw = mca.mca_out_raw(m.fnames_out[0][0])
    assert [v['name'].split()[0] for v in raw.data] == ['rad', 'rdir'] and np.all(raw.data[1]['data'] == 0.0)
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        assert sorted(a.keys()) == sorted(b.keys())
        for k in ('f', 'f_diffuse', 'f_direct'):
            x, y = a[k]['data'], b[k]['data']
            assert x.shape == y.shape and x.shape[0] == 4 and np.allclose(x, y, rtol=2e-5, atol=0.0), (mode, k, x, y)
        assert np.all(a['f_direct']['data'] == 0.0) and np.array_equal(a['f']['data'], a['f_diffuse']['data'])
    t = np.asarray(atm.lev['temperature']['data'], dtype=np.float64)
    f = b['f']['data'][:, 0]
    # pyrgeometers read less than pi B of the warmest air -- one of them from inside the cloud layer (700 m), where the forward route's noise is heavy-tailed
    assert np.all(f > 0.0) and np.all(f*1.0e3 < np.pi*planck(WL, t.max()))


def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on the one GPU) against one rank on the same ids: the shards of [0, N) add to the
    job's raw tally, and the read-out divides by the job's counts (tests/backward_dist_worker.py)"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'backward_dist_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(str(tmp_path), 'result.npz'))
    assert str(z['kernel']) == 'k_backward<0> [thermal]' and int(z['capped']) == 0
    a, b = z['job_dist_rad'], z['job_solo_rad']
    assert a.shape == b.shape == (4,) and a.min() > 0.0 and np.allclose(a, b, rtol=2e-6, atol=0.0), (a, b)     # the same histories: float32 of sums in another order
    for v in ('f', 'f_diffuse'):
        a, b = z['file_'+v], z['fused_'+v]
        assert a.shape == b.shape == (4,) and np.allclose(a, b, rtol=0.05, atol=0.0), (v, a, b)                   # different seeds
    assert np.all(z['file_f_direct'] == 0.0) and np.all(z['fused_f_direct'] == 0.0)
