"""
An independent float64 reference for the cameras and point radiometers of a NON-SCATTERING thermal scene (tests/test_gpu_thermal_camera.py,
tests/test_thermal_camera_host.py): the line integral of ka B(T) exp(-tau) ds from a sensor through the cyclic voxel grid and the 1-D
layers, plus what the Lambertian surface sends up the line of sight -- its emission eps B(Ts) and the downwelling irradiance it reflects,
(1 - eps) E_down / pi --, cut off where the line leaves the box |dx| <= (N + 1/2) Lx, |dy| <= (N + 1/2) Ly around the sensor: the events
whose periodic images of the sensor the solver serves with cam_images = N.  Pixel values are quadratures over the pixel with the pixel's
own weight.  Written from the scene arrays alone, in the manner of march_tau in tests/test_gpu_radiometer.py; nothing of the solver is used.
"""

import numpy as np

from er3t_amd.thermal import planck


def cells(sc):
    """absorption coefficient [1/m] and Planck function of every cell, (nz, ny, nx), float64 from the float32 inputs; the surface's
    emissivity and Planck function"""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    nz = sc.nz
    ka1 = f(sc.abs1d) + (f(sc.ext1d)*(1.0-f(sc.omg1d))).sum(axis=0)
    t = f(sc.tmp1d)
    tl = 0.5*(t[:-1]+t[1:])
    ka = np.repeat(ka1[:, None, None], sc.ny, axis=1).repeat(sc.nx, axis=2)
    T = np.repeat(tl[:, None, None], sc.ny, axis=1).repeat(sc.nx, axis=2)
    if sc.nz3 > 0:
        k3 = slice(sc.iz3l-1, sc.iz3l-1+sc.nz3)
        if np.any(f(sc.extp)*f(sc.omgp) != 0.0) or np.any(f(sc.ext1d)*f(sc.omg1d) != 0.0):
            raise ValueError('the reference is for non-scattering scenes')
        ka[k3] += f(sc.extp).sum(axis=0) + (f(sc.abst) if sc.abst is not None else 0.0)
        if sc.tmpa3d is not None:
            T[k3] += f(sc.tmpa3d)
    assert ka.shape == (nz, sc.ny, sc.nx)
    eps = 1.0-float(np.clip(np.float32(sc.sfc_param[0]), 0.0, 1.0))
    return ka, planck(sc.src_wlen, T), eps, float(planck(sc.src_wlen, float(t[0])))


def march(sc, org, dirs, nimg=None, refl=None, max_steps=20000):
    """radiance arriving at the points org (n, 3) from the directions dirs (n, 3), unit vectors pointing AWAY from the sensor along the line
    of sight.  nimg: the box (None: no box: the whole cyclic domain).  refl: a function (x, y) -> reflected radiance leaving the surface
    there (None: emission only).  Every ray is cut at the x, y and z cell faces it crosses and summed piece by piece."""
    ka, B, eps, Bs = cells(sc)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, float(sc.dx), float(sc.dy)
    org = np.atleast_2d(np.asarray(org, dtype=np.float64)); dirs = np.atleast_2d(np.asarray(dirs, dtype=np.float64))
    n = dirs.shape[0]
    org = np.broadcast_to(org, (n, 3)).copy()
    sx, sy, sz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    if np.any(sz == 0.0):
        raise ValueError('horizontal line of sight')
    ixu = np.floor(org[:, 0]/dx).astype(np.int64); iyu = np.floor(org[:, 1]/dy).astype(np.int64)
    k = np.clip(np.searchsorted(zg, org[:, 2], side='right')-1, 0, nz-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        tbox = np.full(n, np.inf)
        if nimg is not None:
            tbox = np.minimum(np.where(sx != 0.0, (nimg+0.5)*nx*dx/np.abs(sx), np.inf), np.where(sy != 0.0, (nimg+0.5)*ny*dy/np.abs(sy), np.inf))
    t = np.zeros(n); tau = np.zeros(n); I = np.zeros(n)
    alive = np.ones(n, dtype=bool)
    for _ in range(max_steps):
        if not alive.any():
            break
        a = np.nonzero(alive)[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            tx = np.where(sx[a] > 0.0, ((ixu[a]+1)*dx-org[a, 0])/sx[a], np.where(sx[a] < 0.0, (ixu[a]*dx-org[a, 0])/sx[a], np.inf))
            ty = np.where(sy[a] > 0.0, ((iyu[a]+1)*dy-org[a, 1])/sy[a], np.where(sy[a] < 0.0, (iyu[a]*dy-org[a, 1])/sy[a], np.inf))
        tz = np.where(sz[a] > 0.0, (zg[k[a]+1]-org[a, 2])/sz[a], (zg[k[a]]-org[a, 2])/sz[a])
        tn = np.minimum(np.minimum(tx, ty), np.minimum(tz, tbox[a]))
        ds = np.maximum(tn-t[a], 0.0)
        kk = ka[k[a], np.mod(iyu[a], ny), np.mod(ixu[a], nx)]
        bb = B[k[a], np.mod(iyu[a], ny), np.mod(ixu[a], nx)]
        I[a] += bb*(-np.expm1(-kk*ds))*np.exp(-tau[a])
        tau[a] += kk*ds
        t[a] = tn
        out = tn >= tbox[a]
        zf = (tz <= tn) & ~out
        xf = (tx <= tn) & ~out & ~zf
        yf = ~out & ~zf & ~xf
        ixu[a[xf]] += np.where(sx[a[xf]] > 0.0, 1, -1)
        iyu[a[yf]] += np.where(sy[a[yf]] > 0.0, 1, -1)
        kz = a[zf]
        k[kz] += np.where(sz[kz] > 0.0, 1, -1)
        gone = kz[k[kz] >= nz]
        hit = kz[k[kz] < 0]
        if hit.size:
            up = eps*Bs
            if refl is not None:
                up = up + refl(org[hit, 0]+sx[hit]*t[hit], org[hit, 1]+sy[hit]*t[hit])
            I[hit] += up*np.exp(-tau[hit])
        k[kz] = np.clip(k[kz], 0, nz-1)
        alive[a[out]] = False; alive[gone] = False; alive[hit] = False
        alive[tau > 60.0] = False
    else:
        raise RuntimeError('march: a ray did not end')
    return I


def surface_reflection(sc, m, nmu, nphi):
    """the radiance a Lambertian surface reflects, (1 - eps) E_down / pi, on an m x m grid of points over the domain (nearest point
    looked up): E_down by Gauss-Legendre in mu and the midpoint rule in phi, through the whole cyclic domain (photons fly on across it)"""
    _, _, eps, _ = cells(sc)
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    if eps >= 1.0:
        return lambda x, y: np.zeros_like(np.asarray(x, dtype=np.float64))
    xs = (np.arange(m)+0.5)*Lx/m; ys = (np.arange(m)+0.5)*Ly/m
    g, w = np.polynomial.legendre.leggauss(nmu)
    mu, wmu = 0.5*(g+1.0), 0.5*w
    ph = (np.arange(nphi)+0.5)*2.0*np.pi/nphi
    MU, PH = np.meshgrid(mu, ph, indexing='ij')
    d = np.stack([np.sqrt(1.0-MU**2)*np.cos(PH), np.sqrt(1.0-MU**2)*np.sin(PH), MU], axis=-1).reshape(-1, 3)
    wq = (np.repeat(wmu[:, None], nphi, axis=1)*MU*2.0*np.pi/nphi).ravel()
    Y, X = np.meshgrid(ys, xs, indexing='ij')
    org = np.stack([X.ravel(), Y.ravel(), np.full(X.size, float(sc.zgrd[0]))], axis=-1)
    I = march(sc, np.repeat(org, d.shape[0], axis=0), np.tile(d, (org.shape[0], 1)))
    E = (I.reshape(org.shape[0], -1)*wq[None]).sum(axis=1).reshape(m, m)
    R = (1.0-eps)*E/np.pi

    def refl(x, y):
        i = np.mod(np.floor(np.asarray(x)/Lx*m).astype(np.int64), m); j = np.mod(np.floor(np.asarray(y)/Ly*m).astype(np.int64), m)
        return R[j, i]
    return refl


def camera_axes(the, phi, psi):
    """image x, image y and the axis of a camera: the world axes turned by Rz(phi) Ry(the) Rz(psi) (include/mi3d.h: mi3d_set_cameras)"""
    def rz(a):
        c, s = np.cos(np.radians(a)), np.sin(np.radians(a))
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(np.radians(the)), np.sin(np.radians(the))
    R = rz(phi) @ np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ rz(psi)
    return R[:, 0], R[:, 1], R[:, 2]


def rect_image(sc, iv, nimg, nsub, refl=None):
    """the image (nyr, nxr) of camera iv of a scene with the rectangular map: per pixel the weighted mean of the radiance, weight
    sin(theta) (Rad_mrproj = 0) or cos(theta) sin(theta) (1), by nsub x nsub Gauss-Legendre points in theta and phi"""
    X, Y, Z = camera_axes(sc.view_the[iv], sc.view_phi[iv], sc.cam_psi[iv])
    org = np.array([float(np.float32(sc.cam_xpos[iv]*sc.nx*sc.dx)), float(np.float32(sc.cam_ypos[iv]*sc.ny*sc.dy)), float(sc.view_zloc[iv])])
    umax, vmax = np.radians(sc.cam_umax[iv]), np.radians(sc.cam_vmax[iv])
    g, w = np.polynomial.legendre.leggauss(nsub)
    img = np.zeros((sc.nyr, sc.nxr))
    D, W, idx = [], [], []
    for jr in range(sc.nyr):
        for ir in range(sc.nxr):
            th = (ir+0.5*(g+1.0))*umax/sc.nxr; ph = -vmax+(jr+0.5*(g+1.0))*2.0*vmax/sc.nyr
            TH, PH = np.meshgrid(th, ph, indexing='ij')
            wt = np.outer(w, w)*np.sin(TH)*(np.cos(TH) if sc.cam_mrproj == 1 else 1.0)
            d = (np.sin(TH)*np.cos(PH))[..., None]*X + (np.sin(TH)*np.sin(PH))[..., None]*Y + np.cos(TH)[..., None]*Z
            D.append(d.reshape(-1, 3)); W.append(wt.ravel()); idx.append((jr, ir))
    I = march(sc, org, np.concatenate(D), nimg=nimg, refl=refl).reshape(len(idx), -1)
    for (jr, ir), wt, Ii in zip(idx, W, I):
        img[jr, ir] = (Ii*wt).sum()/wt.sum()
    return img
