"""
Scenes and an independent float64 reference for the sunlight term of the backward satellite views (mi3d_set_view_sunlight 1, Rad_mvsun = 1;
DESIGN.md §5.18; tests/test_backward_sun_host.py, tests/test_gpu_backward_sun.py).  The scenes are those of tests/backward_views_ref.py --
6 x 5 x 4 voxels under two 1-D layers, dx = 300 != dy = 250, top at 1500 m -- at 3.75 um with a sun.  The reference is the optical depth of
ka + ks of every constituent from a point to where a straight line leaves the atmosphere, through the cyclic grid, cut at every x, y and z
face it crosses, written from the scene's arrays alone.  Nothing of the solver is used.
"""

import dataclasses

import numpy as np

from tests import backward_views_ref as vref

WL = 3.75
COLD = 20.0               # K: planck(3.75, T) is 0 in float32 up to some 35 K -- a scene this cold emits nothing, whatever its anomalies


def sun_direction(the, phi):
    """the unit vector along which sunlight travels (Src_the, Src_phi in degrees; d_z < 0 for a sun above the horizon)"""
    t, p = np.radians(the), np.radians(phi)
    return np.array([np.sin(t)*np.cos(p), np.sin(t)*np.sin(p), np.cos(t)])


def sunlit(sc, the, phi, fsol, qmax=0.0, cold=False, **kw):
    """scene sc (a thermal one of tests/backward_views_ref.py) as the solar+thermal job served backwards with the sunlight term: Src_mtype = 2
    at 3.75 um.  cold: 20 K at every level"""
    tmp = np.full(sc.zgrd.size, COLD) if cold else sc.tmp1d
    return dataclasses.replace(sc, src_mtype=2, src_wlen=WL, src_fsol=float(fsol), src_the=float(the), src_phi=float(phi), src_qmax=float(qmax),
                               tmp1d=tmp, view_method=1, view_sunlight=1, **kw)


def thermal_twin(sc):
    """the thermal job (Src_mtype = 3) of a sunlit scene, the switch off: what Src_fsol = 0 must reproduce bit for bit"""
    return dataclasses.replace(sc, src_mtype=3, src_fsol=None, view_sunlight=0)


ALBEDO_MAP = np.array([[0.10, 0.35, 0.60], [0.80, 0.25, 0.45]], dtype=np.float32)       # (nyb, nxb) = (2, 3)


def absorbing_sunlit(the, phi, fsol=100.0, qmax=0.0, views=vref.VIEWS[:2]):
    """the absorbing scene (no scattering) over a 3 x 2 albedo map, 20 K everywhere: nothing emits, and a history that reaches the surface
    scores the one term w_sfc a / pi F mu0 T_sun"""
    sc = vref.absorbing_scene(views=views, albedo=0.0, sfc2d=True)
    psfc = np.zeros((5, 2, 3), dtype=np.float32); psfc[0] = ALBEDO_MAP
    return sunlit(sc, the, phi, fsol, qmax, cold=True, psfc=psfc)


def scattering_sunlit(the, phi, fsol, qmax=0.0, omgp=None, nxr=6, nyr=6):
    """the checkerboard cloud (a tabulated and an analytic constituent) at 3.75 um, its own temperatures"""
    sc = vref.scattering_scene(nxr=nxr, nyr=nyr)
    kw = {} if omgp is None else dict(omgp=np.full_like(sc.omgp, omgp))
    return sunlit(sc, the, phi, fsol, qmax, **kw)


def extinction(sc):
    """ka + ks of every constituent in every cell, (nz, ny, nx), float64 from the float32 inputs"""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    ke1 = f(sc.abs1d)+f(sc.ext1d).sum(axis=0)
    ke = np.repeat(ke1[:, None, None], sc.ny, axis=1).repeat(sc.nx, axis=2)
    if sc.nz3 > 0:
        k3 = slice(sc.iz3l-1, sc.iz3l-1+sc.nz3)
        ke[k3] += f(sc.extp).sum(axis=0)+(f(sc.abst) if sc.abst is not None else 0.0)
    return ke


def tau_line(sc, org, dirs, max_steps=100000):
    """the optical depth of ka + ks from the points org (n, 3) along the unit vectors dirs (n, 3) to where the line leaves the atmosphere --
    through the top (dirs_z > 0) or into the surface (dirs_z < 0) -- through the cyclic grid, and the point (x, y) where it leaves, unfolded:
    (tau (n,), xy (n, 2)).  A point on a level or a cell face belongs to the cell the direction points into"""
    ke = extinction(sc)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, float(sc.dx), float(sc.dy)
    org = np.atleast_2d(np.asarray(org, dtype=np.float64)); dirs = np.atleast_2d(np.asarray(dirs, dtype=np.float64))
    n = max(org.shape[0], dirs.shape[0])
    org = np.broadcast_to(org, (n, 3)).copy(); dirs = np.broadcast_to(dirs, (n, 3))
    sx, sy, sz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    if np.any(sz == 0.0):
        raise ValueError('horizontal line')
    fx, fy = org[:, 0]/dx, org[:, 1]/dy
    ix = np.where((fx == np.floor(fx)) & (sx < 0.0), np.floor(fx)-1, np.floor(fx)).astype(np.int64)
    iy = np.where((fy == np.floor(fy)) & (sy < 0.0), np.floor(fy)-1, np.floor(fy)).astype(np.int64)
    k = np.where(sz > 0.0, np.searchsorted(zg, org[:, 2], side='right')-1, np.searchsorted(zg, org[:, 2], side='left')-1)
    k = np.clip(k, 0, nz-1)
    t = np.zeros(n); tau = np.zeros(n)
    alive = np.ones(n, dtype=bool)
    for _ in range(max_steps):
        a = np.nonzero(alive)[0]
        if not a.size:
            break
        with np.errstate(divide='ignore', invalid='ignore'):
            tx = np.where(sx[a] > 0.0, ((ix[a]+1)*dx-org[a, 0])/sx[a], np.where(sx[a] < 0.0, (ix[a]*dx-org[a, 0])/sx[a], np.inf))
            ty = np.where(sy[a] > 0.0, ((iy[a]+1)*dy-org[a, 1])/sy[a], np.where(sy[a] < 0.0, (iy[a]*dy-org[a, 1])/sy[a], np.inf))
        tz = np.where(sz[a] > 0.0, (zg[k[a]+1]-org[a, 2])/sz[a], (zg[k[a]]-org[a, 2])/sz[a])
        tn = np.minimum(np.minimum(tx, ty), tz)
        tau[a] += ke[k[a], np.mod(iy[a], ny), np.mod(ix[a], nx)]*np.maximum(tn-t[a], 0.0)
        t[a] = tn
        zf = tz <= tn
        xf = (tx <= tn) & ~zf
        yf = ~zf & ~xf
        ix[a[xf]] += np.where(sx[a[xf]] > 0.0, 1, -1)
        iy[a[yf]] += np.where(sy[a[yf]] > 0.0, 1, -1)
        kz = a[zf]
        k[kz] += np.where(sz[kz] > 0.0, 1, -1)
        alive[kz[(k[kz] >= nz) | (k[kz] < 0)]] = False
        k[kz] = np.clip(k[kz], 0, nz-1)
    else:
        raise RuntimeError('tau_line: a line did not end')
    return tau, np.stack([org[:, 0]+sx*t, org[:, 1]+sy*t], axis=-1)


def surface_albedo(sc, x, y):
    """the albedo of the surface cell that holds the points (x, y), folded into the domain"""
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    if sc.jsfc is None:
        return np.full(np.shape(x), float(np.float32(sc.sfc_param[0])))
    a = np.asarray(sc.psfc[0], dtype=np.float64)
    ib = np.clip(np.floor(np.mod(x, Lx)/Lx*a.shape[1]).astype(int), 0, a.shape[1]-1)
    jb = np.clip(np.floor(np.mod(y, Ly)/Ly*a.shape[0]).astype(int), 0, a.shape[0]-1)
    return a[jb, ib]


def surface_scores(sc, start, d):
    """what the down-looking histories from the points start (n, 3) along d (n, 3) score in a scene that neither scatters nor emits, float64:
    w_sfc a / pi F mu0 T_sun Src_flx at the point where the line meets the surface, Src_qmax = 0.  Also the hit points, folded: (score, xy)"""
    sun = sun_direction(sc.src_the, sc.src_phi)
    tau_v, xy = tau_line(sc, start, d)
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    hit = np.stack([np.mod(xy[:, 0], Lx), np.mod(xy[:, 1], Ly), np.full(len(xy), float(sc.zgrd[0]))], axis=-1)
    tau_s, _ = tau_line(sc, hit, np.broadcast_to(-sun, hit.shape))
    a = surface_albedo(sc, hit[:, 0], hit[:, 1])
    return np.exp(-tau_v)*a/np.pi*float(sc.src_fsol)*abs(sun[2])*np.exp(-tau_s)*float(sc.src_flx), hit[:, :2]
