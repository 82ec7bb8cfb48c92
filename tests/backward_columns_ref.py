"""
An independent float64 reference for the backward satellite views under independent columns and partial 3-D (mi3d_set_view_columns 1,
Rad_mvcol = 1; tests/test_backward_columns_host.py, tests/test_gpu_backward_columns.py).  The scenes are those of
tests/backward_views_ref.py with solver 2 / 1 and the switch on.  A history of a non-scattering scene is the slant Schwarzschild sum over
the layers of ONE column,

    sum_k B_k (1 - exp(-ka_k l_k)) exp(-tau before k) [+ exp(-tau) (eps B_s + (1 - eps) E_down / pi) at the surface],

l_k the slant path in layer k (dz_k / |mu|, the first one from the start's height), written from the scene's arrays alone by the contract
of include/mi3d.h (mi3d_set_view_columns): the column is the one under the point (xr, yr) of the pixel, there is no parallax shift, the
horizontal position folds inside the column.  Nothing of the solver is used.
"""

import dataclasses

import numpy as np

from er3t_amd.thermal import planck
from tests import backward_views_ref as vref
from tests import thermal_camera_ref as ref


def columns(sc, solver=2, **kw):
    """scene sc (one of tests/backward_views_ref.py or tests/backward_sun_ref.py) under independent columns (solver 2) or partial 3-D (1),
    the switch on"""
    return dataclasses.replace(sc, solver=solver, view_columns=1, **kw)


def column_of(sc, x, y):
    """(ix, iy) of the column that contains the points (x, y), clipped to the grid"""
    ix = np.clip(np.floor(np.asarray(x, dtype=np.float64)/float(sc.dx)).astype(np.int64), 0, sc.nx-1)
    iy = np.clip(np.floor(np.asarray(y, dtype=np.float64)/float(sc.dy)).astype(np.int64), 0, sc.ny-1)
    return ix, iy


def _surface(sc):
    """(eps, B_s) of every surface cell, (nyb, nxb) each (1 x 1: a uniform surface), float64 from the float32 inputs"""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    t0 = float(f(sc.tmp1d)[0])
    if sc.jsfc is None:
        return np.array([[1.0-float(np.clip(f(sc.sfc_param[0]), 0.0, 1.0))]]), np.array([[float(planck(sc.src_wlen, t0))]])
    eps = 1.0-np.clip(f(sc.psfc[0]), 0.0, 1.0)
    dT = f(sc.tmps2d) if sc.tmps2d is not None else np.zeros(eps.shape)
    return eps, planck(sc.src_wlen, t0+dT)


def _air(sc):
    """(ka, B) of every cell, (nz, ny, nx): tests/thermal_camera_ref.py's, which reads the air alone"""
    twin = sc if sc.jsfc is None else dataclasses.replace(sc, jsfc=None, psfc=None, tmps2d=None, sfc_mtype=1, sfc_param=[0.0, 0, 0, 0, 0])
    ka, B, _, _ = ref.cells(twin)
    return ka, B


def slant_paths(sc, z0, uz):
    """the layers a line from height z0 with vertical direction cosine uz crosses, in the order it crosses them, and its path in each:
    (k (m,), l (m,)); uz < 0: down to the surface, uz > 0: up to the top.  A start on a level belongs to the layer the direction points into"""
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    z0 = min(max(float(z0), zg[0]), zg[-1])
    if uz < 0.0:
        k0 = int(np.clip(np.searchsorted(zg, z0, side='left')-1, 0, sc.nz-1))
        ks = np.arange(k0, -1, -1)
        l = np.diff(zg)[ks].copy(); l[0] = z0-zg[k0]
    else:
        k0 = int(np.clip(np.searchsorted(zg, z0, side='right')-1, 0, sc.nz-1))
        ks = np.arange(k0, sc.nz)
        l = np.diff(zg)[ks].copy(); l[0] = zg[k0+1]-z0
    return ks, l/abs(uz)


def downwelling(sc, nmu):
    """E_down / pi at the surface of every column, (ny, nx): 2 int_0^1 I(mu) mu dmu of the column's own slant sum from the surface to the
    top, by nmu Gauss-Legendre points"""
    ka, B = _air(sc)
    g, w = np.polynomial.legendre.leggauss(nmu)
    mu, wmu = 0.5*(g+1.0), 0.5*w
    dz = np.diff(np.asarray(sc.zgrd, dtype=np.float64))
    E = np.zeros((sc.ny, sc.nx))
    for m, wm in zip(mu, wmu):
        tau = np.zeros((sc.ny, sc.nx)); I = np.zeros((sc.ny, sc.nx))
        for k in range(sc.nz):
            a = ka[k]*dz[k]/m
            I += B[k]*(-np.expm1(-a))*np.exp(-tau)
            tau += a
        E += 2.0*wm*m*I
    return E


def line_terms(sc, iv, xr, yr, nmu=None):
    """what the histories of view iv through the points (xr, yr) of the unshifted pixel grid score in a non-scattering scene, term by term:
    (rows (n, nz + 1) -- the term of every layer from the surface up, then the surface's --, weights (n, nz + 1) -- the same without the
    Planck functions: (1 - exp(-ka l)) exp(-tau before), and eps exp(-tau) --, column (ix, iy)).  nmu: the points of the downwelling
    irradiance a grey surface reflects (None: emission alone)"""
    v, zs, zreg = vref.view_geometry(sc, iv)
    u = -v
    xr = np.atleast_1d(np.asarray(xr, dtype=np.float64)); yr = np.atleast_1d(np.asarray(yr, dtype=np.float64))
    n = xr.size
    ix, iy = column_of(sc, xr, yr)
    ka, B = _air(sc)
    eps, Bs = _surface(sc)
    rows = np.zeros((n, sc.nz+1)); wts = np.zeros((n, sc.nz+1))
    ztoa = float(sc.zgrd[-1])
    if u[2] > 0.0 and zs >= ztoa:
        return rows, wts, (ix, iy)                                       # (looks into space from the top)
    ks, l = slant_paths(sc, min(zs, ztoa), u[2])
    tau = np.zeros(n)
    for k, lk in zip(ks, l):
        a = ka[k, iy, ix]*lk
        wts[:, k] = -np.expm1(-a)*np.exp(-tau)
        rows[:, k] = B[k, iy, ix]*wts[:, k]
        tau += a
    if u[2] < 0.0:
        # the surface cell under the folded position: the line has drifted u t from its start and stays in its column
        t = l.sum()
        px = np.mod(xr-ix*float(sc.dx)+u[0]*t, float(sc.dx)); py = np.mod(yr-iy*float(sc.dy)+u[1]*t, float(sc.dy))
        Lx, Ly = sc.nx*float(sc.dx), sc.ny*float(sc.dy)
        nyb, nxb = eps.shape
        ib = np.clip(np.floor((ix*float(sc.dx)+px)/Lx*nxb).astype(np.int64), 0, nxb-1)
        jb = np.clip(np.floor((iy*float(sc.dy)+py)/Ly*nyb).astype(np.int64), 0, nyb-1)
        wts[:, sc.nz] = eps[jb, ib]*np.exp(-tau)
        rows[:, sc.nz] = Bs[jb, ib]*wts[:, sc.nz]
        if nmu is not None:
            rows[:, sc.nz] += (1.0-eps[jb, ib])*downwelling(sc, nmu)[iy, ix]*np.exp(-tau)
    return rows, wts, (ix, iy)


def line_scores(sc, iv, xr, yr, nmu=None):
    return line_terms(sc, iv, xr, yr, nmu)[0].sum(axis=1)*float(sc.src_flx)


def line_scores32(sc, iv, xr, yr):
    """the same sum restated in float32, step by step as a history takes it: float32 ka, B, paths, weights and pieces, the score summed in
    float64; non-scattering scenes over a black or an emitting uniform surface"""
    f = np.float32
    v, zs, zreg = vref.view_geometry(sc, iv)
    u = (-v).astype(f)
    xr = np.atleast_1d(xr); yr = np.atleast_1d(yr)
    ix, iy = column_of(sc, xr, yr)
    ka, B = _air(sc)
    ka, B = ka.astype(f), B.astype(f)
    eps, Bs = _surface(sc)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    dzl = np.diff(zg).astype(f)
    az = f(1)/abs(u[2])
    out = np.zeros(xr.size)
    ztoa = float(zg[-1])
    if u[2] > 0 and zs >= ztoa:
        return out
    ks, _ = slant_paths(sc, min(zs, ztoa), float(u[2]))
    k0 = int(ks[0])
    pz = f(f(min(zs, ztoa))-f(zg[k0]))
    pz = min(max(pz, f(0)), dzl[k0])
    for i in range(xr.size):
        w, s = f(1), 0.0
        tz = f((dzl[k0]-pz if u[2] > 0 else pz)*az)
        for k in ks:
            if k != k0:
                tz = f(dzl[k]*az)
            a = f(ka[k, iy[i], ix[i]]*tz)
            e = np.exp(-a, dtype=f)
            em = f(-np.expm1(-a, dtype=f))
            s += float(f(f(w*B[k, iy[i], ix[i]])*em))
            w = f(w*e)
            if w < 1e-7:
                break
        else:
            if u[2] < 0:
                s += float(f(f(w*f(eps[0, 0]))*f(Bs[0, 0])))
        out[i] = s*float(f(sc.src_flx))
    return out


def _pieces(npx, L, breaks):
    """the pieces of every pixel of one image axis between the break points: (midpoints, weights that add to 1 per pixel, the pixel of each)"""
    X, W, I = [], [], []
    bk = np.unique(np.round(np.mod(np.asarray(breaks, dtype=np.float64), L), 9))
    for i in range(npx):
        a, b = i*L/npx, (i+1)*L/npx
        e = np.concatenate([[a], bk[(bk > a) & (bk < b)], [b]])
        X.append(0.5*(e[:-1]+e[1:])); W.append(np.diff(e)/(b-a)); I.append(np.full(e.size-1, i))
    return np.concatenate(X), np.concatenate(W), np.concatenate(I)


def _axis_breaks(sc, iv, axis):
    """where along xr (axis 0) or yr (1) the score of a line changes: the column faces, and -- the surface grid may cut a column -- the points
    whose folded position at the surface lies on a face of the surface grid or on the column's own face"""
    v, zs, zreg = vref.view_geometry(sc, iv)
    u = -v
    d, n = ((float(sc.dx), sc.nx), (float(sc.dy), sc.ny))[axis]
    L = n*d
    bk = [np.arange(n)*d]
    eps, _ = _surface(sc)
    nb = eps.shape[1-axis]
    if u[2] < 0.0:
        _, l = slant_paths(sc, min(zs, float(sc.zgrd[-1])), u[2])
        drift = u[axis]*l.sum()
        faces = np.concatenate([np.arange(nb)*L/nb, np.arange(n)*d])
        for m in range(n):
            inside = faces[(faces >= m*d) & (faces < (m+1)*d)]-m*d           # the faces inside column m, from its low face
            bk.append(m*d+np.mod(inside-drift, d))
    return np.concatenate(bk)


def column_image(sc, iv, nmu=None):
    """the image (nyr, nxr) of view iv of a non-scattering scene under independent columns: per pixel the mean over its area of the unshifted
    grid of the column sums (line_scores).  The score is piecewise constant in (xr, yr), so the mean is exact: one point per piece between
    the break points of either axis"""
    x, wx, ix = _pieces(sc.nxr, sc.nx*float(sc.dx), _axis_breaks(sc, iv, 0))
    y, wy, iy = _pieces(sc.nyr, sc.ny*float(sc.dy), _axis_breaks(sc, iv, 1))
    Y, X = np.meshgrid(y, x, indexing='ij')
    R = line_scores(sc, iv, X.ravel(), Y.ravel(), nmu).reshape(y.size, x.size)
    img = np.zeros((sc.nyr, sc.nxr))
    np.add.at(img, (iy[:, None], ix[None, :]), R*wy[:, None]*wx[None, :])
    return img


# ---- the sun ray of a reflecting surface under a non-scattering atmosphere (tests/backward_sun_ref.py's scene) ---------------------------------

def sun_surface_scores(sc, iv, xr, yr, ray3d):
    """what the down-looking histories of view iv through (xr, yr) score in a scene that neither scatters nor emits, float64:
    exp(-tau_view) a / pi F mu0 exp(-tau_sun) Src_flx, the view's path the column's own; the sun ray from the folded hit point in the
    column: ray3d False (independent columns) level to level in that column, True (partial 3-D) through the cyclic grid, by
    tests/backward_sun_ref.py's tau_line"""
    from tests import backward_sun_ref as sref
    v, zs, zreg = vref.view_geometry(sc, iv)
    u = -v
    xr = np.atleast_1d(np.asarray(xr, dtype=np.float64)); yr = np.atleast_1d(np.asarray(yr, dtype=np.float64))
    ix, iy = column_of(sc, xr, yr)
    ke = sref.extinction(sc)
    dz = np.diff(np.asarray(sc.zgrd, dtype=np.float64))
    ks, l = slant_paths(sc, min(zs, float(sc.zgrd[-1])), u[2])
    tau_v = (ke[ks][:, iy, ix]*l[:, None]).sum(axis=0)
    t = l.sum()
    hx = ix*float(sc.dx)+np.mod(xr-ix*float(sc.dx)+u[0]*t, float(sc.dx)); hy = iy*float(sc.dy)+np.mod(yr-iy*float(sc.dy)+u[1]*t, float(sc.dy))
    sun = sref.sun_direction(sc.src_the, sc.src_phi)
    if ray3d:
        hit = np.stack([hx, hy, np.full(hx.size, float(sc.zgrd[0]))], axis=-1)
        tau_s, _ = sref.tau_line(sc, hit, np.broadcast_to(-sun, hit.shape))
    else:
        tau_s = (ke[:, iy, ix]*dz[:, None]).sum(axis=0)/abs(sun[2])
    a = sref.surface_albedo(sc, hx, hy)
    return np.exp(-tau_v)*a/np.pi*float(sc.src_fsol)*abs(sun[2])*np.exp(-tau_s)*float(sc.src_flx)
