"""
A float64 reference for the per-cell emission weights of the backward route (mi3d_set_emission_weights 1) in a scene that
does NOT scatter, over a black or grey surface: the line of sight from a sensor is cut at every cell face it crosses, and the piece of
length l in cell c, reached through the optical depth tau, carries the weight exp(-tau) (1 - exp(-ka l)); the surface cell carries
exp(-tau) eps.  (Over a grey surface this is the line's own part of the reading: what the surface reflects is not followed.)  Written from
the scene arrays alone; the cells are in the order of the solver's tally: voxels [nz3][ny][nx], layers [nz] -- those inside the 3-D region
stay empty --, surface cells [nyb][nxb].  Its own check is tests/thermal_camera_ref.march: sum_c K_c B_c is that line integral.
"""

import numpy as np

from er3t_amd.thermal import planck


def cell_tables(sc):
    """(ka, B, eps, nvox, nsfc): float64 absorption coefficient and Planck radiance of every cell in tally order ([ncell]; the layers inside
    the 3-D region hold 0), the surface cells' emissivities [nsfc] (their B is in B)"""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    nz, nx, ny, nz3 = sc.nz, sc.nx, sc.ny, sc.nz3
    if np.any(f(sc.ext1d)*f(sc.omg1d) != 0.0) or (nz3 > 0 and np.any(f(sc.extp)*f(sc.omgp) != 0.0)):
        raise ValueError('the reference is for non-scattering scenes')
    t = f(sc.tmp1d)
    tl = 0.5*(t[:-1]+t[1:])
    ka1 = f(sc.abs1d)+(f(sc.ext1d)*(1.0-f(sc.omg1d))).sum(axis=0)
    b1 = planck(sc.src_wlen, tl)
    k3lo = sc.iz3l-1
    nvox = nx*ny*nz3
    if nz3 > 0:
        kv = ka1[k3lo:k3lo+nz3, None, None]+f(sc.extp).sum(axis=0)+(f(sc.abst) if sc.abst is not None else 0.0)
        tv = tl[k3lo:k3lo+nz3, None, None]+(f(sc.tmpa3d) if sc.tmpa3d is not None else np.zeros((nz3, ny, nx)))
        ka1 = ka1.copy(); b1 = b1.copy()
        ka1[k3lo:k3lo+nz3] = 0.0; b1[k3lo:k3lo+nz3] = 0.0
        kav, bv = kv.ravel(), planck(sc.src_wlen, tv).ravel()
    else:
        kav, bv = np.zeros(0), np.zeros(0)
    if sc.jsfc is not None:
        alb = f(sc.psfc[0]).ravel()
        ts = t[0]+(f(sc.tmps2d).ravel() if sc.tmps2d is not None else np.zeros(alb.size))
    else:
        alb = np.array([float(np.float32(sc.sfc_param[0]))])
        ts = np.array([t[0]])
    eps = 1.0-np.clip(alb, 0.0, 1.0)
    return np.concatenate([kav, ka1, np.zeros(eps.size)]), np.concatenate([bv, b1, planck(sc.src_wlen, ts)]), eps, nvox, eps.size


def line_weights(sc, org, dirs, max_steps=100000):
    """K (n, ncell) float64 of the lines of sight from org (n, 3) along the unit vectors dirs (n, 3), which point away from the sensor"""
    ka, B, eps, nvox, nsfc = cell_tables(sc)
    zg = np.asarray(sc.zgrd, dtype=np.float64)
    nz, nx, ny, nz3, k3lo = sc.nz, sc.nx, sc.ny, sc.nz3, sc.iz3l-1
    dx, dy = float(sc.dx), float(sc.dy)
    nyb, nxb = sc.jsfc.shape if sc.jsfc is not None else (1, 1)
    dirs = np.atleast_2d(np.asarray(dirs, dtype=np.float64))
    org = np.broadcast_to(np.atleast_2d(np.asarray(org, dtype=np.float64)), dirs.shape)
    K = np.zeros((dirs.shape[0], ka.size))
    for i, (o, u) in enumerate(zip(org, dirs)):
        if u[2] == 0.0:
            raise ValueError('horizontal line of sight')
        ixu, iyu = int(np.floor(o[0]/dx)), int(np.floor(o[1]/dy))
        k = int(np.clip(np.searchsorted(zg, o[2], side='right')-1, 0, nz-1))
        t, tau = 0.0, 0.0
        for _ in range(max_steps):
            tx = (((ixu+1) if u[0] > 0.0 else ixu)*dx-o[0])/u[0] if u[0] != 0.0 else np.inf
            ty = (((iyu+1) if u[1] > 0.0 else iyu)*dy-o[1])/u[1] if u[1] != 0.0 else np.inf
            tz = ((zg[k+1] if u[2] > 0.0 else zg[k])-o[2])/u[2]
            tn = min(tx, ty, tz)
            ds = max(tn-t, 0.0)
            c = ((k-k3lo)*ny+iyu % ny)*nx+ixu % nx if k3lo <= k < k3lo+nz3 else nvox+k
            K[i, c] += np.exp(-tau)*(-np.expm1(-ka[c]*ds))
            tau += ka[c]*ds
            t = tn
            if tz <= tn:
                k += 1 if u[2] > 0.0 else -1
                if k >= nz:
                    break
                if k < 0:
                    x, y = (o[0]+u[0]*t) % (nx*dx), (o[1]+u[1]*t) % (ny*dy)
                    ib, jb = min(int(x/(nx*dx)*nxb), nxb-1), min(int(y/(ny*dy)*nyb), nyb-1)
                    K[i, nvox+nz+jb*nxb+ib] += np.exp(-tau)*eps[jb*nxb+ib]
                    break
            elif tx <= tn:
                ixu += 1 if u[0] > 0.0 else -1
            else:
                iyu += 1 if u[1] > 0.0 else -1
            if tau > 60.0:
                break
        else:
            raise RuntimeError('line_weights: a line did not end')
    return K


def planck_cells(sc):
    """[ncell] float64 Planck radiance of every cell in tally order"""
    return cell_tables(sc)[1]
