"""
A float64 prediction of every raw flux and heating tally of the FORWARD flux loops, photon by photon (DESIGN.md §5.21;
tests/test_flight_host.py, tests/test_gpu_flight.py).  numpy only; nothing of the solver is used.

The scenes are those of tests/le_rays_ref.py -- nothing scatters, every extinction a multiple of a power of two -- as flux + heating jobs
without views, wmin = 0, every extinction scaled by SCALE = 1/8 (multiples of 2^-15 / m: still exact), over a black or a Lambert surface of
albedo 0.5.  A history is then fixed by the photon's Philox blocks alone.  Read in mi3d_kernels.hip / mi3d_kernel_flux.hip (blocks B6 launch,
B5 finish, B6 flight), the lean loop's shared finish and k_entry, and the same in oracle/mi3d_oracle.c (run_photon):

  block 0   words 0, 1: the start (u0 Lx, u1 Ly) on the top (x >= Lx -> 0); words 2, 3 the solar cone (not used: src_qmax = 0)
  block 1   word 0: the free path -ln u of the DOWN leg; words 2, 3 stay with the photon as u2, u3 and serve the next event: the Lambert
            reflection takes the direction rotate_dir((0, 0, 1), sqrt(u2), u3), bz = max(bz, 1e-9)
  block 2   word 0: the free path of the UP leg (wmin = 0: no roulette block in between)

  down leg  weight 1, direction the float32-rounded sun direction (rounded = False: the formula's own float64, what the oracle flies along);
            every level crossed is ONE tally of plane 0 (direct-down) in the column of the crossing point; the collision deposits the weight
            in the cell where the cumulative optical depth reaches the free path and ends the history
  surface   albedo 0: the photon ends.  Albedo 0.5: weight 0.5, one tally of plane 2 at level 0
  up leg    the same march upwards, tallies in plane 2 (up); ends by collision (deposit 0.5) or through the top
  solvers   (oracle/mi3d_oracle.c: photon_t::ipa, cross_face, advance_inside) 2, independent columns: both legs stay in the start column and
            every tally goes there; 1, partial 3-D: the down leg is 3-D, from the first event on the photon keeps the column of that event
  analytic  the HIP path tallies no direct beam at the levels >= kdir (the top of the voxel layers, lowered through the horizontally uniform
            voxel layers under it; the top level always): the raw plane 0 is exactly 0 there and the read-out adds exp(-tau / mu0).  The oracle
            tallies every level, the top included, and keeps total-down in plane 1

predict() returns a lower and an upper bound of every raw tally element.  A photon on the DROP LIST is uncertain: it adds to no lower bound,
and to the upper bound of every element it might touch -- the 3 x 3 columns around every crossing and every cell of its flight continued
through both legs without a collision.  The list (margin m(t) = M_SCALE (Lx + Ly + t) metres, t the ray parameter; on the up leg t counts
on from the down leg's and m grows by ROT_GROW t, the 32 EPS tests/test_gpu_device_geometry.py allows rotate_dir carried along the ray):

  D_FATE     the free path within FATE_MARGIN relative of the cumulative optical depth at a face the photon passes
  D_POINT    a level-crossing point within m of a column face; the collision point within m of a face of its cell
  D_FACES    two faces of one step closer than m in ray parameter
  D_COLUMN   column-bound legs: the start or reflection point within m of a column face

march() is the float64 flight, flight_emul() the float32 emulation of the kernels' walk (incremental face parameters in walked layers, one
multiply-add per level from where a run of uniform layers was entered) that gives m its confirmation and the path-length heating its scale.
"""

import dataclasses
import functools

import numpy as np

from er3t_amd.scene import TARGET_FLUX, TARGET_HEAT
from tests import geometry_ref as gref
from tests import le_rays_ref as L

F32, F64 = np.float32, np.float64
EPS = 2.0**-24
SCALE = 0.125                 # of every extinction of le_rays_ref.scene
FATE_MARGIN = L.FATE_MARGIN
M_SCALE = 2.0**-18            # m(t) = M_SCALE (Lx + Ly + t): 64 float32 half-ulps of the largest magnitude the walk forms
ROT_GROW = 2.0**-19           # 32 EPS: rotate_dir's allowance, carried along the up leg
D_FATE, D_POINT, D_FACES, D_COLUMN = 1, 2, 4, 8
ALBEDOS = {'black': 0.0, 'lambert': 0.5}
DROP_CAP = 0.03


def scene(variant='base', solver=0, sun=(180.0, 0.0), surface='lambert', hest=0, mix2=False):
    """le_rays_ref.scene as a flux + heating job: no views, wmin = 0, every extinction times SCALE; surface 'black' or 'lambert' (albedo 0.5).
    mix2: the 1-D absorption split over TWO 1-D constituents that do not scatter (the kernels' general mixture, MIX 2)"""
    sc = L.scene(variant, 'solar', 'lambert', solver, views=[], sun=sun, nxr=1, nyr=1)
    kw = dict(target=TARGET_FLUX | TARGET_HEAT, wmin=0.0, abs1d=np.asarray(sc.abs1d)*SCALE, extp=(np.asarray(sc.extp, dtype=F64)*SCALE).astype(F32),
              abst=None if sc.abst is None else (np.asarray(sc.abst, dtype=F64)*SCALE).astype(F32),
              sfc_param=[ALBEDOS[surface], 0, 0, 0, 0], heat_estimator=int(hest))
    if mix2:
        nz = sc.nz
        a = np.asarray(kw['abs1d'], dtype=F64)
        kw.update(abs1d=a*0.0, ext1d=np.stack([a*0.5, a*0.5]), omg1d=np.zeros((2, nz)), apf1d=np.stack([np.full(nz, -1.0), np.full(nz, 0.6)]))
    return dataclasses.replace(sc, **kw)


def kdir_of(sc):
    """DevScene::kdir: direct-beam crossings of the levels >= kdir are not tallied on the HIP path"""
    if sc.nz3 == 0:
        return 0
    walked = L.walked_layers(sc)
    kd = sc.iz3l - 1 + sc.nz3
    while kd > sc.iz3l - 1 and not walked[kd - 1]:
        kd -= 1
    return kd


def direct_levels(sc):
    """(nz + 1,) exp(-tau / mu0) of the direct beam at the levels >= kdir, 0 below: what the read-out adds per unit amplitude"""
    ke = L.extinction(sc)
    zg = np.asarray(sc.zgrd, dtype=F64)
    mu0 = abs(np.cos(np.radians(sc.src_the)))
    out = np.zeros(sc.nz + 1)
    tau = 0.0
    for lev in range(sc.nz, kdir_of(sc) - 1, -1):
        if lev < sc.nz:
            tau += ke[lev, 0, 0]*(zg[lev + 1] - zg[lev])          # (uniform above kdir: any column)
        out[lev] = np.exp(-tau/mu0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the float64 flight
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Legs:
    fate: np.ndarray          # (n,) 0 collision, 1 surface, 2 top
    cell: np.ndarray          # (n, 3) k, iy, ix of the collision
    tend: np.ndarray          # (n,) ray parameter where the leg ends
    drop: np.ndarray          # (n,) bit mask D_*
    cross: dict               # ph, lev, iy, ix, t, x, y of every level crossing, in flight order
    piece: dict               # ph, k, iy, ix, t0, t1 of every piece between two faces (pieces = True)
    org: np.ndarray = None    # (n, 3) start points, (n, 3) directions, (n, 2) iy, ix of the start column
    dirs: np.ndarray = None
    col: np.ndarray = None


def _cat(parts, keys, ints):
    return {k: (np.concatenate([p[k] for p in parts]) if parts else np.zeros(0)).astype(np.int64 if k in ints else F64) for k in keys}


def march(sc, org, dirs, need, column=False, t0=0.0, grow=0.0, pieces=False, max_steps=400000):
    """Rays from org (n, 3) along dirs (n, 3) with free paths need (n,) through the cyclic grid, cut at every x, y and z face (column: at the
    levels only, the ray keeps the column of its start point).  t0 (n,) what the margin's ray parameter starts from; grow its extra slope"""
    ke = L.extinction(sc)
    zg = np.asarray(sc.zgrd, dtype=F64)
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, float(sc.dx), float(sc.dy)
    lxy = nx*dx + ny*dy
    org = np.atleast_2d(np.asarray(org, dtype=F64))
    n = org.shape[0]
    dirs = np.broadcast_to(np.asarray(dirs, dtype=F64), (n, 3))
    need = np.broadcast_to(np.asarray(need, dtype=F64), (n,))
    t0 = np.broadcast_to(np.asarray(t0, dtype=F64), (n,))
    sx, sy, sz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    up = sz > 0.0
    ix, iy, k = L._start_cells(sc, org, dirs)
    if column:
        ix, iy = np.clip(np.floor(org[:, 0]/dx).astype(np.int64), 0, nx - 1), np.clip(np.floor(org[:, 1]/dy).astype(np.int64), 0, ny - 1)
    col0 = np.stack([np.mod(iy, ny), np.mod(ix, nx)], axis=-1)
    t, tau = np.zeros(n), np.zeros(n)
    fate, cell, tend, drop = np.full(n, -1), np.zeros((n, 3), dtype=np.int64), np.zeros(n), np.zeros(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    cr, pc = [], []
    margin = lambda tt, a: M_SCALE*(lxy + t0[a] + tt) + grow*tt
    for _ in range(max_steps):
        a = np.nonzero(alive)[0]
        if not a.size:
            break
        inf = np.full(a.size, np.inf)
        if column:
            tx, ty = inf, inf
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                tx = np.where(sx[a] > 0.0, ((ix[a] + 1)*dx - org[a, 0])/sx[a], np.where(sx[a] < 0.0, (ix[a]*dx - org[a, 0])/sx[a], np.inf))
                ty = np.where(sy[a] > 0.0, ((iy[a] + 1)*dy - org[a, 1])/sy[a], np.where(sy[a] < 0.0, (iy[a]*dy - org[a, 1])/sy[a], np.inf))
        tz = np.where(up[a], (zg[k[a] + 1] - org[a, 2])/sz[a], (zg[k[a]] - org[a, 2])/sz[a])
        tn = np.minimum(np.minimum(tx, ty), tz)
        m = margin(tn, a)
        srt = np.sort(np.stack([tx, ty, tz]), axis=0)
        drop[a] |= np.where(srt[1] - srt[0] < m, D_FACES, 0)
        jy, jx = np.mod(iy[a], ny), np.mod(ix[a], nx)
        kk = ke[k[a], jy, jx]
        tau_new = tau[a] + kk*np.maximum(tn - t[a], 0.0)
        drop[a] |= np.where(np.abs(need[a] - tau_new) <= FATE_MARGIN*tau_new, D_FATE, 0)
        coll = tau_new >= need[a]
        # ---- the collision: the cell where the cumulative optical depth reaches the free path
        c = a[coll]
        if c.size:
            tc = t[c] + (need[c] - tau[c])/kk[coll]
            p = org[c] + dirs[c]*tc[:, None]
            dist = np.minimum(p[:, 2] - zg[k[c]], zg[k[c] + 1] - p[:, 2])
            if not column:
                dist = np.minimum(dist, np.minimum(np.minimum(p[:, 0] - ix[c]*dx, (ix[c] + 1)*dx - p[:, 0]),
                                                   np.minimum(p[:, 1] - iy[c]*dy, (iy[c] + 1)*dy - p[:, 1])))
            drop[c] |= np.where(dist <= margin(tc, c), D_POINT, 0)
            fate[c] = 0; tend[c] = tc; alive[c] = False
            cell[c] = np.stack([k[c], jy[coll], jx[coll]], axis=-1)
            if pieces:
                pc.append(dict(ph=c, k=k[c], iy=jy[coll], ix=jx[coll], t0=t[c], t1=tc))
        # ---- the face
        go = ~coll
        g = a[go]
        if pieces:
            pc.append(dict(ph=g, k=k[g], iy=jy[go], ix=jx[go], t0=t[g], t1=tn[go]))
        tau[g] = tau_new[go]; t[g] = tn[go]
        zf = go & (tz <= tn)
        xf = go & ~zf & (tx <= tn)
        yf = go & ~zf & ~xf
        j = a[zf]
        if j.size:
            x, y = org[j, 0] + sx[j]*tn[zf], org[j, 1] + sy[j]*tn[zf]
            if not column:
                fx, fy = x/dx, y/dy
                near = np.minimum(np.abs(fx - np.round(fx))*dx, np.abs(fy - np.round(fy))*dy) <= m[zf]
                drop[j] |= np.where(near, D_POINT, 0)
            cr.append(dict(ph=j, lev=np.where(up[j], k[j] + 1, k[j]), iy=jy[zf], ix=jx[zf], t=tn[zf], x=x, y=y))
            k[j] += np.where(up[j], 1, -1)
            out = (k[j] < 0) | (k[j] >= nz)
            o = j[out]
            fate[o] = np.where(k[o] < 0, 1, 2); tend[o] = t[o]; alive[o] = False
            k[j] = np.clip(k[j], 0, nz - 1)
        j = a[xf]; ix[j] += np.where(sx[j] > 0.0, 1, -1)
        j = a[yf]; iy[j] += np.where(sy[j] > 0.0, 1, -1)
    else:
        raise RuntimeError('march: a ray did not end')
    ints = ('ph', 'lev', 'iy', 'ix', 'k')
    return Legs(fate=fate, cell=cell, tend=tend, drop=drop, cross=_cat(cr, ('ph', 'lev', 'iy', 'ix', 't', 'x', 'y'), ints),
                piece=_cat(pc, ('ph', 'k', 'iy', 'ix', 't0', 't1'), ints), org=org, dirs=dirs, col=col0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the prediction
# ---------------------------------------------------------------------------------------------------------------------------------------
def reflected_dirs(u2, u3, rounded=True):
    """the direction a Lambert surface sends a photon up in: rotate_dir((0, 0, 1), sqrt(u2), u3), bz = max(bz, 1e-9).  rounded: geometry_ref's
    float32 emulation of rotate_dir / sincos_turns, as float64; else the oracle's float64"""
    n = u2.size
    if rounded:
        mu = np.sqrt(u2.astype(F32)).astype(F32)
        d, _ = gref.rotate_emul(np.tile(F32([0.0, 0.0, 1.0]), (n, 1)), mu, u3.astype(F32))
        d = d.astype(F64)
    else:
        mu = np.sqrt(u2)
        st, phi = np.sqrt(np.maximum(0.0, 1.0 - mu*mu)), 2.0*np.pi*u3
        d = np.stack([st*np.cos(phi), st*np.sin(phi), mu], axis=-1)
        d = d/np.sqrt((d*d).sum(axis=1))[:, None]
    d[:, 2] = np.maximum(d[:, 2], 1e-9)
    return d


@dataclasses.dataclass
class Pred:
    flux_lo: np.ndarray       # (3, nz + 1, ny, nx): every crossing of every level, the top included; planes direct-down, (unused), up
    flux_hi: np.ndarray
    heat_lo: np.ndarray       # (nz, ny, nx) collision estimator
    heat_hi: np.ndarray
    counts: dict              # 'surface', 'top', 'collide', 'tally' (crossings the HIP path tallies, the surface's up tally included): (lo, hi)
    drop: np.ndarray          # (n,) bit mask, 0 = certain
    fate: np.ndarray          # (n, 2) fate of the down and the up leg (-1: no such leg)
    ncross: np.ndarray        # (n,) levels crossed by the down leg (the launch's top level not counted)
    budget: np.ndarray        # (n, 3) weight deposited, absorbed by the surface, escaped
    kdir: int
    path: dict                # hest: 'sum', 'unc' (nz, ny, nx) and the certain photons' terms ph, k, iy, ix, val; else empty
    legs: tuple               # (down, up, ids of the up legs): the float64 legs themselves, for the emulation check

    def certain(self):
        return self.drop == 0

    def dropped_share(self):
        return float((self.drop != 0).mean())

    def gpu_flux(self):
        """bounds of the HIP path's raw flux: no direct tally at the levels >= kdir, nothing in the diffuse-down plane"""
        lo, hi = self.flux_lo.copy(), self.flux_hi.copy()
        lo[0, self.kdir:] = 0.0; hi[0, self.kdir:] = 0.0
        lo[1] = 0.0; hi[1] = 0.0
        return lo, hi

    def oracle_flux(self):
        """bounds of the oracle's raw flux: every level, plane 1 total-down"""
        lo, hi = self.flux_lo.copy(), self.flux_hi.copy()
        lo[1] = lo[0]; hi[1] = hi[0]
        return lo, hi


def _spread(arr, plane, lev, iy, ix, w):
    """add w to the 3 x 3 columns around (iy, ix), cyclic, once per distinct column"""
    ny, nx = arr.shape[-2:]
    for oy in sorted({o % ny for o in (-1, 0, 1)}):
        for ox in sorted({o % nx for o in (-1, 0, 1)}):
            idx = (lev, np.mod(iy + oy, ny), np.mod(ix + ox, nx))
            np.add.at(arr, idx if plane is None else (plane,) + idx, w)


def predict(sc, n, seed, offset=0, rounded=True, pieces=False):
    """bounds of every raw tally of the photons [offset, offset + n) of `seed` in scene sc (one of this module's), and the drop list"""
    nz, nx, ny, dx, dy = sc.nz, sc.nx, sc.ny, float(sc.dx), float(sc.dy)
    Lx, Ly = nx*dx, ny*dy
    zg = np.asarray(sc.zgrd, dtype=F64)
    albedo = min(max(float(F32(sc.sfc_param[0])), 0.0), 1.0)
    ids = np.arange(offset, offset + n, dtype=np.uint64)
    u0, u1, u2 = (L.u01(L.philox(seed, ids, b)) for b in (0, 1, 2))
    x0, y0 = u0[:, 0]*Lx, u0[:, 1]*Ly
    x0, y0 = np.where(x0 >= Lx, 0.0, x0), np.where(y0 >= Ly, 0.0, y0)
    top = np.stack([x0, y0, np.full(n, zg[-1])], axis=-1)
    sun = L.sun_direction(sc, rounded)
    m0 = M_SCALE*(Lx + Ly)

    def near_column_face(x, y, m):
        fx, fy = x/dx, y/dy
        return np.minimum(np.abs(fx - np.round(fx))*dx, np.abs(fy - np.round(fy))*dy) <= m

    def fly(sel, need_dn, need_up):
        """both legs of the photons sel; need = inf: the flight continued without a collision"""
        dn = march(sc, top[sel], sun, need_dn, column=(sc.solver == 2), pieces=pieces)
        if sc.solver == 2:
            dn.drop |= np.where(near_column_face(x0[sel], y0[sel], m0), D_COLUMN, 0)
        r = np.nonzero(dn.fate == 1)[0]
        upl = None
        if albedo > 0.0 and r.size:
            px, py = x0[sel][r] + sun[0]*dn.tend[r], y0[sel][r] + sun[1]*dn.tend[r]
            if sc.solver == 2:        # the column repeated for ever: the point folded into the start column
                cx, cy = np.floor(x0[sel][r]/dx), np.floor(y0[sel][r]/dy)
                px, py = cx*dx + np.mod(px - cx*dx, dx), cy*dy + np.mod(py - cy*dy, dy)
            else:
                px, py = np.mod(px, Lx), np.mod(py, Ly)
            d = reflected_dirs(u1[sel][r, 2], u1[sel][r, 3], rounded)
            o = np.stack([px, py, np.full(r.size, zg[0])], axis=-1)
            upl = march(sc, o, d, need_up[r] if np.ndim(need_up) else need_up, column=(sc.solver != 0), t0=dn.tend[r], grow=ROT_GROW, pieces=pieces)
            if sc.solver != 0:
                upl.drop |= np.where(near_column_face(px, py, M_SCALE*(Lx + Ly + dn.tend[r])), D_COLUMN, 0)
        return dn, r, upl

    allp = np.arange(n)
    dn, r, upl = fly(allp, -np.log(u1[:, 0]), -np.log(u2[:, 0]))
    drop = dn.drop.copy()
    if upl is not None:
        drop[r] |= upl.drop
    ok = drop == 0
    fate = np.full((n, 2), -1); fate[:, 0] = dn.fate
    if upl is not None:
        fate[r, 1] = upl.fate
    kd = kdir_of(sc)
    flux_lo, heat_lo = np.zeros((3, nz + 1, ny, nx)), np.zeros((nz, ny, nx))
    budget = np.zeros((n, 3))
    # ---- certain photons: the launch's top level, the crossings, the deposits
    sx0, sy0 = np.clip(np.floor(x0/dx).astype(int), 0, nx - 1), np.clip(np.floor(y0/dy).astype(int), 0, ny - 1)
    np.add.at(flux_lo, (0, nz, sy0[ok], sx0[ok]), 1.0)
    c = dn.cross; s = ok[c['ph']]
    np.add.at(flux_lo, (0, c['lev'][s], c['iy'][s], c['ix'][s]), 1.0)
    ncross = np.bincount(c['ph'], minlength=n)
    ntally = int((s & (c['lev'] < kd)).sum())
    col = ok & (dn.fate == 0)
    np.add.at(heat_lo, tuple(dn.cell[col].T), 1.0)
    budget[dn.fate == 0, 0] = 1.0
    budget[dn.fate == 1, 1] = 1.0 - albedo
    cnt = {'surface': int((ok & (dn.fate == 1)).sum()), 'collide': int(col.sum()), 'top': 0}
    if upl is not None:
        okr = ok[r]
        np.add.at(flux_lo, (2, 0, np.clip(np.floor(upl.org[okr, 1]/dy).astype(int), 0, ny - 1), np.clip(np.floor(upl.org[okr, 0]/dx).astype(int), 0, nx - 1)), albedo)
        c = upl.cross; s = okr[c['ph']]
        np.add.at(flux_lo, (2, c['lev'][s], c['iy'][s], c['ix'][s]), albedo)
        ntally += int(okr.sum()) + int(s.sum())
        col = okr & (upl.fate == 0)
        np.add.at(heat_lo, tuple(upl.cell[col].T), albedo)
        budget[r[upl.fate == 0], 0] = albedo
        budget[r[upl.fate == 2], 2] = albedo
        cnt['collide'] += int(col.sum()); cnt['top'] = int((okr & (upl.fate == 2)).sum())
    flux_hi, heat_hi = flux_lo.copy(), heat_lo.copy()
    counts = {k_: [v, v] for k_, v in cnt.items()}
    counts['tally'] = [ntally, ntally]
    # ---- uncertain photons: the flight continued through both legs without a collision, 3 x 3 columns around everything it meets
    un = np.nonzero(~ok)[0]
    gdn = gup = None
    if un.size:
        save, pieces = pieces, True
        gdn, gr, gup = fly(un, np.inf, np.inf)
        pieces = save
        _spread(flux_hi, 0, nz, sy0[un], sx0[un], 1.0)
        c = gdn.cross
        _spread(flux_hi, 0, c['lev'], c['iy'], c['ix'], 1.0)
        p = gdn.piece
        _spread(heat_hi, None, p['k'], p['iy'], p['ix'], 1.0)          # (a cell met in several pieces counts more than once: an upper bound)
        nt = int((c['lev'] < kd).sum())
        if gup is not None:
            _spread(flux_hi, 2, 0, np.clip(np.floor(gup.org[:, 1]/dy).astype(int), 0, ny - 1), np.clip(np.floor(gup.org[:, 0]/dx).astype(int), 0, nx - 1), albedo)
            c = gup.cross
            _spread(flux_hi, 2, c['lev'], c['iy'], c['ix'], albedo)
            p = gup.piece
            _spread(heat_hi, None, p['k'], p['iy'], p['ix'], albedo)
            nt += un.size + c['ph'].size
        for key in ('surface', 'collide'):
            counts[key][1] += un.size
        counts['top'][1] += un.size if albedo > 0.0 else 0
        counts['tally'][1] += nt
    path = {}
    if pieces:
        path = _path_heating(sc, dn, r, upl, ok, albedo, top, sun, gdn, gup, un)
    return Pred(flux_lo=flux_lo, flux_hi=flux_hi, heat_lo=heat_lo, heat_hi=heat_hi, counts={k_: tuple(v) for k_, v in counts.items()}, drop=drop,
                fate=fate, ncross=ncross, budget=budget, kdir=kd, path=path, legs=(dn, upl, r))


# ---------------------------------------------------------------------------------------------------------------------------------------
# path-length heating (Flx_mhest = 1): w kappa_a l per flight piece and cell
# ---------------------------------------------------------------------------------------------------------------------------------------
def _layer_pieces(sc, leg, org, dirs):
    """the pieces of a leg as the estimator defines them (include/mi3d.h, mi3d_set_heating_estimator): per cell in the layers walked voxel
    by voxel; ONE piece per horizontally uniform layer, in the column of the piece's midpoint.  Returns ph, k, iy, ix, len, near (the midpoint
    within the margin of a column face)"""
    p = leg.piece
    walked = L.walked_layers(sc)
    nx, ny, dx, dy = sc.nx, sc.ny, float(sc.dx), float(sc.dy)
    w = walked[p['k']]
    out = [dict(ph=p['ph'][w], k=p['k'][w], iy=p['iy'][w], ix=p['ix'][w], len=(p['t1'] - p['t0'])[w], near=np.zeros(int(w.sum()), dtype=bool))]
    u = ~w
    if u.any():
        key = p['ph'][u]*sc.nz + p['k'][u]
        uniq, inv = np.unique(key, return_inverse=True)
        ta, tb = np.full(uniq.size, np.inf), np.full(uniq.size, -np.inf)
        np.minimum.at(ta, inv, p['t0'][u]); np.maximum.at(tb, inv, p['t1'][u])
        ph, k = uniq//sc.nz, uniq % sc.nz
        tm = 0.5*(ta + tb)
        d = np.broadcast_to(dirs, (org.shape[0], 3))
        x, y = org[ph, 0] + d[ph, 0]*tm, org[ph, 1] + d[ph, 1]*tm
        fx, fy = x/dx, y/dy
        near = np.minimum(np.abs(fx - np.round(fx))*dx, np.abs(fy - np.round(fy))*dy) <= M_SCALE*(nx*dx + ny*dy + tm)*2.0
        out.append(dict(ph=ph, k=k, iy=np.mod(np.floor(fy).astype(np.int64), ny), ix=np.mod(np.floor(fx).astype(np.int64), nx), len=tb - ta, near=near))
    return {key: np.concatenate([o[key] for o in out]) for key in out[0]}


def _path_heating(sc, dn, r, upl, ok, albedo, top, sun, gdn, gup, un):
    ke = L.extinction(sc)              # (nothing scatters: kappa_a is the extinction)
    nz, ny, nx = sc.nz, sc.ny, sc.nx
    total, unc = np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx))
    terms = []
    column = sc.solver == 2
    for leg, w, sel, col in ((dn, 1.0, np.arange(top.shape[0]), column), (upl, albedo, r, sc.solver != 0)):
        if leg is None:
            continue
        q = _layer_pieces(sc, leg, leg.org, leg.dirs)
        if col:                   # column-bound: every piece in the leg's column
            q['iy'], q['ix'] = leg.col[q['ph'], 0], leg.col[q['ph'], 1]
            q['near'][:] = False
        good = ok[sel[q['ph']]] & ~q['near']
        val = w*ke[q['k'], q['iy'], q['ix']]*q['len']
        np.add.at(total, (q['k'][good], q['iy'][good], q['ix'][good]), val[good])
        terms.append(dict(ph=sel[q['ph'][good]], k=q['k'][good], iy=q['iy'][good], ix=q['ix'][good], val=val[good], leg=np.full(int(good.sum()), 0 if w == 1.0 else 1)))
        # a certain photon whose midpoint is near a face: that piece alone is uncertain, in the columns around it
        bad = ok[sel[q['ph']]] & q['near']
        _spread(unc, None, q['k'][bad], q['iy'][bad], q['ix'][bad], val[bad])
    # uncertain photons: per layer the whole length of the leg in it, with the largest kappa_a of the 3 x 3 columns around every cell met
    zg = np.asarray(sc.zgrd, dtype=F64)
    kmax = ke.copy()
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            kmax = np.maximum(kmax, np.roll(np.roll(ke, oy, axis=1), ox, axis=2))
    for leg, w in ((gdn, 1.0), (gup, albedo)):
        if leg is None:
            continue
        p = leg.piece
        key = p['ph']*nz + p['k']
        uniq, inv = np.unique(key, return_inverse=True)
        ll = np.zeros(uniq.size); np.add.at(ll, inv, p['t1'] - p['t0'])
        _spread(unc, None, p['k'], p['iy'], p['ix'], w*kmax[p['k'], p['iy'], p['ix']]*ll[inv])
    out = {key: np.concatenate([t_[key] for t_ in terms]) for key in terms[0]}
    out.update(sum=total, unc=unc)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------------
SLANT, VERTICAL, ALONG_X, ALONG_X_NEG0, ALONG_NEG_Y, GRAZING, DIAGONAL = (150.0, 37.0), (180.0, 0.0), (120.0, 0.0), (120.0, -0.0), (120.0, 270.0), (105.0, 200.0), (150.0, 45.0)
TUNING_DEFAULTS = dict(tile_cols=-1, entry_records=1, tally_lists=1, tally_runs=1, tlcap_log2=31)
N_SORTED, N_SMALL = 20000, 3000
SEED, ID0 = 41, 3


@dataclasses.dataclass(frozen=True)
class Launch:
    name: str
    variant: str = 'base'
    solver: int = 0
    sun: tuple = SLANT
    surface: str = 'lambert'
    n: int = N_SORTED
    offset: int = ID0
    seed: int = SEED
    tuning: tuple = ()            # ((knob, value), ...) on top of TUNING_DEFAULTS
    general: bool = False
    hest: int = 0
    mix2: bool = False
    lists: bool = True            # the route's name carries the record lists' kernels

    def scene(self):
        return scene(self.variant, self.solver, self.sun, self.surface, self.hest, self.mix2)

    def kernel(self, counting=False):
        """what mi3d_last_kernel must say"""
        c, p = int(counting), int(self.solver == 1)
        if self.general:
            return 'k_transport<%d,0,1,%d>' % (c, p) + (' [heating: path length]' if self.hest else '')
        mix = 2 if self.mix2 else (1 if self.variant == 'two' else 0)
        return 'k_transport_flux<%d,%d,%d%s>' % (c, p, mix, ',1' if self.hest else '') + (' + k_tl_scatter + k_tl_sum' if self.lists else '')

    def key(self):
        return (self.variant, self.solver, self.sun, str(self.sun[1]), self.surface, self.n, self.seed, self.offset, self.hest, self.mix2)


def _launches():
    out = []
    for surface in ('black', 'lambert'):
        for variant in L.VARIANTS:       # the default flux loop, lists and runs: every scene variant at a slant sun in general position
            out.append(Launch('default-%s-%s' % (variant, surface), variant, surface=surface))
        for variant in ('base', 'stacked'):
            for tag, sun in (('vertical', VERTICAL), ('along_x', ALONG_X), ('along_x_neg0', ALONG_X_NEG0), ('along_neg_y', ALONG_NEG_Y), ('grazing', GRAZING)):
                out.append(Launch('default-%s-%s-%s' % (variant, tag, surface), variant, sun=sun, surface=surface))
        out.append(Launch('default-diag-diagonal-%s' % surface, 'diag', sun=DIAGONAL, surface=surface))
    for variant in ('base', 'stacked'):  # the same job through the other tally routes
        out.append(Launch('no_runs-%s' % variant, variant, tuning=(('tally_runs', 0),)))
        out.append(Launch('atomics-%s' % variant, variant, tuning=(('tally_lists', 0),), lists=False))
        # (lists of fewer than 64 chunks are not kept at all, mi3d_api.hip: tlcap_log2 = 16 is the atomics route again; 17 is the smallest
        #  value with lists, 127 chunks for the 313 waves of the launch: they run full and the rest goes out as atomics)
        out.append(Launch('full_lists-%s' % variant, variant, tuning=(('tlcap_log2', 17),)))
        out.append(Launch('cap16-%s' % variant, variant, tuning=(('tlcap_log2', 16),), lists=False))
        out.append(Launch('small-%s' % variant, variant, n=N_SMALL, lists=False))
        out.append(Launch('offset-%s' % variant, variant, offset=(1 << 33) + 12345))
        out.append(Launch('tiles-%s' % variant, variant, tuning=(('tile_cols', 4),)))
    for solver in (1, 2):                # partial 3-D and independent columns
        for variant in ('base', 'stacked', 'to_surface'):
            for surface in ('black', 'lambert'):
                out.append(Launch('solver%d-%s-%s' % (solver, variant, surface), variant, solver=solver, surface=surface))
        out.append(Launch('solver%d-base-grazing' % solver, solver=solver, sun=GRAZING))
    out.append(Launch('mix2-base', mix2=True))
    out.append(Launch('mix2-stacked-solver1', 'stacked', solver=1, mix2=True))
    for solver in (0, 1, 2):             # the general loop
        for variant in ('base', 'stacked'):
            out.append(Launch('general-%s-solver%d' % (variant, solver), variant, solver=solver, general=True, lists=False))
    out.append(Launch('general-base-grazing-black', sun=GRAZING, surface='black', general=True, lists=False))
    out.append(Launch('general-two', 'two', general=True, lists=False))
    return out


LAUNCHES = _launches()
LAUNCH_IDS = [c.name for c in LAUNCHES]
HEST_LAUNCHES = [Launch('path-%s-%s-solver%d%s' % (variant, surface, solver, '-general' if general else ''), variant, solver=solver, surface=surface, hest=1,
                        general=general, lists=not general)
                 for variant, surface, solver, general in (('base', 'lambert', 0, False), ('stacked', 'black', 0, False), ('stacked', 'lambert', 1, False),
                                                           ('base', 'lambert', 2, False), ('to_surface', 'lambert', 0, False), ('base', 'lambert', 0, True))]
HEST_IDS = [c.name for c in HEST_LAUNCHES]


@functools.lru_cache(maxsize=None)
def _evaluate(key, pieces):
    variant, solver, sun, _, surface, n, seed, offset, hest, mix2 = key
    sc = scene(variant, solver, sun, surface, hest, mix2)
    return sc, predict(sc, n, seed, offset, pieces=pieces)


def evaluate(launch):
    """(scene, Pred) of a launch, shared by the tests of a session and left unchanged"""
    return _evaluate(launch.key(), bool(launch.hest))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the float32 emulation of the flux loops' walk
# ---------------------------------------------------------------------------------------------------------------------------------------
import math
import struct

_pack, _unpack = struct.Struct('f').pack, struct.Struct('f').unpack


def _f(x):
    """a double rounded to float32 (as a Python float: the product of two such values is exact, one rounding makes a fused multiply-add)"""
    return _unpack(_pack(x))[0]


class _Tables:
    """what the kernels hold of a scene: float32 layer table (dz, zlo, bt of uniform layers, tauz, runs), total extinction per cell"""
    def __init__(self, sc):
        self.b = L.extinction32(sc).astype(F64)
        self.walked = L.walked_layers(sc)
        zg = np.asarray(sc.zgrd, dtype=F64)
        self.nz, self.nx, self.ny = sc.nz, sc.nx, sc.ny
        self.dz = [_f(v) for v in np.diff(zg)]
        self.zlo = [_f(v) for v in zg[:-1]]
        self.ztoa = _f(zg[-1])
        self.dx, self.dy = _f(sc.dx), _f(sc.dy)
        self.inv_dx, self.inv_dy = _f(1.0/sc.dx), _f(1.0/sc.dy)
        self.Lx, self.Ly = _f(sc.nx*float(sc.dx)), _f(sc.ny*float(sc.dy))
        self.bt = [float(self.b[k, 0, 0]) for k in range(sc.nz)]
        acc, self.tauz = 0.0, []
        for k in range(sc.nz):
            self.tauz.append(_f(acc))
            if not self.walked[k]:
                acc += self.bt[k]*self.dz[k]
        self.run = {}
        k = 0
        while k < sc.nz:
            if self.walked[k]:
                k += 1
                continue
            e = k
            while e + 1 < sc.nz and not self.walked[e + 1]:
                e += 1
            for j in range(k, e + 1):
                self.run[j] = (k, e)
            k = e + 1


def _emul_leg(T, ix, iy, k, px, py, pz, u, rem, column, t_off=0.0):
    """one flight in float32 with the flux loop's formulas: phase A's voxel steps on incremental face parameters, block B0's runs of uniform
    layers with one multiply-add per level from where the run was entered, fold_xy at its end.  Returns (fate, cell, crossings [(level, iy,
    ix, x, y, t)], pieces [(k, iy, ix, length)] -- per cell in walked layers, per layer at the midpoint's column in uniform ones --, the
    end state (ix, iy, px, py))"""
    ux, uy, uz = u
    up = uz > 0.0
    aux, auy, auz = max(abs(ux), 1e-20), max(abs(uy), 1e-20), max(abs(uz), 1e-20)
    iux, iuy, iuz = _f(1.0/aux), _f(1.0/auy), _f(1.0/auz)
    stepx, stepy = (0, 0) if column else ((1 if ux > 0.0 else -1), (1 if uy > 0.0 else -1))
    stepk = 1 if up else -1
    nx, ny, nz, dx, dy = T.nx, T.ny, T.nz, T.dx, T.dy
    cross, piece = [], []
    tsum = t_off          # (the ray parameter of the whole leg, for the margin: float64 bookkeeping, not part of the emulation)
    clamp = lambda v, hi: min(max(v, 0.0), hi)
    while True:
        if T.walked[k]:
            tx = _f((_f(dx - px) if ux > 0.0 else px)*iux)
            ty = _f((_f(dy - py) if uy > 0.0 else py)*iuy)
            tz = _f((_f(T.dz[k] - pz) if up else pz)*iuz)
            t = 0.0
            while True:
                tn = min(tx, ty, tz)
                bt = float(T.b[k, iy, ix])
                dtau = _f(bt*_f(tn - t))
                if dtau >= rem:
                    piece.append((k, iy, ix, _f(rem*_f(1.0/bt))))
                    return 0, (k, iy, ix), cross, piece, (ix, iy, px, py)
                piece.append((k, iy, ix, _f(tn - t)))
                rem = _f(rem - dtau); t = tn
                zf = tz == tn
                xf = (not zf) and tx == tn
                yf = (not zf) and (not xf)
                if zf:
                    ax, ay = clamp(_f(_f(tx - t)*aux), dx), clamp(_f(_f(ty - t)*auy), dy)
                    cross.append((k + 1 if up else k, iy, ix, ix*dx + (dx - ax if ux > 0.0 else ax), iy*dy + (dy - ay if uy > 0.0 else ay), tsum + t))
                    k += stepk
                    if k < 0 or k >= nz or not T.walked[k]:
                        break
                    tz = _f(T.dz[k]*iuz + tz)
                elif xf:
                    ix = (ix + stepx) % nx
                    tx = _f(dx*iux + tx)
                elif yf:
                    iy = (iy + stepy) % ny
                    ty = _f(dy*iuy + ty)
            # (M_UNIFW: where the walk has ended on a level)
            ax, ay = clamp(_f(_f(tx - t)*aux), dx), clamp(_f(_f(ty - t)*auy), dy)
            px, py = (_f(dx - ax) if ux > 0.0 else ax), (_f(dy - ay) if uy > 0.0 else ay)
            tsum += t
            if k < 0:
                return 1, None, cross, piece, (ix, iy, px, py)
            if k >= nz:
                return 2, None, cross, piece, (ix, iy, px, py)
            pz = 0.0 if up else T.dz[k]
        # ---- B0: the run of uniform layers
        lo_, hi_ = T.run[k]
        kend = hi_ if up else lo_
        if up:
            tv = _f(_f(_f(_f(T.tauz[kend] + _f(T.bt[kend]*T.dz[kend])) - T.tauz[k])) - _f(T.bt[k]*pz))
            hv = _f(_f(T.zlo[kend] + T.dz[kend]) - _f(T.zlo[k] + pz))
        else:
            tv = _f(_f(T.tauz[k] - T.tauz[kend]) + _f(T.bt[k]*pz))
            hv = _f(_f(T.zlo[k] + pz) - T.zlo[kend])
        iuzl = _f(1.0/max(abs(uz), 1e-20))
        tpath = _f(tv*iuzl)
        z0 = _f(T.zlo[k] + pz)
        if tpath < rem:
            rem = _f(rem - tpath)
            s = _f(hv*iuzl)
            kraw = knew = kend + 1 if up else kend - 1
            hk_last, hz_end = kend, (_f(T.zlo[kend] + T.dz[kend]) if up else T.zlo[kend])
            coll = False
            pzn = T.dz[knew] if (not up and 0 <= knew < nz) else 0.0
        else:
            Tt = _f(_f(T.tauz[k] + _f(T.bt[k]*pz)) + _f((rem if up else -rem)*abs(uz)))
            lo, hi = (k, kend) if up else (kend, k)
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if T.tauz[mid] <= Tt:
                    lo = mid
                else:
                    hi = mid - 1
            pzn = min(max(_f(_f(Tt - T.tauz[lo])*_f(1.0/max(T.bt[lo], 1e-30))), 0.0), T.dz[lo])
            s = _f(abs(_f(_f(T.zlo[lo] + pzn) - z0))*iuzl)
            kraw = knew = lo
            hk_last, hz_end = lo, _f(T.zlo[lo] + pzn)
            coll = True
        la, lb = (k + 1, kraw) if up else (kraw + 1, k)
        bx, by = (0.0, 0.0) if column else (_f(ux*iuzl), _f(uy*iuzl))
        order = range(la, lb + 1) if up else range(lb, la - 1, -1)
        for lev in order:
            zl = T.zlo[lev] if lev < nz else T.ztoa
            sl = abs(_f(zl - z0))
            x, y = _f(bx*sl + px), _f(by*sl + py)
            jx, jy = ix, iy
            if not column:
                jx, jy = (ix + int(math.floor(_f(x*T.inv_dx)))) % nx, (iy + int(math.floor(_f(y*T.inv_dy)))) % ny
            cross.append((lev, jy, jx, ix*dx + x, iy*dy + y, tsum + sl*iuzl))
        zlo_f, zhi_f = min(z0, hz_end), max(z0, hz_end)
        for j in range(k, hk_last + (1 if hk_last >= k else -1), 1 if hk_last >= k else -1):
            za, zb = max(T.zlo[j], zlo_f), min(_f(T.zlo[j] + T.dz[j]), zhi_f)
            jx, jy = ix, iy
            if not column:
                sl = _f(abs(_f(_f(0.5*_f(za + zb)) - z0))*iuzl)
                jx = min(max((ix + int(math.floor(_f(_f(ux*sl + px)*T.inv_dx)))) % nx, 0), nx - 1)
                jy = min(max((iy + int(math.floor(_f(_f(uy*sl + py)*T.inv_dy)))) % ny, 0), ny - 1)
            if zb > za:
                piece.append((j, jy, jx, _f(_f(zb - za)*iuzl)))
        px, py = _f(px + _f(ux*s)), _f(py + _f(uy*s))
        fx, fy = math.floor(_f(px*T.inv_dx)), math.floor(_f(py*T.inv_dy))
        px, py = clamp(_f(px - fx*dx), dx), clamp(_f(py - fy*dy), dy)
        if not column:
            ix, iy = (ix + int(fx)) % nx, (iy + int(fy)) % ny
        tsum += s
        if coll:
            return 0, (knew, iy, ix), cross, piece, (ix, iy, px, py)
        if knew >= nz:
            return 2, None, cross, piece, (ix, iy, px, py)
        if knew < 0:
            return 1, None, cross, piece, (ix, iy, px, py)
        k, pz = knew, pzn


def flight_emul(sc, n, seed, offset=0):
    """the histories of the photons [offset, offset + n) in float32, leg by leg: a list per photon of (fate, cell, crossings, pieces) of the
    down leg and, after a reflection, of the up leg"""
    T = _Tables(sc)
    albedo = min(max(float(F32(sc.sfc_param[0])), 0.0), 1.0)
    ids = np.arange(offset, offset + n, dtype=np.uint64)
    u0, u1, u2 = (L.u01(L.philox(seed, ids, b)) for b in (0, 1, 2))
    sun = tuple(float(v) for v in L.sun_direction(sc, True))
    dirs = reflected_dirs(u1[:, 2], u1[:, 3], True)
    # (the free path: -0.69314718f log2(u) with the hardware's log2, good to an ulp: here the correctly rounded one)
    need = lambda u: _f(_f(-0.69314718)*_f(math.log2(u)))
    out = []
    for i in range(n):
        x, y = _f(u0[i, 0]*T.Lx), _f(u0[i, 1]*T.Ly)
        x, y = (0.0 if x >= T.Lx else x), (0.0 if y >= T.Ly else y)
        ix, iy = min(int(_f(x*T.inv_dx)), T.nx - 1), min(int(_f(y*T.inv_dy)), T.ny - 1)
        px, py = min(max(_f(x - _f(ix*T.dx)), 0.0), T.dx), min(max(_f(y - _f(iy*T.dy)), 0.0), T.dy)
        k = T.nz - 1
        legs = [_emul_leg(T, ix, iy, k, px, py, T.dz[k], sun, need(u1[i, 0]), sc.solver == 2)]
        fate, _, _, _, (ix, iy, px, py) = legs[0]
        if fate == 1 and albedo > 0.0:
            tdn = float(sc.zgrd[-1] - sc.zgrd[0])/abs(sun[2])
            legs.append(_emul_leg(T, ix, iy, 0, px, py, 0.0, tuple(float(v) for v in dirs[i].astype(F32)), need(u2[i, 0]), sc.solver != 0, t_off=tdn))
        out.append(legs)
    return out


def emul_check(sc, n, seed, offset=0):
    """The emulation against the float64 flight, over the certain photons of a launch.  Returns a dict: `moved` photons whose emulated
    crossings (level, column), fate or collision cell differ; `disp` the largest displacement of a crossing point over the margin m(t) there;
    `E` the largest error of a cell's path-length heating, the sum of w kappa_a l over the compared photons, relative to that sum (the sum of
    the terms' magnitudes: all are positive); `E_term` the largest relative error of a single term; `photons` compared"""
    p = predict(sc, n, seed, offset, pieces=True)
    em = flight_emul(sc, n, seed, offset)
    dn, upl, r = p.legs
    Lx, Ly = sc.nx*float(sc.dx), sc.ny*float(sc.dy)
    upi = {int(ph): j for j, ph in enumerate(r)}
    moved, disp, E, compared = 0, 0.0, 0.0, 0
    ke = L.extinction(sc)
    albedo = min(max(float(F32(sc.sfc_param[0])), 0.0), 1.0)
    sum_em, sum_ref = np.zeros(ke.shape), np.zeros(ke.shape)
    for leg_no, leg in ((0, dn), (1, upl)):
        if leg is None:
            continue
        c, q = leg.cross, leg.piece
        order = np.argsort(c['ph'], kind='stable')
        cs = {k_: v[order] for k_, v in c.items()}
        starts = np.searchsorted(cs['ph'], np.arange(leg.fate.size + 1))
        lp = _layer_pieces(sc, leg, leg.org, leg.dirs)
        if (sc.solver == 2) if leg_no == 0 else (sc.solver != 0):
            lp['iy'], lp['ix'] = leg.col[lp['ph'], 0], leg.col[lp['ph'], 1]
            lp['near'][:] = False
        po = np.argsort(lp['ph'], kind='stable')
        lps = {k_: v[po] for k_, v in lp.items()}
        pstarts = np.searchsorted(lps['ph'], np.arange(leg.fate.size + 1))
        grow = ROT_GROW if leg_no else 0.0
        for j in range(leg.fate.size):
            ph = j if leg_no == 0 else int(r[j])
            if p.drop[ph] != 0:
                continue
            if leg_no == 1 and (len(em[ph]) < 2):
                moved += 1
                continue
            fate, cell, cross, piece, _ = em[ph][leg_no]
            compared += 1 if leg_no == 0 else 0
            a, b = starts[j], starts[j + 1]
            want = list(zip(cs['lev'][a:b].tolist(), cs['iy'][a:b].tolist(), cs['ix'][a:b].tolist()))
            same = fate == leg.fate[j] and [x[:3] for x in cross] == want and (fate != 0 or tuple(leg.cell[j]) == tuple(cell))
            if not same:
                moved += 1
                continue
            for (lev, jy, jx, x, y, t), xr, yr, tr in zip(cross, cs['x'][a:b], cs['y'][a:b], cs['t'][a:b]):
                ddx = abs((x - xr + 0.5*Lx) % Lx - 0.5*Lx); ddy = abs((y - yr + 0.5*Ly) % Ly - 0.5*Ly)
                if leg_no == 0 and sc.solver == 2 or leg_no == 1 and sc.solver != 0:
                    continue              # (column-bound: the crossing point decides nothing)
                tt = tr + (dn.tend[int(r[j])] if leg_no else 0.0)
                disp = max(disp, max(ddx, ddy)/(M_SCALE*(Lx + Ly + tt) + grow*tr))
            # path-length terms: per (layer, column) of this leg
            a, b = pstarts[j], pstarts[j + 1]
            ref = {}
            for kk, jy, jx, ln, nr in zip(lps['k'][a:b].tolist(), lps['iy'][a:b].tolist(), lps['ix'][a:b].tolist(), lps['len'][a:b].tolist(), lps['near'][a:b].tolist()):
                if nr:
                    ref = None
                    break
                ref[(kk, jy, jx)] = ref.get((kk, jy, jx), 0.0) + ln
            if ref is None:
                continue
            got = {}
            for kk, jy, jx, ln in piece:
                got[(kk, jy, jx)] = got.get((kk, jy, jx), 0.0) + ln
            w = albedo if leg_no else 1.0
            for key, ln in ref.items():
                sum_ref[key] += w*ke[key]*ln
                if ln > 0.0 and ke[key] > 0.0:
                    E = max(E, abs(got.get(key, 0.0) - ln)/ln)
            for key, ln in got.items():
                sum_em[key] += w*ke[key]*ln
    cells = sum_ref > 0.0
    e_cell = float(np.max(np.abs(sum_em - sum_ref)[cells]/sum_ref[cells])) if cells.any() else 0.0
    return dict(moved=moved, disp=float(disp), E=max(e_cell, float(np.abs(sum_em[~cells]).max()) if (~cells).any() else 0.0), E_term=E, photons=compared)


N_EMUL = 3000


@functools.lru_cache(maxsize=None)
def _emul_class(variant, solver, sun, sunkey, surface):
    return emul_check(scene(variant, solver, sun, surface, 1), N_EMUL, SEED, ID0)


def path_scale(launch):
    """E_emul of a path-length launch's class (scene, sun, solver): from the float32 emulation alone"""
    return _emul_class(launch.variant, launch.solver, launch.sun, str(launch.sun[1]), launch.surface)['E']
