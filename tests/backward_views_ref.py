"""
Scenes and an independent float64 reference for the satellite views of a thermal job served backwards (mi3d_set_view_method 1, Rad_mvbwd = 1;
DESIGN.md §5.14; tests/test_backward_views_host.py, tests/test_gpu_backward_views.py).  A view's geometry is worked out here from the scene's
angles alone, by the rules include/mi3d.h states; the radiance along a line is the line integral of tests/thermal_camera_ref.py; a pixel
value is the mean over the pixel's footprint on the registration level, by Gauss-Legendre points in (xr, yr).  Nothing of the solver is used.
"""

import numpy as np

from er3t_amd.scene import Scene, TARGET_RADIANCE
from tests import thermal_camera_ref as ref

WL = 11.0
NXR, NYR = 20, 9          # 3 x 2 tiles of 8 x 8 pixels per view, clipped both ways; neither is the grid's 6 x 5
ZREF = 100.0
# (Rad_the, Rad_phi, Rad_zloc): nadir from above the top; down-looking, sensor zenith angle 40, azimuth 70, from inside the atmosphere;
# up-looking slant from a plane above the surface
VIEWS = [(180.0, 0.0, 1.0e6), (140.0, 70.0, 1000.0), (30.0, 200.0, 150.0)]
ZGRD = np.array([0.0, 200.0, 400.0, 600.0, 800.0, 1100.0, 1500.0])
NX, NY, DX, DY = 6, 5, 300.0, 250.0


def _views(views, nxr, nyr, zref=ZREF):
    return dict(target=TARGET_RADIANCE, rad_kind=2, view_the=[v[0] for v in views], view_phi=[v[1] for v in views],
                view_zloc=[v[2] for v in views], zref=zref, nxr=nxr, nyr=nyr, view_method=1)


def absorbing_scene(views=VIEWS, nxr=NXR, nyr=NYR, albedo=0.0, sfc2d=False):
    """6 x 5 x 4 voxels under two 1-D layers, dx != dy: absorbing voxels (no scattering) with temperature anomalies, two absorbing 1-D
    layers, a lapse rate.  albedo: of the Lambertian surface; sfc2d: a 3 x 2 surface with temperature anomalies (Sfc_tmps2d)"""
    nz = ZGRD.size-1
    yy, xx = np.meshgrid(np.arange(NY), np.arange(NX), indexing='ij')
    ext = np.zeros((1, 4, NY, NX), dtype=np.float32)
    tmpa = np.zeros((4, NY, NX), dtype=np.float32)
    for k3 in range(4):
        blk = (xx+2*yy+k3) % 3
        ext[0, k3] = 0.0002+0.0009*blk
        tmpa[k3] = -2.5*blk+0.5*k3
    absk = np.zeros(nz); absk[4] = 0.002; absk[5] = 0.001
    kw = dict(sfc_mtype=1, sfc_param=[albedo, 0, 0, 0, 0])
    if sfc2d:
        jsfc = np.ones((2, 3), dtype=np.float32)
        psfc = np.zeros((5, 2, 3), dtype=np.float32); psfc[0] = albedo
        kw = dict(jsfc=jsfc, psfc=psfc, tmps2d=np.array([[0.0, 4.0, -3.0], [2.0, -1.0, 5.0]], dtype=np.float32))
    return Scene(zgrd=ZGRD, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=NX, ny=NY, dx=DX, dy=DY,
                 nz3=4, iz3l=1, extp=ext, omgp=np.zeros_like(ext), apfp=np.zeros_like(ext), tmpa3d=tmpa, src_mtype=3, src_wlen=WL,
                 tmp1d=np.array([299.0, 292.0, 290.0, 288.0, 286.0, 283.0, 279.0]), src_the=180.0, src_qmax=0.0, **kw, **_views(views, nxr, nyr))


def opaque_scene(views=VIEWS, nxr=NXR, nyr=NYR, T=285.0):
    """the same grid, isothermal, its top layer with an absorption optical depth of 48: no line of sight escapes, and every history scores
    B(T) to float32"""
    nz = ZGRD.size-1
    ext = np.full((1, 4, NY, NX), 0.0005, dtype=np.float32)
    absk = np.zeros(nz); absk[5] = 48.0/(ZGRD[6]-ZGRD[5])
    return Scene(zgrd=ZGRD, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=NX, ny=NY, dx=DX, dy=DY,
                 nz3=4, iz3l=1, extp=ext, omgp=np.zeros_like(ext), apfp=np.zeros_like(ext), src_mtype=3, src_wlen=WL,
                 tmp1d=np.full(nz+1, T), src_the=180.0, src_qmax=0.0, sfc_mtype=1, sfc_param=[0.0, 0, 0, 0, 0], **_views(views, nxr, nyr))


def scattering_scene(nxr=6, nyr=6):
    """a checkerboard cloud, omega = 0.6, with a tabulated phase function (Henyey-Greenstein g = 0.8 on a one-degree grid) beside an analytic
    Rayleigh constituent in the 1-D layers; views 1 and 2"""
    nz = ZGRD.size-1
    yy, xx = np.meshgrid(np.arange(NY), np.arange(NX), indexing='ij')
    ext = np.zeros((1, 4, NY, NX), dtype=np.float32)
    for k3 in (1, 2):
        ext[0, k3] = 0.004*((xx+yy+k3) % 2)
    ang = np.arange(181.0)
    g = 0.8
    pha = (1.0-g*g)/(1.0+g*g-2.0*g*np.cos(np.radians(ang)))**1.5
    absk = np.zeros(nz); absk[0] = 0.0003; absk[5] = 0.0002
    return Scene(zgrd=ZGRD, ext1d=np.full(nz, 2.0e-5), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=NX, ny=NY, dx=DX, dy=DY,
                 nz3=4, iz3l=1, extp=ext, omgp=np.full_like(ext, 0.6), apfp=np.full_like(ext, 1.0), ang=ang, pha=pha[None], src_mtype=3,
                 src_wlen=WL, tmp1d=np.array([299.0, 292.0, 290.0, 288.0, 286.0, 283.0, 279.0]), src_the=180.0, src_qmax=0.0, sfc_mtype=1,
                 sfc_param=[0.1, 0, 0, 0, 0], **_views(VIEWS[:2], nxr, nyr))


def view_geometry(sc, iv):
    """(v, zs, zreg) of view iv by the rules of include/mi3d.h (mi3d_set_view_method): v the unit vector towards the sensor (an all but
    vertical one snapped), zs the sensor plane, zreg the registration level -- float64 of the float32 values the device holds"""
    t, p = np.radians(sc.view_the[iv]), np.radians(sc.view_phi[iv])
    v = np.array([-np.sin(t)*np.cos(p), -np.sin(t)*np.sin(p), -np.cos(t)])
    if abs(v[0]) < 1e-7 and abs(v[1]) < 1e-7:
        v = np.array([0.0, 0.0, 1.0 if v[2] > 0.0 else -1.0])
    ztoa, zsfc = float(sc.zgrd[-1]), float(sc.zgrd[0])
    zs = min(float(sc.view_zloc[iv]), ztoa)
    if v[2] <= 0.0:
        zs = max(zs, zsfc)
    zreg = float(sc.zref) if v[2] > 0.0 else zs
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return f(v), float(f(zs)), float(f(zreg))


def start_points(sc, iv, xr, yr):
    """where the lines of sight through the points (xr, yr) of the registration level meet the sensor plane, folded into the domain: (n, 3)"""
    v, zs, zreg = view_geometry(sc, iv)
    Lx, Ly = sc.nx*sc.dx, sc.ny*sc.dy
    t = (zs-zreg)/v[2]
    x, y = np.mod(np.asarray(xr, dtype=np.float64)+v[0]*t, Lx), np.mod(np.asarray(yr, dtype=np.float64)+v[1]*t, Ly)
    return np.stack([x, y, np.full(x.shape, zs)], axis=-1)


def _breaks(sc, iv, axis):
    """where, along xr (axis 0) or yr (1), the lines of sight of view iv change the ORDER in which they cross a level and a cell face of that
    axis -- the points m d - v_axis / vz (z_l - zreg) for every level z_l, the sensor plane among them: between two of them, and at a fixed
    value of the other coordinate, the radiance is smooth but for the kinks where a line crosses an x and a y face at once"""
    v, zs, zreg = view_geometry(sc, iv)
    L, d, n = ((sc.nx*sc.dx, sc.dx, sc.nx), (sc.ny*sc.dy, sc.dy, sc.ny))[axis]
    b = [np.mod(np.arange(n)*d-v[axis]/v[2]*(zl-zreg), L) for zl in list(np.asarray(sc.zgrd, dtype=np.float64))+[zs, zreg]]
    return np.unique(np.round(np.concatenate(b), 9))


def _pixel_points(npx, L, bk, nq):
    """Gauss-Legendre points of every pixel of one image axis, nq per piece of the pixel between two break points: (points, weights that add
    to 1 per pixel, the pixel each belongs to)"""
    g, w = np.polynomial.legendre.leggauss(nq)
    X, W, I = [], [], []
    for i in range(npx):
        a, b = i*L/npx, (i+1)*L/npx
        e = np.concatenate([[a], bk[(bk > a) & (bk < b)], [b]])
        for lo, hi in zip(e[:-1], e[1:]):
            X.append(lo+0.5*(g+1.0)*(hi-lo)); W.append(0.5*w*(hi-lo)/(b-a)); I.append(np.full(nq, i))
    return np.concatenate(X), np.concatenate(W), np.concatenate(I)


def view_image(sc, iv, nq, refl=None):
    """the image (nyr, nxr) of view iv of a non-scattering scene: per pixel the mean over its footprint on the registration level of the
    radiance along the view direction, by nq x nq Gauss-Legendre points in (xr, yr) on every piece of the pixel between the break points
    of either axis (_breaks)"""
    v, zs, zreg = view_geometry(sc, iv)
    if v[2] < 0.0 and zs >= float(sc.zgrd[-1]):
        return np.zeros((sc.nyr, sc.nxr))
    x, wx, ix = _pixel_points(sc.nxr, sc.nx*sc.dx, _breaks(sc, iv, 0), nq)
    y, wy, iy = _pixel_points(sc.nyr, sc.ny*sc.dy, _breaks(sc, iv, 1), nq)
    Y, X = np.meshgrid(y, x, indexing='ij')
    org = start_points(sc, iv, X.ravel(), Y.ravel())
    R = ref.march(sc, org, np.broadcast_to(-v, org.shape), refl=refl).reshape(y.size, x.size)
    img = np.zeros((sc.nyr, sc.nxr))
    np.add.at(img, (iy[:, None], ix[None, :]), R*wy[:, None]*wx[None, :])
    return img
