"""
Point radiometers on the GPU (include/mi3d.h: mi3d_set_camera_map, mi3d_get_camera_direct): the rectangular map's exact binning,
irradiance against the flux grid and the analytic direct beam, the direct sun through a 3-D column against a ray march written
here, actinic flux against the polar camera, existing cameras unchanged, and two ranks against one.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import TARGET_FLUX, TARGET_RADIANCE
from tests.util import slab_scene

pytestmark = pytest.mark.gpu


def _sol():
    from er3t_amd.solver import Mi3dSolver
    return Mi3dSolver(device=0)


def cameras(base, the, zloc, xpos=0.5, ypos=0.5, mpmap=2, mrproj=1, nxr=1, nyr=1, umax=90.0, vmax=180.0, qmax=180.0, apsize=0.05,
            phi=0.0, psi=0.0):
    the = list(np.atleast_1d(np.asarray(the, dtype=float)))
    n = len(the)
    per = lambda v: list(np.resize(np.atleast_1d(np.asarray(v, dtype=float)), n))
    return dataclasses.replace(base, target=TARGET_RADIANCE, rad_kind=1, view_the=the, view_phi=per(phi), view_zloc=per(zloc),
                               cam_xpos=per(xpos), cam_ypos=per(ypos), cam_psi=per(psi), cam_qmax=per(qmax), cam_umax=per(umax),
                               cam_vmax=per(vmax), cam_apsize=per(apsize), nxr=nxr, nyr=nyr, cam_mpmap=mpmap, cam_mrproj=mrproj)


def rect_w(n, m, umax=90.0, vmax=180.0, mrproj=1):
    t = np.radians(umax)*np.arange(n+1)/n
    dphi = 2.0*np.radians(vmax)/m
    w = (np.cos(t[:-1])-np.cos(t[1:]))*dphi if mrproj == 0 else 0.5*(np.sin(t[1:])**2-np.sin(t[:-1])**2)*dphi
    return np.repeat(w[None, :], m, axis=0)             # (nyr, nxr): the image's layout


def run(sol, scene, nph, seed, direct=True):
    sol.load_scene(scene)
    sol.reset()
    sol.run(nph, seed=seed)
    rad = sol.radiance(nph).astype(np.float64)
    return (rad, sol.camera_direct()) if direct else rad


# a horizontally uniform Rayleigh + absorbing atmosphere over a Lambert surface (a 3-D grid of one layer holding the same medium)
def uniform(target, tau=0.5, omega=0.9, albedo=0.3, sza=30.0, apf=-1.0):
    return slab_scene(tau=tau, omega=omega, apf=apf, albedo=albedo, sza=sza, nz=4, ztop=4000.0, nx=2, ny=2, nz3=1, dx=20000.0,
                      dy=20000.0, target=target, vza=(0.0,))


def batches(sol, scene, nb, nph, seed, post):
    xs = np.array([post(*run(sol, scene, nph, seed+i)) for i in range(nb)])
    return xs.mean(axis=0), xs.std(axis=0, ddof=1)/np.sqrt(nb)


def test_rectangular_binning_is_exact():
    """the same photon histories binned into 1 x 1 and 9 x 36 hemisphere pixels: sum(value W) is the same number"""
    sol = _sol()
    base = uniform(TARGET_RADIANCE)
    for mrproj, whemi in ((1, np.pi), (0, 2.0*np.pi)):
        one, _ = run(sol, cameras(base, 0.0, 1.0, mrproj=mrproj), 400000, 21)
        fine, _ = run(sol, cameras(base, 0.0, 1.0, mrproj=mrproj, nxr=9, nyr=36), 400000, 21)
        assert fine.shape == (1, 36, 9) and np.count_nonzero(fine) > 200
        a, b = (fine[0]*rect_w(9, 36, mrproj=mrproj)).sum(), one[0, 0, 0]*whemi
        assert a > 0.0 and abs(a/b-1.0) < 1.0e-5, (mrproj, a, b)


def camera_axes(the, phi, psi):
    """image x, image y and the axis of a camera: the world axes turned by Rz(phi) Ry(the) Rz(psi) (include/mi3d.h: mi3d_set_cameras)"""
    def rz(a):
        c, s = np.cos(np.radians(a)), np.sin(np.radians(a))
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(np.radians(the)), np.sin(np.radians(the))
    R = rz(phi) @ np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ rz(psi)
    return R[:, 0], R[:, 1], R[:, 2]


@pytest.mark.parametrize('case', [
    dict(sun_phi=203.0, cam=(0.0, 0.0, 0.0), n=(9, 36), umax=90.0, vmax=180.0, mrproj=1),     # looking up, the sun at theta 33, phi 23
    dict(sun_phi=20.0, cam=(25.0, 60.0, 30.0), n=(7, 20), umax=80.0, vmax=150.0, mrproj=0),  # a tilted and turned camera, a narrower map
    dict(sun_phi=0.0, cam=(0.0, 0.0, 0.0), n=(9, 36), umax=90.0, vmax=180.0, mrproj=1)])      # the sun at phi = 180: the first row
def test_sun_lands_in_its_rectangular_pixel(case):
    """the direct sun (noise-free) in a multi-pixel rectangular image: exactly one pixel, the one at (floor(theta / dtheta),
    floor((phi + vmax) / dphi)) in the camera's own axes, holding Src_flx exp(-tau) w / W_ij"""
    sza = 33.0
    base = dataclasses.replace(uniform(TARGET_RADIANCE, sza=sza), src_phi=case['sun_phi'])
    the, phi, psi = case['cam']
    nxr, nyr = case['n']
    sc = cameras(base, the, 1.0, phi=phi, psi=psi, nxr=nxr, nyr=nyr, umax=case['umax'], vmax=case['vmax'], mrproj=case['mrproj'])
    sol = _sol()
    sol.load_scene(sc)
    d = sol.camera_direct()[0]
    th, ph = np.radians(180.0-sza), np.radians(case['sun_phi'])
    s = -np.array([np.sin(th)*np.cos(ph), np.sin(th)*np.sin(ph), np.cos(th)])
    X, Y, Z = camera_axes(the, phi, psi)
    theta, azi = np.degrees(np.arccos(s @ Z)), np.degrees(np.arctan2(s @ Y, s @ X))
    u, v = theta/(case['umax']/nxr), (azi+case['vmax'])/(2.0*case['vmax']/nyr)
    ir, jr = int(np.floor(u)), int(np.floor(v)) % nyr
    if case['sun_phi'] != 0.0:
        assert min(u-np.floor(u), np.ceil(u)-u, v-np.floor(v), np.ceil(v)-v) > 1e-3      # (not on a pixel edge)
    else:
        assert abs(abs(azi)-180.0) < 1e-9 and jr == 0
    assert np.count_nonzero(d) == 1 and d[jr, ir] > 0.0, (np.argwhere(d), jr, ir)
    tau = 0.5*(1.0-1.0/4000.0)/s[2]
    w = np.cos(np.radians(theta)) if case['mrproj'] == 1 else 1.0
    want = np.exp(-tau)*w/rect_w(nxr, nyr, case['umax'], case['vmax'], case['mrproj'])[jr, ir]
    assert abs(d[jr, ir]/want-1.0) < 2e-6, (d[jr, ir], want)


def test_irradiance_against_the_flux_grid():
    sol = _sol()
    nb, nph = 4, 1000000
    flux_sc = uniform(TARGET_FLUX)
    fl = []
    for i in range(nb):
        sol.load_scene(flux_sc); sol.reset(); sol.run(nph, seed=50+i)
        f = sol.flux(nph).astype(np.float64)
        fl.append([(f[1, 0]-f[0, 0]).mean(), f[2, -1].mean()])
    fl = np.array(fl)
    dn_m, up_m = fl.mean(axis=0)
    dn_e, up_e = fl.std(axis=0, ddof=1)/np.sqrt(nb)
    # up-looking sensor just above the surface, down-looking one at the top of the atmosphere
    sc = cameras(uniform(TARGET_RADIANCE), [0.0, 180.0], [1.0, 4000.0])
    mean, err = batches(sol, sc, nb, nph, 70, lambda r, d: np.concatenate([np.pi*r[:, 0, 0], np.pi*d[:, 0, 0]]))
    f_dif_up, f_dif_top, f_dir_up, f_dir_top = mean
    mu0 = np.cos(np.radians(30.0))
    tau_above = 0.5*(1.0-1.0/4000.0)                                 # the sensor stands 1 m above the surface
    assert abs(f_dir_up/(mu0*np.exp(-tau_above/mu0))-1.0) < 1.0e-5, f_dir_up
    assert f_dir_top == 0.0                                           # the sun is not in a down-looking sensor's hemisphere
    assert abs(f_dif_up-dn_m) < 4.0*np.hypot(err[0], dn_e), (f_dif_up, err[0], dn_m, dn_e)
    assert abs(f_dif_top-up_m) < 4.0*np.hypot(err[1], up_e), (f_dif_top, err[1], up_m, up_e)


def march_tau(sc, x, y, z, s):
    """optical depth from (x, y, z) to the top of the atmosphere along s, sampled finely (an independent restatement: 1 mm steps
    in the 3-D layers would be slow, so the path is cut at every x, y and z cell boundary it crosses and summed piece by piece)"""
    zg = sc.zgrd
    k3lo, nz3 = sc.iz3l-1, sc.nz3
    bt1 = (sc.abs1d.astype(np.float64)+sc.ext1d.astype(np.float64).sum(axis=0)).astype(np.float32).astype(np.float64)
    bext = (bt1[k3lo:k3lo+nz3, None, None].astype(np.float32)+sc.extp.sum(axis=0)).astype(np.float64)     # (nz3, ny, nx)
    tz = (zg[-1]-z)/s[2]
    ts = [0.0, tz]
    for axis, d, n in ((0, sc.dx, sc.nx), (1, sc.dy, sc.ny)):
        p0, p1 = (x, y)[axis], (x, y)[axis]+s[axis]*tz
        lo, hi = sorted((p0, p1))
        ts += [(b*d-p0)/s[axis] for b in range(int(np.ceil(lo/d)), int(np.floor(hi/d))+1)] if s[axis] != 0.0 else []
    ts += [(zz-z)/s[2] for zz in zg if z < zz < zg[-1]]
    ts = np.unique(np.clip(ts, 0.0, tz))
    tau = 0.0
    for t0, t1 in zip(ts[:-1], ts[1:]):
        tm = 0.5*(t0+t1)
        px, py, pz = x+s[0]*tm, y+s[1]*tm, z+s[2]*tm
        k = int(np.searchsorted(zg, pz, side='right'))-1
        if k3lo <= k < k3lo+nz3:
            b = bext[k-k3lo, int(np.floor(py/sc.dy)) % sc.ny, int(np.floor(px/sc.dx)) % sc.nx]
        else:
            b = bt1[k]
        tau += b*(t1-t0)
    return tau


def test_direct_sun_through_a_cloud_column():
    sza = 40.0
    base = slab_scene(tau=0.1, omega=1.0, apf=0.85, sza=sza, nz=10, ztop=2000.0, nx=10, ny=10, nz3=5, dx=100.0, dy=100.0,
                      target=TARGET_RADIANCE)
    extp = base.extp.copy()
    extp[0, :, 5, 5] = 0.02                                           # one opaque column: vertical optical depth 20
    base = dataclasses.replace(base, extp=extp)
    # photons travel towards phi = 270 (-y): the sun stands towards +y.  Sensor 0 looks at it through the column, sensor 1 past it
    xs, ys = np.array([550.0, 250.0]), np.array([300.0, 300.0])
    sc = cameras(base, [0.0, 0.0], [1.0, 1.0], xpos=xs/1000.0, ypos=ys/1000.0)
    sol = _sol()
    sol.load_scene(sc)
    d = sol.camera_direct()
    th = np.radians(180.0-sza); ph = np.radians(270.0)
    s = -np.array([np.sin(th)*np.cos(ph), np.sin(th)*np.sin(ph), np.cos(th)])
    mu0 = s[2]
    for i in range(2):
        tau = march_tau(sc, float(np.float32(xs[i])), float(np.float32(ys[i])), 1.0, s)
        want = mu0*np.exp(-tau)
        assert abs(np.pi*d[i, 0, 0]/want-1.0) < 1.0e-5, (i, tau, np.pi*d[i, 0, 0], want)
        if i == 0:
            assert tau > 3.0                                          # the line of sight crosses the column
        else:
            assert abs(tau-0.1*(1.0-1.0/2000.0)/mu0) < 1e-6                 # the clear sky's slant optical depth


def test_actinic_flux():
    """2 pi x the hemispherical mean of the polar camera's image (the same histories) = the actinic sensor's diffuse part;
    actinic >= irradiance; under a thick conservative layer the ratio of the two tends to 2"""
    sol = _sol()
    base = uniform(TARGET_RADIANCE)
    nph = 1000000
    act, act_dir = run(sol, cameras(base, 0.0, 1.0, mrproj=0), nph, 91)
    n = 60
    pol = run(sol, cameras(base, 0.0, 1.0, mpmap=1, mrproj=0, nxr=n, nyr=n, umax=180.0, vmax=180.0), nph, 91, direct=False)
    c = (np.arange(n)+0.5)/n*np.pi-0.5*np.pi
    th = np.hypot(c[None, :], c[:, None])
    dudv = (np.pi/n)**2
    integral = (pol[0]*dudv*np.where(th > 0.0, np.sin(th)/th, 1.0)).sum()
    assert abs(2.0*np.pi*act[0, 0, 0]/integral-1.0) < 0.01, (2.0*np.pi*act[0, 0, 0], integral)
    irr, irr_dir = run(sol, cameras(base, 0.0, 1.0, mrproj=1), nph, 91)
    assert 2.0*np.pi*(act+act_dir)[0, 0, 0] >= np.pi*(irr+irr_dir)[0, 0, 0]
    assert abs(2.0*np.pi*act_dir[0, 0, 0]/(np.pi*irr_dir[0, 0, 0]*1.0/np.cos(np.radians(30.0)))-1.0) < 1e-5
    # a conservative layer of optical depth 10 from 2 to 4 km over clear air and a bright surface: below it the light is nearly
    # isotropic (the sensor sees no event close by: the estimator's 1 / r^2 stays tame)
    thick = uniform(TARGET_RADIANCE, tau=20.0, omega=1.0, albedo=0.9, apf=0.0)
    ext1d = thick.ext1d.copy(); ext1d[0, :2] = 0.0
    thick = dataclasses.replace(thick, ext1d=ext1d, extp=np.zeros_like(thick.extp))
    a, ad = run(sol, cameras(thick, 0.0, 1.0, mrproj=0), 400000, 93)
    i, idr = run(sol, cameras(thick, 0.0, 1.0, mrproj=1), 400000, 93)
    ratio = 2.0*(a+ad)[0, 0, 0]/(i+idr)[0, 0, 0]
    print('actinic / irradiance under the thick layer: %.4f' % ratio)
    assert 1.85 < ratio < 2.02, ratio


def test_polar_cameras_unchanged():
    """a polar all-sky job: the same image whether the map is left alone or set to (1, 0) after another map was used"""
    sol = _sol()
    sc = cameras(uniform(TARGET_RADIANCE), 0.0, 1.0, mpmap=1, mrproj=0, nxr=32, nyr=32, umax=180.0, vmax=180.0, qmax=178.0)
    a = run(sol, sc, 300000, 5, direct=False)
    sol.set_camera_map(2, 0)
    sol.prepare()
    sol.set_camera_map(1, 0)
    sol.reset(); sol.run(300000, seed=5)
    b = sol.radiance(300000).astype(np.float64)
    assert np.count_nonzero(a) > 500 and np.array_equal(a, b)
    # the polar map with mrproj = 1: the cosine weight cancels against the per-direction denominator
    sol.set_camera_map(1, 1)
    sol.reset(); sol.run(300000, seed=5)
    c = sol.radiance(300000).astype(np.float64)
    assert np.allclose(a, c, rtol=1e-5, atol=0.0)


def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on this box's one GPU) against one rank on the same photon ids: the
    direct part is added once, on the batched file route and on the fused route (tests/radiometer_dist_worker.py)"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'radiometer_dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(out, 'result.npz'))
    for v in ('rad', 'rdir'):
        a, b = z['job_dist_'+v], z['job_solo_'+v]
        assert a.shape == b.shape and a.max() > 0.0 and np.allclose(a, b, rtol=2e-3, atol=0.0), (v, a, b)
    assert np.array_equal(z['job_dist_rdir'], z['job_solo_rdir'])
    for v in ('f', 'f_diffuse', 'f_direct'):
        a, b = z['file_'+v], z['fused_'+v]
        assert a.shape == b.shape == (4,)
        if v == 'f_direct':
            assert a.min() > 0.0 and np.allclose(a, b, rtol=1e-5, atol=0.0), (a, b)     # known, no noise: added once
        else:
            assert np.allclose(a, b, rtol=0.1, atol=0.0), (v, a, b)                    # different seeds
