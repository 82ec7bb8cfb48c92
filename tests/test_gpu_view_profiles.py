"""
Per-layer profiles of the backward route's satellite views on the GPU (mi3d_set_view_profiles 1, Rad_mvprf = 1): the weighting
function K[pixel][layer | surface] and the contribution C[pixel][layer | surface] of k_backward_vp.

  1  partition       Src_flx sum_k C = the radiance, raw and through the read-outs, for any temperatures
  2  float64         single histories against the per-layer sums of the line's float64 weights
  3  opaque          sum_k K = 1 and C / K = B(T) in an isothermal scene under an opaque layer
  4  Jacobian        K against the plain route by finite differences of a layer's and of the surface's temperature
  5  hand-out        every chunk, batch and id offset gives the same raw tallies, and id ranges add
  6  switch          the switch, its refusals and those of the route
  7  two ranks       sharded ids all-reduced against one rank (tests/view_profiles_dist_worker.py)
  8  drop-in         mcarats_ng(view_profiles=True) through files and fused, mca_out_ng's keys

The scenes are those of tests/backward_views_ref.py: 6 x 5 x 4 voxels under two 1-D layers, 20 x 9 pixels, three views.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import TARGET_FLUX
from er3t_amd.thermal import planck
from tests import backward_views_ref as vref
from tests import thermal_camera_ref as ref
from tests import view_profiles_ref as pref
from tests.test_gpu_backward import _march32

pytestmark = pytest.mark.gpu

NAME = 'k_backward<0,V,P> [thermal]'
PLAIN = 'k_backward<0,V> [thermal]'
U24 = 2.0**-24


@pytest.fixture(autouse=True)
def defaults_again(solver):
    solver.set_counting(False)               # (the solver is the session's: a test before this file may have left the counting builds on)
    solver.set_kernel(general=False)
    yield
    solver.bind(None, None, None)
    solver.set_tuning(bwd_chunk=-1, batch_log2=30)
    solver.set_counting(False)
    solver.set_emission_weights(False)
    solver.set_view_profiles(False)
    solver.set_view_method('forward')


def _on(sc, **kw):
    return dataclasses.replace(sc, view_profiles=1, **kw)


def _raw(solver, sc, ranges, seed, chunk=-1, lg=30):
    """the raw tallies of the scene's job over the id ranges [(offset, n), ...] through bound buffers: (rad [npix], P [npix][nz + 1][2] or None
    where the scene's switch is off) float64, and the kernel's name"""
    import torch
    npix, nrow = sc.nview*sc.nxr*sc.nyr, sc.nz+1
    on = bool(sc.view_profiles)
    rad = torch.zeros(npix, dtype=torch.float64, device='cuda:0')
    prf = torch.zeros(npix*nrow*2, dtype=torch.float64, device='cuda:0') if on else None
    try:
        solver.bind(rad.data_ptr(), None, None, prf_ptr=None if prf is None else prf.data_ptr())
        solver.set_tuning(bwd_chunk=chunk, batch_log2=lg)
        solver.load_scene(sc); solver.reset()
        for off, n in ranges:
            solver.run(n, seed=seed, offset=off)
        solver.sync()
        torch.cuda.synchronize()
        name = solver.kernel_name()
        assert solver.debug_backward_views(seed, 0, 0)[3] == 0       # no history was capped
        return rad.cpu().numpy().copy(), (prf.cpu().numpy().reshape(npix, nrow, 2).copy() if on else None), name
    finally:
        solver.bind(None, None, None)


# ---- 1: the partition ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['absorbing', 'scattering'])
def test_contributions_add_up_to_the_radiance_for_any_temperatures(solver, which):
    """the terms of C are the very terms of the score: raw, Src_flx sum_k C_raw is the raw image up to the order of float64 sums of
    non-negative terms (rtol 1e-12); through the read-outs both sides are rounded to float32 -- the image once, every row of C once,
    2^-24 each, so 2^-23 = 1.2e-7 in all: rtol 3e-7.  Src_flx = 2.5 in the scattering case"""
    if which == 'absorbing':
        sc, flx = _on(pref.with_anomalies(vref.absorbing_scene(sfc2d=True, albedo=0.2), seed=11)), 1.0
    else:
        sc, flx = _on(pref.with_anomalies(vref.scattering_scene(), seed=12), src_flx=2.5), 2.5
    npix = sc.nview*sc.nxr*sc.nyr
    N = 40*npix+13
    rad, P, name = _raw(solver, sc, [(0, N)], seed=101)
    assert name == NAME, name
    tot = flx*P[:, :, 1].sum(axis=1)
    print('partition (%s): %d pixels, raw: largest |Src_flx sum C / rad - 1| %.3e (allowed 1e-12)' % (which, npix, np.abs(tot/rad-1.0).max()))
    assert rad.min() > 0.0 and P.min() >= 0.0 and np.all(P[:, :, 0].sum(axis=1) > 0.0)
    assert np.allclose(tot, rad, rtol=1.0e-12, atol=0.0)
    # the public read-outs (the library's own tally this time)
    solver.load_scene(sc); solver.reset(); solver.run(N, seed=101)
    r = solver.radiance(N).astype(np.float64)
    p = solver.view_profiles(N)
    assert solver.kernel_name() == NAME
    assert p['weight'].shape == p['contribution'].shape == (sc.nview, sc.nyr, sc.nxr, sc.nz+1) and p['weight'].dtype == np.float32
    tot = flx*p['contribution'].astype(np.float64).sum(axis=-1)
    print('partition (%s): read-outs: largest |Src_flx sum C / rad - 1| %.3e (allowed 3e-7)' % (which, np.abs(tot/r-1.0).max()))
    assert np.allclose(tot, r, rtol=3.0e-7, atol=0.0)
    # ... and they are the raw tallies divided by the pixels' own counts, rounded once
    cnt = (N//npix+(np.arange(npix) < N % npix)).astype(np.float64)
    assert np.allclose(p['weight'].reshape(npix, -1), P[:, :, 0]/cnt[:, None], rtol=2.0*U24, atol=0.0)
    assert np.allclose(p['contribution'].reshape(npix, -1), P[:, :, 1]/cnt[:, None], rtol=2.0*U24, atol=0.0)


# ---- 2: single histories against float64 ---------------------------------------------------------------------------------------------------------

def test_single_histories_against_the_float64_line(solver):
    """a scene that never scatters over a black surface, one history per pixel: its rows are the per-layer sums of the float64 weights of the
    very line mi3d_debug_backward_views reports.  Tolerance: that of test_gpu_backward_views.py's single-history scores -- four times the gap
    of the float32 restatement of the walk (_march32) to the float64 march --, taken, like the per-cell comparison of
    test_gpu_emission_weights.py, relative to the line's total (sum_k K_ref, sum_k C_ref): what float32 misplaces is a piece of path at a face,
    which is as large for a thin row as for the whole line"""
    sc = _on(vref.absorbing_scene(albedo=0.0))
    npix, nz = sc.nview*sc.nxr*sc.nyr, sc.nz
    rad, P, name = _raw(solver, sc, [(0, npix)], seed=83)
    assert name == NAME
    st, d, score, capped = solver.debug_backward_views(83, 0, npix)
    assert capped == 0
    K_ref, C_ref = pref.line_profiles(sc, st.astype(np.float64), d.astype(np.float64))
    want = ref.march(sc, st.astype(np.float64), d.astype(np.float64))
    gap32 = np.abs(_march32(sc, st, d)/want-1.0).max()
    tol = 4.0*gap32
    assert np.allclose(C_ref.sum(axis=1), want, rtol=1.0e-12, atol=0.0)           # (the helper against the march it is summed from)
    K, C = P[:, :, 0], P[:, :, 1]
    gK = np.abs(K-K_ref)/K_ref.sum(axis=1)[:, None]
    gC = np.abs(C-C_ref)/C_ref.sum(axis=1)[:, None]
    print('single histories: %d lines; float32 restatement: gap %.3e; rows of K: %.3e, rows of C: %.3e (allowed %.3e)' % (npix, gap32, gK.max(), gC.max(), tol))
    assert 1.0e-9 < gap32 < 1.0e-5 and np.allclose(rad, score, rtol=1.0e-15, atol=0.0)
    never = K_ref == 0.0
    assert never.sum() == 2*sc.nxr*sc.nyr and np.all(K[never] == 0.0) and np.all(C[never] == 0.0)       # (view 2 starts below the top layer, view 3 looks up)
    assert np.all(gK <= tol) and np.all(gC <= tol), (gK.max(), gC.max(), tol)
    # the surface row: the down-looking views reach the ground and read the line's transmittance there (eps = 1); the up-looking one does not
    iv = np.arange(npix)//(sc.nxr*sc.nyr)
    trans = 1.0-K_ref[:, :nz].sum(axis=1)
    down = iv < 2
    assert np.all(K_ref[down, nz] > 0.01) and np.allclose(K_ref[down, nz], trans[down], rtol=1.0e-12, atol=0.0)
    assert np.all(np.abs(K[down, nz]-trans[down]) <= tol) and np.all(K[~down, nz] == 0.0)


# ---- 3: opaque, isothermal -----------------------------------------------------------------------------------------------------------------------

def test_opaque_isothermal_scene(solver):
    """no line of sight escapes an isothermal scene under an opaque layer over a black surface: sum_k K = 1 within 1e-6, and C / K = B(T) to
    float32 in every row with K > 0 -- a term of C is fl(fl(w B) em), 2 roundings, one of K fl(w em), 1, either read-out rounds once and B
    itself once: 6 x 2^-24.  Seen from above the opaque layer, nothing below it contributes"""
    T = 285.0
    B = planck(vref.WL, T)
    above = [(180.0, 0.0, 1.0e6), (140.0, 70.0, 1.0e6), (30.0, 200.0, 150.0)]      # both down-looking views from above the top
    for views in (vref.VIEWS, above):
        sc = _on(vref.opaque_scene(views=views, T=T))
        npix, nz = sc.nview*sc.nxr*sc.nyr, sc.nz
        N = 20*npix
        solver.load_scene(sc); solver.reset(); solver.run(N, seed=71)
        assert solver.kernel_name() == NAME
        p = solver.view_profiles(N)
        K, C = p['weight'].astype(np.float64), p['contribution'].astype(np.float64)
        print('opaque: largest |sum K - 1| %.3e (allowed 1e-6); largest |C / (K B) - 1| %.3e (allowed %.3e)'
              % (np.abs(K.sum(axis=-1)-1.0).max(), np.abs(C[K > 0.0]/(K[K > 0.0]*B)-1.0).max(), 6.0*U24))
        assert np.all(np.abs(K.sum(axis=-1)-1.0) <= 1.0e-6)
        assert np.all((C > 0.0) == (K > 0.0)) and np.allclose(C[K > 0.0], K[K > 0.0]*B, rtol=6.0*U24, atol=0.0)
        assert np.all(K[0, :, :, nz-1] > 0.99) and np.all(K[0, :, :, :nz-1] == 0.0) and np.all(K[0, :, :, nz] == 0.0)      # nadir from above
        if views is above:
            assert np.all(K[1, :, :, nz-1] > 0.99) and np.all(K[1, :, :, :nz-1] == 0.0) and np.all(K[1, :, :, nz] == 0.0)
        else:                                                 # (its plane lies below the opaque layer: it sees the thin air and the black ground)
            assert np.all(K[1, :, :, nz-1] == 0.0) and np.all(K[1, :, :, nz] > 0.5)
        assert np.all(K[2, :, :, nz] == 0.0) and np.all(K[2, :, :, nz-1] > 0.5)                                       # up-looking


# ---- 4: K against the plain route by finite differences ------------------------------------------------------------------------------------------

def test_weights_are_the_plain_routes_temperature_jacobian(solver):
    """paths and weights do not depend on any temperature: with the same seed and ids, warming one 3-D layer uniformly, or the whole 2-D
    surface, changes the plain route's radiance by Src_flx K[p][k] (B' - B) -- within 1e-6 rad[p]: float32 rounding of the terms and of the
    read-outs, 2^-23 each"""
    base = vref.scattering_scene()
    jsfc = np.ones((2, 3), dtype=np.float32)
    psfc = np.zeros((5, 2, 3), dtype=np.float32); psfc[0] = 0.1
    base = dataclasses.replace(base, src_flx=1.5, jsfc=jsfc, psfc=psfc, tmps2d=np.zeros((2, 3), dtype=np.float32),
                               tmpa3d=np.zeros((base.nz3, base.ny, base.nx), dtype=np.float32))
    npix, nz = base.nview*base.nxr*base.nyr, base.nz
    N, seed, off = 300*npix+5, 113, 77
    solver.load_scene(_on(base)); solver.reset(); solver.run(N, seed=seed, offset=off)
    assert solver.kernel_name() == NAME
    K = solver.view_profiles(N)['weight'].astype(np.float64)

    def plain(sc):
        solver.load_scene(sc); solver.reset(); solver.run(N, seed=seed, offset=off)
        assert solver.kernel_name() == PLAIN, solver.kernel_name()
        return solver.radiance(N).astype(np.float64)
    rad = plain(base)
    t = np.asarray(base.tmp1d, dtype=np.float64)
    k3 = 2
    k = base.iz3l-1+k3
    ta = base.tmpa3d.copy(); ta[k3] += 5.0
    tl = 0.5*(t[k]+t[k+1])
    cases = [('layer %d' % k, dataclasses.replace(base, tmpa3d=ta), k, planck(vref.WL, tl+5.0)-planck(vref.WL, tl)),
             ('surface', dataclasses.replace(base, tmps2d=base.tmps2d+3.0), nz, planck(vref.WL, t[0]+3.0)-planck(vref.WL, t[0]))]
    for what, sc, row, dB in cases:
        diff = plain(sc)-rad
        want = 1.5*K[..., row]*dB
        gap = np.abs(diff-want)/rad
        print('Jacobian, %s: largest K %.4f, largest change %.3e of rad; |change - Src_flx K dB| / rad: %.3e (allowed 1e-6)'
              % (what, K[..., row].max(), (diff/rad).max(), gap.max()))
        assert K[..., row].max() > 0.05 and (diff/rad).max() > 1.0e-3
        assert np.all(gap <= 1.0e-6), (what, gap.max())


# ---- 5: hand-out and launch invariance -----------------------------------------------------------------------------------------------------------

def test_same_ids_same_tallies_whatever_the_hand_out_and_ranges_add(solver):
    sc = vref.absorbing_scene(albedo=0.3)
    npix = sc.nview*sc.nxr*sc.nyr
    N, off = 23*npix+211, 1000                                  # (N is no multiple of npix, the ids do not start at a pixel 0)
    rad0, none, name = _raw(solver, sc, [(off, N)], seed=79)
    assert name == PLAIN and none is None and rad0.min() > 0.0
    first = None
    for chunk, lg in ((0, 30), (1, 30), (4, 30), (-1, 30), (4, 12), (0, 12), (-1, 12)):
        rad, P, name = _raw(solver, _on(sc), [(off, N)], seed=79, chunk=chunk, lg=lg)
        assert name == NAME, name
        if chunk >= 0:
            assert solver.lib.mi3d_debug_backward_chunk(solver._h) == chunk
        assert np.allclose(rad, rad0, rtol=1.0e-12, atol=0.0), (chunk, lg)
        if first is None:
            first = P
            assert P[:, :, 0].sum(axis=1).min() > 0.0
        assert np.allclose(P, first, rtol=1.0e-12, atol=0.0), (chunk, lg, np.abs(P-first).max())
    for chunk in (-1, 0):
        rad, P, name = _raw(solver, _on(sc), [(off, N//2), (off+N//2, N-N//2)], seed=79, chunk=chunk)
        assert name == NAME and np.allclose(rad, rad0, rtol=1.0e-12, atol=0.0) and np.allclose(P, first, rtol=1.0e-12, atol=0.0), chunk


# ---- 6: the switch and the refusals --------------------------------------------------------------------------------------------------------------

def test_switch_and_refusals(solver):
    from er3t_amd.solver import Mi3dSolver
    lib = solver.lib
    err = lambda: lib.mi3d_last_error().decode()
    sc = vref.absorbing_scene()
    npix, nz = sc.nview*sc.nxr*sc.nyr, sc.nz
    k = np.zeros((npix, nz+1), dtype=np.float32)
    ptr = k.ctypes.data_as(lib.mi3d_get_view_profiles.argtypes[2])
    # off by default: a new handle runs the plain build and has nothing to read
    fresh = Mi3dSolver(device=0)
    try:
        fresh.load_scene(sc); fresh.reset(); fresh.run(2000, seed=5)
        assert fresh.kernel_name() == PLAIN
        assert lib.mi3d_get_view_profiles(fresh._h, 2000, ptr, None) == -2 and 'mi3d_set_view_profiles' in err()
    finally:
        fresh.close()
    assert lib.mi3d_set_view_profiles(solver._h, 2) == -1 and lib.mi3d_set_view_profiles(solver._h, -1) == -1
    # on, and the route not selected: the forward method, cameras, the cameras' backward method, emission weights
    cams = dataclasses.replace(sc, view_method=0, rad_kind=1, view_the=[180.0], view_phi=[0.0], view_zloc=[500.0], nxr=2, nyr=2, cam_images=0)
    for s, vm, cm, wg in ((dataclasses.replace(sc, view_method=0), 0, 0, 0), (cams, 1, 0, 0), (cams, 0, 1, 0), (cams, 0, 1, 1), (sc, 1, 0, 1)):
        solver.load_scene(s)
        solver.set_view_method(vm); solver.set_camera_method(cm); solver.set_emission_weights(wg); solver.set_view_profiles(1)
        rc = lib.mi3d_run(solver._h, 1000, 1, 0)
        msg = err()
        solver.set_view_profiles(0); solver.set_emission_weights(0); solver.set_camera_method(0); solver.set_view_method(0)
        assert rc == -4 and 'mi3d_set_view_profiles' in msg, (vm, cm, wg, rc, msg)
    # get before a run
    solver.load_scene(_on(sc))
    assert lib.mi3d_get_view_profiles(solver._h, 1000, ptr, None) == -2 and 'nothing has been tallied' in err()
    solver.reset(); solver.run(4*npix, seed=9)
    assert solver.kernel_name() == NAME
    p = solver.view_profiles(4*npix)
    assert p['weight'].sum() > 0.0
    only_c = np.zeros_like(k)
    assert lib.mi3d_get_view_profiles(solver._h, 4*npix, None, only_c.ctypes.data_as(lib.mi3d_get_view_profiles.argtypes[3])) == 0
    assert np.array_equal(only_c.reshape(p['contribution'].shape), p['contribution'])
    # mi3d_reset zeroes the tally; off and on again gives a zero tally that must be run into before it is read
    solver.reset()
    assert solver.view_profiles(4*npix)['weight'].max() == 0.0
    solver.run(4*npix, seed=9)
    solver.set_view_profiles(0); solver.set_view_profiles(1)
    assert lib.mi3d_get_view_profiles(solver._h, 1000, ptr, None) == -2
    solver.run(npix, seed=10)                                   # (no reset: the tally is new, not what the run before left)
    q = solver.view_profiles(npix)
    solver.reset(); solver.run(npix, seed=10)
    assert q['weight'].sum() > 0.0 and np.array_equal(q['weight'], solver.view_profiles(npix)['weight'])
    # mi3d_debug_backward_views ignores the switch
    st, d, score, capped = solver.debug_backward_views(9, 0, 64)
    solver.set_view_profiles(0)
    st0, d0, score0, _ = solver.debug_backward_views(9, 0, 64)
    assert np.array_equal(st, st0) and np.array_equal(d, d0) and np.array_equal(score, score0)
    # the refusals of the route read as before with the switch on
    lsrt = dataclasses.replace(sc, sfc_mtype=4, sfc_param=np.array([0.1, 0.05, 0.02, 0, 0], dtype=np.float32))
    cases = [(dataclasses.replace(sc, src_mtype=1, view_method=0), 'solar'),
             (dataclasses.replace(sc, src_mtype=2, src_fsol=5.0, src_the=150.0, view_method=0), 'solar+thermal'),
             (dataclasses.replace(sc, target=TARGET_FLUX), 'flux'), (dataclasses.replace(sc, solver=1), 'partial 3-D'),
             (dataclasses.replace(sc, solver=2), 'independent columns'), (lsrt, 'Lambertian')]
    for s, word in cases:
        msgs = []
        for on in (0, 1):
            try:
                solver.load_scene(s)
            except OSError:
                pass                                             # (mi3d_prepare refuses the LSRT surface of a thermal job already)
            solver.set_view_method('backward'); solver.set_view_profiles(on)
            rc = lib.mi3d_run(solver._h, 1000, 1, 0)
            msgs.append((rc, err()))
            solver.set_view_profiles(0)
        assert msgs[0][0] == -4 and word in msgs[0][1] and msgs[0] == msgs[1], (word, msgs)
    solver.load_scene(_on(dataclasses.replace(sc, view_zloc=[1.0e6, 0.0, 150.0])))
    assert lib.mi3d_run(solver._h, 1000, 1, 0) == -1 and 'surface' in err()
    solver.load_scene(_on(dataclasses.replace(sc, view_the=[], view_phi=[], view_zloc=[])))
    assert lib.mi3d_run(solver._h, 1000, 1, 0) == -2 and 'no view' in err()


# ---- 7: two ranks --------------------------------------------------------------------------------------------------------------------------------

def test_two_ranks_match_one(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on the one GPU) against one rank on the same ids (tests/view_profiles_dist_worker.py):
    the shards of [0, N) add to the job's raw tallies, and the read-out divides by the job's counts.  The same histories; the float64 sums
    of a row differ in their order (1e-16 relative), either value is rounded to float32 once: at most 2^-23 relative"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'view_profiles_dist_worker.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(str(tmp_path), 'result.npz'))
    assert str(z['kernel']) == NAME and int(z['capped']) == 0
    ulp = 2.0**-23
    for v in ('rad', 'weight', 'contribution'):
        a, b = z['dist_'+v].astype(np.float64), z['solo_'+v].astype(np.float64)
        print('two ranks against one, %s: largest relative gap %.3e (allowed %.3e)' % (v, np.abs(a[b > 0.0]/b[b > 0.0]-1.0).max(), ulp))
        assert a.shape == b.shape and b.max() > 0.0 and np.all(np.abs(a-b) <= ulp*np.maximum(a, b)), v
    assert z['dist_weight'].shape == (2, 10, 12, int(z['nz'])+1)


# ---- 8: the drop-in ------------------------------------------------------------------------------------------------------------------------------

def test_dropin_files_against_fused(tmp_path):
    """mcarats_ng(source='thermal', view_method='backward', view_profiles=True) with two views through the file route and the fused one under
    the same seeds: mca_out_ng's keys and shapes, view_contribution.sum(-1) = rad to float32, and files against fused as the radiance of
    test_gpu_backward_views.py: rad and bt bit for bit.  The profiles are the same float32 job arrays reduced by the same reducer on either
    route (read from .prf.bin or taken as the job ends): bit for bit too"""
    import contextlib
    import io
    import er3t_amd.rtm.mca as mca
    from er3t_amd.rtm.mca.mca_exe import get_runner, profiles_fname
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from tests.golden import inputs as gin
    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=3)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=str(tmp_path/'atm3d.bin'), quiet=True)
        kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=3, target='radiance', surface_albedo=0.05, source='thermal', view_method='backward',
                  view_profiles=True, Nrun=3, photons=6e4, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True,
                  date=gin.DATE, quiet=True, sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
        np.random.seed(7)                                    # (mcarats_ng shuffles the seeds over its jobs)
        files = mca.mcarats_ng(fdir=str(tmp_path/'files'), **kw)
        np.random.seed(7)
        fused = mca.mcarats_ng(fdir=str(tmp_path/'fused'), abs_obj=ab, keep_files=False, **kw)
    sol = get_runner().sol
    assert sol.kernel_name() == NAME and sol.debug_backward_views(1, 0, 0)[3] == 0
    assert fused.fused is not None and 'prf' in fused.fused and files.fused is None
    nml = mca.mca_inp_read(files.fnames_inp[0][0])
    nz = int(nml['Atm_nz'])
    assert nml['Rad_mvprf'] == 1 and nml['Rad_mvbwd'] == 1
    for f in sum(files.fnames_out, []):
        assert os.path.getsize(profiles_fname(f)) == 4*2*(2*10*12)*(nz+1)
    for mode in ('mean', 'all'):
        a = mca.mca_out_ng(mca_obj=fused, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        b = mca.mca_out_ng(mca_obj=files, abs_obj=ab, mode=mode, squeeze=True, quiet=True).data
        keys = ['view_weight', 'view_contribution', 'view_layer_planck']+(['view_weight_std', 'view_contribution_std'] if mode == 'mean' else [])
        assert sorted(a.keys()) == sorted(b.keys()) and all(k in a for k in keys)
        for k in ('rad', 'bt'):
            assert np.array_equal(a[k]['data'], b[k]['data']), (mode, k)
        tail = (nz+1,)+((3,) if mode == 'all' else ())
        for k in keys:
            assert a[k]['data'].shape == b[k]['data'].shape == (12, 10, 2)+tail, (mode, k, a[k]['data'].shape)
            assert a[k]['dims_info'] == ['Nxr', 'Nyr', 'Nview', 'Nz+1']+(['Nr'] if mode == 'all' else [])
            assert np.array_equal(a[k]['data'], b[k]['data'], equal_nan=True), (mode, k)
        # the partition after the g / run reduction, in roundings of 2^-24 (all terms positive): a job's rad 1 and its rows of C 1; rad's run
        # sum is formed in float32 over Ng = 3 jobs, a product and an addition each: 6; its mean over 3 runs in float32: 3; the float64
        # reduction of C is rounded once at the end: 1 -- 12 in all
        rad = b['rad']['data'].astype(np.float64)
        tot = b['view_contribution']['data'].astype(np.float64).sum(axis=3)
        print('drop-in (%s): largest |sum C / rad - 1| %.3e (allowed %.3e)' % (mode, np.abs(tot/rad-1.0).max(), 12.0*U24))
        assert rad.min() > 0.0 and np.allclose(tot, rad, rtol=12.0*U24, atol=0.0), mode
        kk, cc, bb = b['view_weight']['data'], b['view_contribution']['data'], b['view_layer_planck']['data']
        assert np.array_equal(np.isnan(bb), kk == 0.0) and np.all(kk >= 0.0) and (kk > 0.0).mean() > 0.5
    lp = b['view_layer_planck']['data']
    assert np.nanmin(lp) > planck(11.0, 180.0) and np.nanmax(lp) < planck(11.0, 330.0)
