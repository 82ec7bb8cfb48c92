"""
Thermal source (Src_mtype = 3): photons per second of the general photon loop on the synthetic cloud scenes of BASELINE
configs 2 (128 x 128 x 50) and 4 (480 x 480 x 100), nadir radiance, flux and net heating rates under both estimators (legs
'heat': collision, 'heat_path': path length; float64 atomics into the heating cells), and what building the source costs per job
(k_thermal_power + the prefix scan + reading P_tot back: the wall time of mi3d_prepare after mi3d_set_thermal).

Leg 'mix': the solar+thermal source (Src_mtype = 2) at 3.75 um, nadir radiance, sun at 40 degrees, Src_fsol = 10 W m-2 um-1; its row
carries the solar share p = P_sol / (P_tot + P_sol).  Legs 'mix_thermal' and 'mix_solar' are its two halves as jobs of their own on
the same scene -- the thermal job at 3.75 um, and the solar job sent to the general loop (set_kernel(general=True)) --: with their
times per photon t_thermal and t_solar a mixed photon should cost p t_solar + (1 - p) t_thermal.

Leg 'cam' (DESIGN.md 5.10): sixteen up-looking irradiance sensors on the ground, a 4 x 4 grid, three rows: cam_images = 2 through the
event lists and the ray kernel, and cam_images = 0 on that route and on the general loop with the rays in the photons' lanes -- the one
like-for-like comparison of the two.  Its rows carry the mean reading of the sixteen sensors.

    python tools/thermal_rate.py [--photons 5e7] [--reps 3] [--legs radiance,flux,heat,heat_path]
    python tools/thermal_rate.py --legs mix,mix_thermal,mix_solar
    python tools/thermal_rate.py --legs cam --photons 1e7

Leg 'bwd' (DESIGN.md 5.11): the same sixteen sensors by backward Monte Carlo (cam_method = 1) and, in the same session, by the forward
route with cam_images = 2: histories (photons) per second, the relative standard error of every sensor's reading over 16 batches (mean
and largest over the sensors) and the figure of merit 1 / (se^2 t), se the mean relative standard error of a sensor and t the kernel
time of the 16 batches.  --photons: photons per forward batch; --histories: histories per backward batch (a multiple of 16).

    python tools/thermal_rate.py --legs bwd --photons 1e7 --histories 1.6e6
Leg 'wgt' (DESIGN.md 5.12): the same sixteen sensors by backward Monte Carlo with the per-cell emission weights (cam_weights) off, then on:
histories per second and kernel time of both, their ratio, and the cell steps of a history from the counting build.
    python tools/thermal_rate.py --legs wgt --histories 1.6e6
Leg 'sat' (DESIGN.md 5.14): a satellite image with a nadir and a 45 degree view in one job, by the forward route and by backward Monte Carlo
(view_method = 1) under "bwd_chunk" 0 (the stride hand-out), 4, 8, 16, 32 and -1 (the default: chosen per launch): 16 batches each over
disjoint id ranges; histories (photons) per second, kernel time, the chunk the launches ran with, the relative standard error per pixel over
the batches (mean and largest over the pixels) and the figure of merit 1 / (se^2 t), se the mean relative standard error of a pixel.
--photons: photons per forward batch; --per-pixel: histories per pixel and backward batch (32: every chunk of the list is a launch of its own).
    python tools/thermal_rate.py --legs sat --photons 2e6 --per-pixel 32
Leg 'prf' (DESIGN.md 5.16): the image of the 'sat' leg by backward Monte Carlo under the default hand-out with the per-layer view profiles
(view_profiles) off, then on, at 8 and at 32 histories per pixel and launch: 16 batches each over disjoint id ranges, three times; histories
per second and kernel time.  Under MI3D_LIBRARY (an older build of the library) the rows with the profiles off alone.
    python tools/thermal_rate.py --legs prf
Leg 'err' (DESIGN.md 5.17): the plain backward builds with the per-pixel standard errors (pixel_errors) off, then on -- the image of the 'sat'
leg at 8 and at 32 histories per pixel and launch under the default hand-out and under the plain stride ("bwd_chunk" 0: two atomics a
history), the sixteen sensors of the 'bwd' leg (both sums per workgroup in LDS) and one all-sky camera of 64 x 64 pixels on the ground
(4096 pixels: two global atomics a history): 16 batches each over disjoint id ranges, three times; histories per second, kernel time and,
with the switch on, the mean relative standard error of a pixel from the histories of the last batch.  Under MI3D_LIBRARY (an older build
of the library) the rows with the switch off alone.
    python tools/thermal_rate.py --legs err
Leg 'sun' (DESIGN.md 5.18): the image of the 'sat' leg (a nadir and a 45 degree view) of the solar+thermal job at 3.75 um, the sun 40 degrees
from the zenith, Src_fsol = 10 W m-2 um-1, by the forward mixed route, by backward Monte Carlo with the sunlight term (view_sunlight = 1) and,
for what the sun rays cost a history, by the backward thermal route of the same scene (Src_mtype = 3): 16 batches each over disjoint id
ranges; histories (photons) per second, kernel time, relative standard error per pixel (mean, largest), merit 1 / (se^2 t), the image means,
and from the counting build the cell steps per history of both backward jobs: their difference is the sun rays'.
    python tools/thermal_rate.py --legs sun --photons 2e6 --per-pixel 32
Leg 'col' (DESIGN.md 5.20): the image of the 'sat' leg (a nadir and a 45 degree view) of the thermal job under independent columns, by the
forward route (solver 2), by backward Monte Carlo with the column histories (solver 2, view_columns = 1) and, for the rate of the build, by
backward Monte Carlo under the 3-D solver: at 8 and at 32 histories per pixel and launch, the three jobs in turn, `--reps` times; 16 batches
each over disjoint id ranges; histories (photons) per second, kernel time, relative standard error per pixel (mean, largest), merit
1 / (se^2 t), the image means and, from the counting build, the cell steps per history of the backward jobs.
    python tools/thermal_rate.py --legs col --photons 2e6
"""

import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from er3t_amd.scene import TARGET_FLUX, TARGET_RADIANCE, TARGET_HEAT      # noqa: E402
from er3t_amd.solver import Mi3dSolver                        # noqa: E402
from er3t_amd.synth import les_scene, z_levels_config4, atm_synth   # noqa: E402


def thermal(scene, levels, wl=11.0):
    atm = atm_synth(levels)
    omgp = np.where(scene.extp > 0.0, np.float32(0.95), np.float32(1.0)).astype(np.float32)   # a cloud that absorbs at 11 um
    return dataclasses.replace(scene, src_mtype=3, src_wlen=wl, tmp1d=atm.lev['temperature']['data'], omgp=omgp)


def pyrgeometers(scene, images, n=4, z=1.0):
    """n x n up-looking irradiance sensors z metres above the ground (cameras with the rectangular map, one pixel over the hemisphere)"""
    g = (np.arange(n)+0.5)/n
    xp, yp = [list(v.ravel()) for v in np.meshgrid(g, g)]
    m = n*n
    return dataclasses.replace(scene, target=TARGET_RADIANCE, rad_kind=1, view_the=[0.0]*m, view_phi=[0.0]*m, view_zloc=[z]*m, cam_xpos=xp,
                               cam_ypos=yp, cam_psi=[0.0]*m, cam_qmax=[180.0]*m, cam_umax=[90.0]*m, cam_vmax=[180.0]*m, cam_apsize=[0.05]*m,
                               nxr=1, nyr=1, cam_mpmap=2, cam_mrproj=1, cam_images=images)


def merit_rows(sol, name, s, n_fwd, n_bwd, nb=16):
    """the 'bwd' leg: the sensors of scene s by the backward and by the forward route, nb batches each over disjoint id ranges"""
    rows = []
    for target, method, n in (('bwd', 1, n_bwd), ('bwd_forward', 0, n_fwd)):
        sc = dataclasses.replace(s, cam_method=method)
        sol.load_scene(sc)
        sol.reset(); sol.run(min(n, 2000000), seed=1); sol.sync()        # warm-up
        vals, ms_all = [], 0.0
        for b in range(nb):
            sol.reset()
            sol.run(n, seed=2, offset=b*n)
            vals.append(np.pi*sol.radiance(n).astype(np.float64).ravel())
            ms_all += sol.timing()[0]
        v = np.array(vals)
        mean, se = v.mean(axis=0), v.std(axis=0, ddof=1)/np.sqrt(nb)
        rel = se/mean
        t = ms_all*1e-3
        row = dict(scene=name, target=target, kernel=sol.kernel_name(), histories_per_batch=n, batches=nb, histories_per_s=float(nb*n/t),
                   kernel_s=float(t), f_down_sensor_mean=float(mean.mean()), rel_se_mean=float(rel.mean()), rel_se_max=float(rel.max()),
                   merit=float(1.0/(rel.mean()**2*t)))
        if method == 1:
            row['capped'] = sol.debug_backward(2, 0, 0)[2]
        else:
            row['cam_images'] = sc.cam_images
        rows.append(row)
        print(json.dumps(row), flush=True)
    sol.set_camera_method('forward')
    return rows


def sat_rows(sol, name, s, n_fwd, per_pixel, chunks=(0, 4, 8, 16, 32, -1), nb=16):
    """the 'sat' leg: the image of scene s (a nadir and a 45 degree view in one job) by the forward route and by the backward route under
    every hand-out of `chunks`, nb batches each over disjoint id ranges"""
    s = dataclasses.replace(s, view_the=[180.0, 135.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6], nxr=s.nx, nyr=s.ny)
    npix = 2*s.nx*s.ny
    rows = []
    try:
        for method, chunk, n in [(0, None, n_fwd)]+[(1, c, per_pixel*npix) for c in chunks]:
            if chunk is not None:
                sol.set_tuning(bwd_chunk=chunk)
            sol.load_scene(dataclasses.replace(s, view_method=method))
            sol.reset(); sol.run(min(n, 2000000), seed=1); sol.sync()        # warm-up
            tot, sq, ms_all = np.zeros((2, s.ny, s.nx)), np.zeros((2, s.ny, s.nx)), 0.0
            for b in range(nb):
                sol.reset()
                sol.run(n, seed=2, offset=b*n)
                r = sol.radiance(n).astype(np.float64)
                tot += r; sq += r*r
                ms_all += sol.timing()[0]
            mean = tot/nb
            se = np.sqrt(np.maximum(sq/nb-mean*mean, 0.0)/(nb-1))
            ok = mean > 0.0
            rel = se[ok]/mean[ok]
            t = ms_all*1e-3
            row = dict(scene=name, target='sat_backward' if method else 'sat_forward', kernel=sol.kernel_name(), histories_per_batch=n, batches=nb,
                       histories_per_s=float(nb*n/t), kernel_s=float(t), image_mean=[float(m.mean()) for m in mean], pixels_without_a_score=int((~ok).sum()),
                       rel_se_mean=float(rel.mean()), rel_se_max=float(rel.max()), merit=float(1.0/(rel.mean()**2*t)))
            if method:
                row.update(bwd_chunk=chunk, chunk_launched=sol.lib.mi3d_debug_backward_chunk(sol._h), capped=sol.debug_backward_views(2, 0, 0)[3])
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        sol.set_tuning(bwd_chunk=-1)
        sol.set_view_method('forward')
    return rows


def sun_rows(sol, name, s, n_fwd, per_pixel, nb=16):
    """the 'sun' leg: scene s, a solar+thermal job, by the forward mixed route, by the backward route with the sunlight term,
    and its thermal half by the backward route; nb batches each over disjoint id ranges"""
    s = dataclasses.replace(s, view_the=[180.0, 135.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6], nxr=s.nx, nyr=s.ny)
    npix = 2*s.nx*s.ny
    rows = []
    jobs = [('sun_forward', dataclasses.replace(s, view_method=0), n_fwd),
            ('sun_backward', dataclasses.replace(s, view_method=1, view_sunlight=1), per_pixel*npix),
            ('sun_backward_thermal', dataclasses.replace(s, src_mtype=3, src_fsol=None, view_method=1), per_pixel*npix)]
    try:
        for target, sc, n in jobs:
            sol.load_scene(sc)
            sol.reset(); sol.run(min(n, 2000000), seed=1); sol.sync()        # warm-up
            tot, sq, ms_all = np.zeros((2, s.ny, s.nx)), np.zeros((2, s.ny, s.nx)), 0.0
            for b in range(nb):
                sol.reset()
                sol.run(n, seed=2, offset=b*n)
                r = sol.radiance(n).astype(np.float64)
                tot += r; sq += r*r
                ms_all += sol.timing()[0]
            mean = tot/nb
            se = np.sqrt(np.maximum(sq/nb-mean*mean, 0.0)/(nb-1))
            ok = mean > 0.0
            rel = se[ok]/mean[ok]
            t = ms_all*1e-3
            row = dict(scene=name, target=target, kernel=sol.kernel_name(), histories_per_batch=n, batches=nb, histories_per_s=float(nb*n/t),
                       kernel_s=float(t), image_mean=[float(m.mean()) for m in mean], image_mean_se=[float(np.sqrt((e**2).sum())/e.size) for e in se],
                       pixels_without_a_score=int((~ok).sum()), rel_se_mean=float(rel.mean()), rel_se_max=float(rel.max()),
                       merit=float(1.0/(rel.mean()**2*t)))
            if sc.view_method:
                sol.set_counting(True)
                sol.reset(); sol.run(n, seed=2); sol.sync()
                c = sol.counters()
                sol.set_counting(False)
                row.update(chunk_launched=sol.lib.mi3d_debug_backward_chunk(sol._h), capped=sol.debug_backward_views(2, 0, 0)[3],
                           steps_per_history=c['steps']/n, steps3d_per_history=c['steps3d']/n, events_per_history=(c['scatter']+c['surface'])/n)
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        sol.set_counting(False)
        sol.set_view_sunlight(False)
        sol.set_view_method('forward')
    return rows


def col_rows(sol, name, s, n_fwd, per_pixels=(8, 32), nb=16, reps=3):
    """the 'col' leg: scene s, a thermal job, under independent columns by the forward route and by the backward route with the
    column histories, and under the 3-D solver by the backward route; the three in turn, `reps` times at every number of histories per pixel
    and launch of `per_pixels`; nb batches each over disjoint id ranges"""
    s = dataclasses.replace(s, view_the=[180.0, 135.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6], nxr=s.nx, nyr=s.ny)
    npix = 2*s.nx*s.ny
    rows = []
    try:
        for pp in per_pixels:
            jobs = [('col_forward_ipa', dataclasses.replace(s, solver=2, view_method=0), n_fwd),
                    ('col_backward_ipa', dataclasses.replace(s, solver=2, view_method=1, view_columns=1), pp*npix),
                    ('col_backward_3d', dataclasses.replace(s, solver=0, view_method=1), pp*npix)]
            for rep in range(reps):
                for target, sc, n in jobs:
                    sol.load_scene(sc)
                    sol.reset(); sol.run(min(n, 2000000), seed=1); sol.sync()        # warm-up
                    tot, sq, ms_all = np.zeros((2, s.ny, s.nx)), np.zeros((2, s.ny, s.nx)), 0.0
                    for b in range(nb):
                        sol.reset()
                        sol.run(n, seed=2, offset=b*n)
                        r = sol.radiance(n).astype(np.float64)
                        tot += r; sq += r*r
                        ms_all += sol.timing()[0]
                    mean = tot/nb
                    se = np.sqrt(np.maximum(sq/nb-mean*mean, 0.0)/(nb-1))
                    ok = mean > 0.0
                    rel = se[ok]/mean[ok]
                    t = ms_all*1e-3
                    row = dict(scene=name, target=target, kernel=sol.kernel_name(), per_pixel=pp, rep=rep, histories_per_batch=n, batches=nb,
                               histories_per_s=float(nb*n/t), kernel_s=float(t), image_mean=[float(m.mean()) for m in mean],
                               image_mean_se=[float(np.sqrt((e**2).sum())/e.size) for e in se], pixels_without_a_score=int((~ok).sum()),
                               rel_se_mean=float(rel.mean()), rel_se_max=float(rel.max()), merit=float(1.0/(rel.mean()**2*t)))
                    if sc.view_method and rep == 0:
                        sol.set_counting(True)
                        sol.reset(); sol.run(n, seed=2); sol.sync()
                        c = sol.counters()
                        sol.set_counting(False)
                        row.update(chunk_launched=sol.lib.mi3d_debug_backward_chunk(sol._h), capped=sol.debug_backward_views(2, 0, 0)[3],
                                   steps_per_history=c['steps']/n, steps3d_per_history=c['steps3d']/n, events_per_history=(c['scatter']+c['surface'])/n)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    finally:
        sol.set_counting(False)
        sol.set_view_columns(False)
        sol.set_view_method('forward')
    return rows


def profiles_rows(sol, name, s, per_pixels=(8, 32), nb=16, reps=3):
    """the 'prf' leg: the image of the 'sat' leg by the backward route under the default hand-out with the view profiles off,
    then on, at every number of histories per pixel and launch of `per_pixels`; nb batches over disjoint id ranges, `reps` times each.  An
    older build of the library (MI3D_LIBRARY) gives the 'off' rows alone"""
    s = dataclasses.replace(s, view_the=[180.0, 135.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6], nxr=s.nx, nyr=s.ny, view_method=1)
    npix = 2*s.nx*s.ny
    rows = []
    have = not getattr(sol.lib.mi3d_set_view_profiles, 'stale', False)
    try:
        for pp in per_pixels:
            n = pp*npix
            for on in ((0, 1) if have else (0,)):
                sol.load_scene(dataclasses.replace(s, view_profiles=on))
                sol.reset(); sol.run(n, seed=1); sol.sync()                  # warm-up
                for rep in range(reps):
                    ms_all, mean = 0.0, 0.0
                    for b in range(nb):
                        sol.reset()
                        sol.run(n, seed=2, offset=b*n)
                        sol.sync()
                        ms_all += sol.timing()[0]
                        mean += float(sol.radiance(n).mean())/nb
                    t = ms_all*1e-3
                    row = dict(scene=name, target='sat_profiles' if on else 'sat_backward', kernel=sol.kernel_name(), per_pixel=pp, histories_per_batch=n,
                               batches=nb, rep=rep, histories_per_s=float(nb*n/t), kernel_s=float(t), image_mean=mean,
                               chunk_launched=sol.lib.mi3d_debug_backward_chunk(sol._h), capped=sol.debug_backward_views(2, 0, 0)[3])
                    if on:
                        c = sol.view_profiles(n)['contribution'].astype(np.float64).sum(axis=-1)
                        row.update(sum_contribution_mean=float(c.mean()))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    finally:
        if have:
            sol.set_view_profiles(False)
        sol.set_view_method('forward')
    return rows


def errors_rows(sol, name, s, n_cam, per_pixels=(8, 32), nb=16, reps=3):
    """the 'err' leg: the plain backward builds with the per-pixel standard errors off, then on; nb batches over disjoint id
    ranges, `reps` times each.  An older build of the library (MI3D_LIBRARY) gives the 'off' rows alone"""
    sat = dataclasses.replace(s, view_the=[180.0, 135.0], view_phi=[0.0, 0.0], view_zloc=[1.0e6, 1.0e6], nxr=s.nx, nyr=s.ny, view_method=1)
    sky = dataclasses.replace(pyrgeometers(s, -1, n=1), nxr=64, nyr=64, cam_mpmap=1, cam_mrproj=0, cam_umax=[90.0], cam_vmax=[90.0], cam_qmax=[90.0],
                              cam_method=1)
    jobs = [('sat', sat, pp*2*s.nx*s.ny, chunk, dict(per_pixel=pp, bwd_chunk=chunk)) for pp in per_pixels for chunk in (-1, 0)]
    jobs += [('bwd', dataclasses.replace(pyrgeometers(s, -1), cam_method=1), n_cam, -1, dict(pixels=16)), ('sky', sky, n_cam, -1, dict(pixels=4096))]
    rows = []
    have = not getattr(sol.lib.mi3d_set_pixel_errors, 'stale', False)
    try:
        for tag, sc, n, chunk, extra in jobs:
            sol.set_tuning(bwd_chunk=chunk)
            for on in ((0, 1) if have else (0,)):
                sol.load_scene(dataclasses.replace(sc, pixel_errors=on))
                sol.reset(); sol.run(n, seed=1); sol.sync()                  # warm-up
                for rep in range(reps):
                    ms_all, mean = 0.0, 0.0
                    for b in range(nb):
                        sol.reset()
                        sol.run(n, seed=2, offset=b*n)
                        sol.sync()
                        ms_all += sol.timing()[0]
                        mean += float(sol.radiance(n).mean())/nb
                    t = ms_all*1e-3
                    row = dict(scene=name, target='%s_errors' % tag if on else '%s_plain' % tag, kernel=sol.kernel_name(), histories_per_batch=n, batches=nb,
                               rep=rep, histories_per_s=float(nb*n/t), kernel_s=float(t), image_mean=mean, **extra)
                    if on:
                        r, se = sol.radiance(n).astype(np.float64), sol.radiance_se(n).astype(np.float64)
                        row.update(rel_se_mean=float((se[r > 0.0]/r[r > 0.0]).mean()))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    finally:
        sol.set_tuning(bwd_chunk=-1)
        if have:
            sol.set_pixel_errors(False)
        sol.set_view_method('forward')
        sol.set_camera_method('forward')
    return rows


def weights_rows(sol, name, s, n, nb=16):
    """the 'wgt' leg: the sensors of scene s by the backward route with the emission weights off, then on, nb batches each
    over the same id ranges; the counting build, once, for the absorbing cell steps of a history (one float64 atomic each with the switch on)"""
    rows, base = [], None
    for on in (0, 1):
        sol.load_scene(dataclasses.replace(s, cam_method=1, cam_weights=on))
        sol.reset(); sol.run(n, seed=1); sol.sync()                      # warm-up
        ms_all = 0.0
        for b in range(nb):
            sol.reset()
            sol.run(n, seed=2, offset=b*n)
            sol.sync()
            ms_all += sol.timing()[0]
        t = ms_all*1e-3
        row = dict(scene=name, target='wgt_on' if on else 'wgt_off', kernel=sol.kernel_name(), histories_per_batch=n, batches=nb,
                   histories_per_s=float(nb*n/t), kernel_s=float(t), capped=sol.debug_backward(2, 0, 0)[2])
        if on:
            k = sol.emission_weights(n)
            nz_steps = sum(int(np.count_nonzero(k[p])) for p in ('voxels', 'layers', 'surface'))
            row.update(npix=int(k['layers'].shape[0]), ncell=int(sum(k[p][0].size for p in ('voxels', 'layers', 'surface'))), cells_with_weight=nz_steps,
                       sum_of_weights_mean=float(sum(k[p].astype(np.float64).sum() for p in ('voxels', 'layers', 'surface'))/k['layers'].shape[0]),
                       lds_staged=int(sol.lib.mi3d_debug_weights_staged(sol._h)), slowdown=float(t/base))
            del k
        else:
            base = t
        rows.append(row)
        print(json.dumps(row), flush=True)
    sol.set_counting(True)
    try:
        sol.reset(); sol.run(n, seed=2); sol.sync()
        c = sol.counters()
        row = dict(scene=name, target='wgt_steps', kernel=sol.kernel_name(), histories=n, steps_per_history=c['steps']/n, steps3d_per_history=c['steps3d']/n,
                   cell_steps_per_s_switch_on=float(c['steps']/n*rows[1]['histories_per_s']))
        rows.append(row)
        print(json.dumps(row), flush=True)
    finally:
        sol.set_counting(False)
        sol.set_emission_weights(False)
        sol.set_camera_method('forward')
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--photons', type=float, default=5e7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--legs', default='radiance,flux,heat,heat_path')
    ap.add_argument('--histories', type=float, default=1.6e6)
    ap.add_argument('--per-pixel', type=int, default=32)
    ap.add_argument('--scenes', default='les128,les480')
    a = ap.parse_args()
    sol = Mi3dSolver(0)
    n = int(a.photons)
    rows = []
    for name, kw, levels in (('les128', dict(nx=128, ny=128, nz3=50), None),
                             ('les480', dict(nx=480, ny=480, nz3=100, levels=z_levels_config4(), z_top=1.6, seed=20251004), z_levels_config4())):
        from er3t_amd.synth import z_levels_config2
        lev = levels if levels is not None else z_levels_config2()
        if name not in a.scenes.split(','):
            continue
        legs = sum([['cam', 'cam0', 'cam0_general'] if t == 'cam' else [t] for t in a.legs.split(',')], [])
        for target in legs:
            general = False
            if target == 'bwd':
                sol.set_kernel(general=False)
                rows += merit_rows(sol, name, pyrgeometers(thermal(les_scene(target='radiance', **kw), lev), 2), n, int(a.histories)//16*16)
                continue
            if target == 'sat':
                sol.set_kernel(general=False)
                rows += sat_rows(sol, name, thermal(les_scene(target='radiance', **kw), lev), n, a.per_pixel)
                continue
            if target == 'sun':
                sol.set_kernel(general=False)
                s = thermal(les_scene(target='radiance', **kw), lev, wl=3.75)
                rows += sun_rows(sol, name, dataclasses.replace(s, src_mtype=2, src_fsol=10.0, src_the=140.0, src_phi=0.0), n, a.per_pixel)
                continue
            if target == 'col':
                sol.set_kernel(general=False)
                rows += col_rows(sol, name, thermal(les_scene(target='radiance', **kw), lev), n, reps=a.reps)
                continue
            if target == 'prf':
                sol.set_kernel(general=False)
                rows += profiles_rows(sol, name, thermal(les_scene(target='radiance', **kw), lev))
                continue
            if target == 'err':
                sol.set_kernel(general=False)
                rows += errors_rows(sol, name, thermal(les_scene(target='radiance', **kw), lev), int(a.histories)//16*16)
                continue
            if target == 'wgt':
                sol.set_kernel(general=False)
                rows += weights_rows(sol, name, pyrgeometers(thermal(les_scene(target='radiance', **kw), lev), 2), int(a.histories)//16*16)
                continue
            if target in ('cam', 'cam0', 'cam0_general'):
                s = pyrgeometers(thermal(les_scene(target='radiance', **kw), lev), 2 if target == 'cam' else 0)
                general = target == 'cam0_general'
            elif target in ('mix', 'mix_thermal', 'mix_solar'):
                s = thermal(les_scene(target='radiance', **kw), lev, wl=3.75)
                s = dataclasses.replace(s, src_the=140.0, src_phi=0.0)
                if target == 'mix':
                    s = dataclasses.replace(s, src_mtype=2, src_fsol=10.0)
                elif target == 'mix_solar':
                    s = dataclasses.replace(s, src_mtype=1)
                    general = True
            elif target in ('heat', 'heat_path'):            # net heating rates beside the fluxes (Flx_mhrt = 2), either estimator
                s = thermal(les_scene(target='flux', **kw), lev)
                s = dataclasses.replace(s, target=TARGET_FLUX | TARGET_HEAT, heat_estimator=int(target == 'heat_path'))
            else:
                s = thermal(les_scene(target=target, **kw), lev)
            sol.set_kernel(general=general)
            sol.load_scene(s)
            # the per-job cost of the source: set again (dirty), then prepare
            build = []
            for _ in range(a.reps):
                if s.src_mtype == 3:
                    sol.set_thermal(3, s.src_wlen, s.tmp1d, s.tmpa3d, s.tmps2d)
                elif s.src_mtype == 2:
                    sol.set_thermal(2, s.src_wlen, s.tmp1d, s.tmpa3d, s.tmps2d, fsol=s.src_fsol)
                t0 = time.perf_counter(); sol.prepare(); build.append((time.perf_counter()-t0)*1e3)
            sol.reset(); sol.run(min(n, 2000000), seed=1); sol.sync()        # warm-up
            rates = []
            for r in range(a.reps):
                sol.reset()
                sol.run(n, seed=2, offset=r*n)
                ms, _ = sol.timing()
                rates.append(n/(ms*1e-3))
            row = dict(scene=name, target=target, kernel=sol.kernel_name(), photons=n, photons_per_s=float(np.median(rates)),
                       photons_per_s_min=float(np.min(rates)), photons_per_s_max=float(np.max(rates)), thermal_build_ms=float(np.median(build)))
            if s.src_mtype == 2:
                ptot, psol = sol.source_power()
                row['solar_share'] = psol/(ptot+psol)
            if getattr(s, 'rad_kind', 2) == 1:
                row['cam_images'] = s.cam_images
                row['f_down_sensor_mean'] = float(np.pi*sol.radiance(n).astype(np.float64).mean())
            if s.target & TARGET_HEAT:                     # (read once: the emission is taken off on the device)
                h = sol.heating(n)
                row['net_heating_domain_mean'] = float(h.astype(np.float64).mean())
            rows.append(row)
            print(json.dumps(row), flush=True)
    sol.set_kernel(general=False)
    return rows


if __name__ == '__main__':
    main()
