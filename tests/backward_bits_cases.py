"""
The cases of tests/test_gpu_backward_bits.py, shared with tools/record_backward_golden.py, which records what a library computes for them.

Two scenes the suite already builds, each with a surface that reflects, so that a history scatters, reaches the surface and is turned there:

    cam_rect, cam_polar   scattering_slab(tables=True) of tests/test_gpu_backward.py (a tabulated and a Rayleigh constituent, Lambert surface
                          0.2) under two sensors inside it, one looking up and one down: rectangular map with cosine weighting (mpmap 2,
                          mrproj 1, one pixel each) and the polar camera (mpmap 1, 3 x 3 pixels each, lines outside the cone of view end at once)
    views                 the scattering checkerboard of tests/backward_views_ref.py over the 3 x 2 grey surface with temperature anomalies of
                          its absorbing scene; a nadir, an oblique and an up-looking view; an image of 3 x 2 pixels, so every tile of 8 x 8 is
                          clipped; the stride hand-out ("bwd_chunk" 0) and the tiles (16)

run_case records, for one case: the debug entry's outputs for the first N_DEBUG ids as raw bytes, the counters of a counting run over those
ids alone, and for N_RUN histories of the same seed and first id the raw float64 tallies of every production build that serves the scene.
"""

import dataclasses

import numpy as np

from er3t_amd.scene import TARGET_RADIANCE
from tests import backward_views_ref as vref
from tests.test_gpu_backward import cameras, scattering_slab

SEED, ID0 = 97, 5
N_DEBUG, N_RUN = 1024, 20000
COUNTERS = ('photons', 'scatter', 'surface', 'steps', 'steps3d')


def camera_scene(polar):
    base = scattering_slab(TARGET_RADIANCE, tables=True)
    if polar:
        return cameras(base, [0.0, 180.0], 2000.0, xpos=0.3, ypos=0.6, mpmap=1, mrproj=0, nxr=3, nyr=3, umax=180.0, vmax=180.0)
    return cameras(base, [0.0, 180.0], 2000.0, xpos=0.3, ypos=0.6, mpmap=2, mrproj=1)


def view_scene():
    grey = vref.absorbing_scene(albedo=0.3, sfc2d=True)
    sc = dataclasses.replace(vref.scattering_scene(), jsfc=grey.jsfc, psfc=grey.psfc, tmps2d=grey.tmps2d)
    return dataclasses.replace(sc, **vref._views(vref.VIEWS, 3, 2))


# name -> (scene, satellite views?, the "bwd_chunk" values the case runs under)
CASES = {
    'cam_rect':  (lambda: camera_scene(False), False, (-1,)),
    'cam_polar': (lambda: camera_scene(True), False, (-1,)),
    'views':     (view_scene, True, (0, 16)),
}


def pixel_counts(npix, id0, n):
    """how many of the ids [id0, id0 + n) map to each pixel"""
    return np.bincount((id0+np.arange(n)) % npix, minlength=npix)


def _counters(sol):
    c = sol.counters()
    return np.array([int(c[k]) for k in COUNTERS], dtype=np.int64)


def _production(sol, sc, sat, counting, weights=False, **tuning):
    """N_RUN histories through one production build: the raw image (and K_raw) through bound buffers, the counters, the capped count, the name"""
    import torch
    sol.load_scene(dataclasses.replace(sc, cam_weights=1) if weights else sc)
    npix = sc.nview*sc.nxr*sc.nyr
    img = torch.zeros(npix, dtype=torch.float64, device='cuda:0')
    K = None
    if weights:
        _, nvox, nz, nsfc = sol.weights_shape()
        K = torch.zeros(npix*(nvox+nz+nsfc), dtype=torch.float64, device='cuda:0')
    try:
        sol.set_tuning(**tuning)
        sol.set_counting(counting)
        sol.bind(img.data_ptr(), None, None, wgt_ptr=K.data_ptr() if weights else None)
        sol.reset()
        sol.run(N_RUN, seed=SEED, offset=ID0); sol.sync()
        out = dict(image=img.cpu().numpy().copy(), kernel=sol.kernel_name())
        if weights:
            out['K'] = K.cpu().numpy().reshape(npix, -1).copy()
            out['staged'] = int(sol.lib.mi3d_debug_weights_staged(sol._h))
        if counting:
            out['counters'] = _counters(sol)
        out['capped'] = (sol.debug_backward_views(SEED, 0, 0)[3] if sat else sol.debug_backward(SEED, 0, 0)[2])
    finally:
        sol.bind(None, None, None)
        sol.set_counting(False)
        sol.set_emission_weights(False)
        sol.set_tuning(wgt_stage=1, bwd_chunk=-1)
    return out


def run_case(sol, name):
    """everything the fixture of a case holds, as a flat dict of arrays (what np.savez takes)"""
    make, sat, chunks = CASES[name]
    sc = make()
    out = {}
    try:
        for chunk in chunks:
            tag = '_c%d' % chunk if sat else ''
            tune = dict(bwd_chunk=chunk) if sat else {}
            # the debug entry: every id's outputs as bytes
            sol.set_tuning(**tune)
            sol.load_scene(sc); sol.reset()
            if sat:
                st, d, score, capped = sol.debug_backward_views(SEED, ID0, N_DEBUG)
                out['start'+tag] = st.view(np.uint8).copy()
            else:
                d, score, capped = sol.debug_backward(SEED, ID0, N_DEBUG)
            out['dir'+tag] = d.view(np.uint8).copy()
            out['score'+tag] = score.view(np.uint8).copy()
            out['debug_capped'+tag] = np.int64(capped)
            # ... and what those ids do, from a counting run over them alone
            sol.set_counting(True)
            sol.load_scene(sc); sol.reset(); sol.run(N_DEBUG, seed=SEED, offset=ID0); sol.sync()
            out['debug_counters'+tag] = _counters(sol)
            sol.set_counting(False)
            # the production builds
            for c in (0, 1):
                r = _production(sol, sc, sat, bool(c), **tune)
                for k, v in r.items():
                    out['run%d%s_%s' % (c, tag, k)] = np.asarray(v)
                if not sat:
                    for stage in (1, 0):
                        r = _production(sol, sc, sat, bool(c), weights=True, wgt_stage=stage)
                        for k, v in r.items():
                            out['wgt%d_s%d_%s' % (c, stage, k)] = np.asarray(v)
    finally:
        sol.set_counting(False)
        sol.set_emission_weights(False)
        sol.set_tuning(bwd_chunk=-1, wgt_stage=1)
        sol.set_camera_method('forward')
        sol.set_view_method('forward')
    return out
