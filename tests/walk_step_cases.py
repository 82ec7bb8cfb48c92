"""
The cases of tests/test_gpu_walk_step.py, shared with tools/record_walk_golden.py, which records what a library computes for them.

The scene is the one of tests/test_gpu_entry_short.py -- 12 x 10 columns of 100 m, six voxel layers of 250 m with 30 % of the voxels clear,
three horizontally uniform layers above them, sun at 30 degrees, Lambert surface 0.3, nadir view -- and every case changes what its name
says: these are the smallest shapes at which a voxel step (phase A of the lean loops) can go wrong.

    nz3 = 1          every level crossing leaves the voxel layers, through the layer table's end records or into a uniform layer
    1 x 1, 2 x 1     every x / y crossing wraps, in the first onto the column it left (1 x 1: no layer varies from column to column, so the
                     layer table makes all of them uniform layers and nothing is walked; 1 x 2 wraps onto the same column AND walks)
    zenith           flight along an axis: two of the three face parameters are built on the floored |u|
    ipa, p3d         no column step at all / none for the direct beam, and the switch after the first event
    n1 .. n65        a wave with one walking lane; the walk loop's two ways out
    two3d, tables, marched, flux     the other builds: <.,.,0,1>, <.,.,0,3>, <.,.,2,0> + k_rays, k_transport_flux
"""

import numpy as np

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE, SOLVER_3D, SOLVER_P3D, SOLVER_IPA

COUNTERS = ('photons', 'scatter', 'surface', 'killed', 'escaped', 'absorbed', 'roulette', 'steps3d', 'le_rays')
SEED = 9


def walk_scene(nx=12, ny=10, nz3=6, above=3, solver=SOLVER_3D, sza=30.0, two3d=False, tables=False, slant=False, target=TARGET_RADIANCE):
    nz = nz3 + above
    rng = np.random.default_rng(11)
    zgrd = np.concatenate([250.0*np.arange(nz3+1), 250.0*nz3 + 1000.0*np.arange(1, above+1)])
    ext1d = np.full((1, nz), 2.0e-5); ext1d[0, nz3:] = 1.5e-4
    shape = (nz3, ny, nx)
    ext = (rng.uniform(2.0e-3, 2.0e-2, shape)*(rng.random(shape) < 0.7)).astype(np.float32)
    if nx*ny <= 2:
        ext[...] = rng.uniform(2.0e-3, 2.0e-2, shape).astype(np.float32)     # (no clear voxel: one or two columns would leave little to walk)
    extp, omgp, apfp = ext[None], np.full((1,)+shape, 0.97, dtype=np.float32), np.full((1,)+shape, 0.85, dtype=np.float32)
    if two3d:    # a thin second constituent in every voxel
        aer = rng.uniform(1.0e-4, 5.0e-4, shape).astype(np.float32)
        extp = np.stack([ext, aer]); omgp = np.stack([omgp[0], np.full(shape, 0.9, dtype=np.float32)])
        apfp = np.stack([apfp[0], np.full(shape, 0.6, dtype=np.float32)])
    kw = dict(zgrd=zgrd, ext1d=ext1d, omg1d=np.ones((1, nz)), apf1d=-np.ones((1, nz)), abs1d=np.zeros(nz), nx=nx, ny=ny, dx=100.0, dy=100.0,
              nz3=nz3, iz3l=1, extp=extp, omgp=omgp, apfp=apfp, sfc_mtype=1, sfc_param=[0.3, 0, 0, 0, 0], src_the=180.0-sza, src_phi=270.0,
              src_qmax=0.0, solver=solver, target=target)
    if tables:   # the cloud scatters by the second of the synthetic Henyey-Greenstein tables (selector 2)
        from er3t_amd.synth import pha_hg_synth
        pha = pha_hg_synth()
        kw.update(ang=pha.data['ang']['data'].astype(np.float32), pha=np.ascontiguousarray(pha.data['pha']['data'].T, dtype=np.float32))
        kw['apfp'] = np.where(extp > 0, np.float32(2.0), apfp).astype(np.float32)
    if target & TARGET_RADIANCE:
        the, phi = ([180.0, 140.0], [0.0, 60.0]) if slant else ([180.0], [0.0])
        kw.update(view_the=the, view_phi=phi, view_zloc=[705000.0]*len(the), nxr=nx, nyr=ny)
    return Scene(**kw)


# name -> (scene arguments, photons, what kernel_name() begins with less its COUNT argument, what it ends with)
LEAN = 'k_transport_lean<%d,'
CASES = {
    '3d':      (dict(), 4097, LEAN + '0,0,0>', ''),
    'nz3_1':   (dict(nz3=1), 4097, LEAN + '0,0,0>', ''),
    '1x1':     (dict(nx=1, ny=1), 4097, LEAN + '0,0,0>', ''),
    '2x1':     (dict(nx=2, ny=1), 4097, LEAN + '0,0,0>', ''),
    '1x2':     (dict(nx=1, ny=2), 4097, LEAN + '0,0,0>', ''),
    'zenith':  (dict(sza=0.0), 4097, LEAN + '0,0,0>', ''),
    'ipa':     (dict(solver=SOLVER_IPA), 4097, LEAN + '0,0,0>', ''),
    'p3d':     (dict(solver=SOLVER_P3D), 4097, LEAN + '1,0,0>', ''),
    'n1':      (dict(), 1, LEAN + '0,0,0>', ''),
    'n63':     (dict(), 63, LEAN + '0,0,0>', ''),
    'n64':     (dict(), 64, LEAN + '0,0,0>', ''),
    'n65':     (dict(), 65, LEAN + '0,0,0>', ''),
    'two3d':   (dict(two3d=True), 4097, LEAN + '0,0,1>', ''),
    'tables':  (dict(tables=True), 4097, LEAN + '0,0,3>', ''),
    'marched': (dict(slant=True), 4097, LEAN + '0,2,0>', '+ k_rays'),
}
FLUX_CASES = {
    'flux':    (dict(target=TARGET_FLUX), 4097, 'k_transport_flux<%d,0,0>', ''),
}


def run_case(solver, name):
    """one counting and one plain run of a case: the event counters as integers, the float32 image (or flux planes) of the plain run, and
    what kernel_name() said after either"""
    args, n, _, _ = {**CASES, **FLUX_CASES}[name]
    sc = walk_scene(**args)
    out = {}
    try:
        solver.set_tuning(tile_cols=4)
        solver.bind(None, None, None)
        for counting in (True, False):
            solver.load_scene(sc); solver.set_counting(counting); solver.reset()
            solver.run(n, seed=SEED); solver.sync()
            if counting:
                c = solver.counters()
                out['counters'] = np.array([int(c[k]) for k in COUNTERS], dtype=np.int64)
                out['kernel_counting'] = solver.kernel_name()
            else:
                out['image'] = np.asarray(solver.radiance(n) if sc.target & TARGET_RADIANCE else solver.flux(n), dtype=np.float32)
                out['kernel'] = solver.kernel_name()
    finally:
        solver.set_tuning(tile_cols=-1)
    return out
