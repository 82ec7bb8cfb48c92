"""
The rarer blocks of the lean photon loop (mi3d_kernel_lean.hip: B0, B2, B5, B6, B4, B7 -- the "full passes") on the smallest scenes
in which they carry the result: an 8 x 8 column grid of six layers, two horizontally uniform layers below, two cloudy voxel layers,
two uniform layers above, over a Lambert surface of albedo 0.5 under a sun at 30 degrees.  Every photon crosses a run of uniform
layers on its way in, most leave the voxel layers and come back, and the surface chain (B0 -> B2 -> B5 -> B6 -> B0) runs all the time.

Criteria:
  * radiance, lean loop against the oracle and against the general kernel, on the SAME photon ids in eight batches: the paired
    criterion of tests/test_gpu_fullsize.py -- the difference of the domain means within 4 standard errors of the paired difference
    + 0.03 % of the mean (float32 against float64 rounding);
  * launch sizes around the hand-out of photon ids (B4): integer counts exact; id ranges add up to the order of float32 sums --
    a pixel's sum is built from at most `le_rays` positive float32 addends (the pending register, the tally window), each addition
    rounding by at most 2^-24 of the partial sum, so two orders of summation differ by less than le_rays x 2^-24 of the pixel's
    value (9e-4 at the largest size here; one lost tally in a pixel of ~250 would show as 4e-3).
"""

import os
import re

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_RADIANCE

gpu = pytest.mark.gpu

NB, NPER = 8, 25000       # 2e5 photons in eight batches


def _chunk():
    """MI3D_CHUNK: the places of a launch's order a wave takes at a time (mi3d_kernels.hip)"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'er3t_amd', 'csrc', 'mi3d_kernels.hip')
    return int(re.search(r'^#define\s+MI3D_CHUNK\s+(\d+)', open(src).read(), re.M).group(1))


def full_pass_scene(omega=1.0, slant=False, second=False):
    nx = ny = 8
    nz, nz3, iz3l = 6, 2, 3
    rng = np.random.default_rng(7)
    zgrd = np.array([0.0, 400.0, 800.0, 1050.0, 1300.0, 2300.0, 3300.0])
    # the 1-D constituent: Rayleigh-like, thick enough that collisions inside the uniform runs (found by B0) are common
    ext1d = np.array([[2.0e-4, 2.0e-4, 1.0e-4, 1.0e-4, 1.5e-4, 1.5e-4]])
    shape = (nz3, ny, nx)
    ext = (rng.uniform(2.0e-3, 2.0e-2, shape)*(rng.random(shape) < 0.7)).astype(np.float32)      # cloudy: 30 % of the voxels clear
    extp, omgp, apfp = [ext], [np.full(shape, omega, dtype=np.float32)], [np.full(shape, 0.85, dtype=np.float32)]
    if second:
        extp.append(rng.uniform(1.0e-4, 6.0e-4, shape).astype(np.float32))
        omgp.append(np.full(shape, 0.92, dtype=np.float32)); apfp.append(np.full(shape, 0.6, dtype=np.float32))
    vza = [0.0, 40.0] if slant else [0.0]
    return Scene(zgrd=zgrd, ext1d=ext1d, omg1d=np.ones((1, nz)), apf1d=-np.ones((1, nz)), abs1d=np.zeros(nz), nx=nx, ny=ny, dx=100.0, dy=100.0,
                 nz3=nz3, iz3l=iz3l, extp=np.stack(extp), omgp=np.stack(omgp), apfp=np.stack(apfp),
                 sfc_mtype=1, sfc_param=[0.5, 0, 0, 0, 0], src_the=150.0, src_phi=270.0,
                 view_the=[180.0-v for v in vza], view_phi=[0.0, 150.0][:len(vza)], view_zloc=[705000.0]*len(vza), nxr=nx, nyr=ny,
                 target=TARGET_RADIANCE)


CASES = {'conservative': dict(), 'roulette': dict(omega=0.9), 'slant': dict(slant=True), 'second3d': dict(second=True)}
_oracle_cache = {}


def oracle_batches(oracle, name, nthreads):
    """the oracle's eight batches of a case: computed once, shared, never changed"""
    if name not in _oracle_cache:
        sc = full_pass_scene(**CASES[name])
        runs = [oracle.run(sc, NPER, seed=71, offset=b*NPER, nthreads=nthreads) for b in range(NB)]
        rad = np.stack([r['rad'] for r in runs]); rad.setflags(write=False)
        cnt = {k: sum(r['counters'][k] for r in runs) for k in runs[0]['counters']}
        _oracle_cache[name] = (rad, cnt)
    return _oracle_cache[name]


def gpu_batches(solver, sc, general=False):
    solver.bind(None, None, None)
    solver.set_kernel(general=general)
    try:
        solver.load_scene(sc)
        solver.set_counting(False)
        g = []
        for b in range(NB):
            solver.reset(); solver.run(NPER, seed=71, offset=b*NPER); solver.sync()
            g.append(solver.radiance(NPER).astype(np.float64))
        name = solver.kernel_name()
    finally:
        solver.set_kernel()
    return np.stack(g), name


def check_paired(a, b, what):
    from bench import parity_stats
    for q in parity_stats(a, b, nblk=8):
        print('%s view %d: paired %+.3e relative = %+.2f paired se' % (what, q['view'], q['paired_rel_diff'], q['paired_diff_in_paired_se']))
        assert abs(q['diff']) < 4.0*q['se_paired'] + 3.0e-4*q['mean_oracle'], (what, q)


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_runs_the_scenes(oracle, nthreads, name):
    """(no GPU) the oracle alone runs every scene of this file, and the scenes do what they are for"""
    rad, c = oracle_batches(oracle, name, nthreads)
    n = NB*NPER
    assert c['photons'] == n and c['killed']+c['escaped']+c['absorbed'] == n
    assert np.all(np.isfinite(rad)) and rad.mean() > 0.0
    assert c['surface'] > 0.3*n and c['scatter'] > 3*n            # the surface chain and the collisions are both busy
    if name == 'roulette':
        assert c['roulette'] > 0.5*n and 0 < c['roulette']-c['killed']          # most histories play, and some survive
    if name == 'slant':
        assert rad.shape[1] == 2


@gpu
@pytest.mark.parametrize('name', ['conservative', 'roulette'])
def test_lean_full_passes_follow_the_oracle_and_the_general_kernel(solver, oracle, nthreads, name):
    sc = full_pass_scene(**CASES[name])
    o, _ = oracle_batches(oracle, name, nthreads)
    g, kname = gpu_batches(solver, sc)
    assert kname.startswith('k_transport_lean<0,0,0,0>'), kname
    check_paired(g, o, name + ': lean against oracle')
    gen, gname = gpu_batches(solver, sc, general=True)
    assert gname.startswith('k_transport<'), gname
    check_paired(g, gen, name + ': lean against general')


@gpu
@pytest.mark.parametrize('name', ['slant', 'second3d'])
def test_lean_full_passes_of_the_other_builds_follow_the_oracle(solver, oracle, nthreads, name):
    """the event-writing build (a slant view beside the nadir one: MARCH 2) and the build with a second 3-D constituent (MIX 1)"""
    sc = full_pass_scene(**CASES[name])
    o, _ = oracle_batches(oracle, name, nthreads)
    g, kname = gpu_batches(solver, sc)
    assert kname.startswith({'slant': 'k_transport_lean<0,0,2,0> + k_rays', 'second3d': 'k_transport_lean<0,0,0,1>'}[name]), kname
    check_paired(g, o, name + ': lean against oracle')


@gpu
def test_launch_sizes_around_the_hand_out(solver):
    """the pool running dry, stealing across the eight pieces of the order, a window that opens, moves and is emptied by the last wave"""
    C = _chunk()
    sc = full_pass_scene()
    solver.bind(None, None, None)
    solver.load_scene(sc)
    solver.set_counting(True)
    sizes = list(dict.fromkeys([1, 63, 65, C-1, C+1, 8*C+7]))
    for n in sizes:
        solver.reset(); solver.run(n, seed=5); solver.sync()
        c = solver.counters()
        assert solver.kernel_name().startswith('k_transport_lean<1,0,0,0>'), solver.kernel_name()
        assert c['photons'] == n and c['killed']+c['escaped']+c['absorbed'] == n, (n, c)
    for n1, n2 in ((1, 63), (63, 2), (C-1, C+1), (C+1, 7*C+6), (8*C+7, 65)):
        n = n1+n2
        solver.reset(); solver.run(n, seed=5); solver.sync()
        whole = solver.radiance(n).astype(np.float64); cw = solver.counters()
        solver.reset(); solver.run(n1, seed=5, offset=0); solver.run(n2, seed=5, offset=n1); solver.sync()
        parts = solver.radiance(n).astype(np.float64); cp = solver.counters()
        for k in ('photons', 'scatter', 'surface', 'le_rays', 'roulette', 'killed', 'escaped', 'absorbed'):
            assert cw[k] == cp[k], (n1, n2, k, cw[k], cp[k])          # identical histories
        assert np.allclose(parts, whole, rtol=cw['le_rays']*2.0**-24, atol=0.0), (n1, n2, np.abs(parts/np.maximum(whole, 1e-300)-1.0).max())
