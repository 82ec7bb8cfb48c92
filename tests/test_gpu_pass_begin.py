"""
The tally window across a pass of the lean photon loop (mi3d_kernel_lean.hip: MI3D_LEAN_C_EARLY).

Round 13 changed the order at the boundary between the voxel walk and block C: C issues its read of the layer table in front of its wait for
the record.  (Counting the pass and reading the window's origin behind the walk was tried with it and not kept: tools/experiments/
pass_begin_late.patch.)  The window's protocol must not notice a change of order there: every tally of a pass comes after that pass's read of
the origin, and a wave that holds an old origin counts a new pass before it tallies again.  What would show if it did: a tally added into a
window that is being emptied is lost or lands twice, and the image with the window differs from the image without it (mi3d_set_tuning
"tally_window" 0: every tally an atomic on the image) by whole tallies, not by rounding.

The histories themselves -- the same arithmetic on the same operands -- are held by tests/test_gpu_walk_step.py against fixtures recorded
before round 12.  Here the same photon ids run with the window on and off:

    the event counters are equal as integers (the window is no part of a history);
    the images agree to 2e-5 of the brightest pixel, the project's bound for equal histories summed in another order (float32 partial sums
    in the window and the pending register against float64 atomics: tests/test_gpu_parity.py, tests/test_gpu_walk_step.py);
    the images' float64 sums agree to 1e-6 relative: nothing lost, nothing added twice when the window moves;
    where the scene has a window the two images are NOT the same to the last bit: float32 sums in LDS round differently from float64 atomics, so
    images that are identical mean that the host gave the "on" run no window and the case compared atomics with atomics (as 48x48 does, on purpose).

Scenes: er3t_amd.synth.les_scene, nadir column view, one pixel per column.
    48x48     narrower than the window (kWin = 64 columns).  The host keeps a window only where the image is at least as wide as it
              (mi3d_api.hip: set_tally_window), so both runs of this case tally with atomics: it holds the loop's path WITHOUT a window,
              where no pass is counted and no origin read.  The cyclic edge (the second origin, worg2) is what 64x64 is for.
    64x64     the smallest image that has a window, which is as wide as the image: wherever it stands it lies across the cyclic edge in
              x and y, and both origins catch tallies.
    96x96     tile_cols = 1, which the host doubles until the tiles fit its table (4 columns, 576 tiles): the window moves hundreds of times
              per workgroup.
    130x70    not square, no multiple of the window or of the tiles.
    small     96x96 and 4100 photons, a few more than the 4096 below which a launch is not sorted and has no window: sixteen workgroups whose
              64 waves share some 68 pieces of the order, so waves find nothing, or leave after one piece, while a window is closed or being moved.
"""

import functools

import numpy as np
import pytest

from er3t_amd.synth import les_scene

pytestmark = pytest.mark.gpu

COUNTERS = ('photons', 'scatter', 'surface', 'killed', 'escaped', 'absorbed', 'roulette', 'steps3d', 'le_rays')
SEED = 13
# name -> (nx, ny, tile_cols, photons, the host gives the launch a window)
CASES = {
    '48x48':  (48, 48, 24, 1000000, False),
    '64x64':  (64, 64, -1, 1000000, True),
    '96x96':  (96, 96, 1, 1000000, True),
    '130x70': (130, 70, -1, 1000000, True),
    'small':  (96, 96, -1, 4100, True),
}


@functools.lru_cache(maxsize=None)
def scene(nx, ny):
    return les_scene(nx=nx, ny=ny, nz3=50)


def run(solver, name, window):
    """one counting and one plain run of a case: the event counters as integers and the plain run's image"""
    nx, ny, tile_cols, n, _ = CASES[name]
    sc = scene(nx, ny)
    out = {}
    try:
        solver.set_tuning(tile_cols=tile_cols, tally_window=window)
        solver.bind(None, None, None)
        for counting in (True, False):
            solver.load_scene(sc); solver.set_counting(counting); solver.reset()
            solver.run(n, seed=SEED); solver.sync()
            kname = solver.kernel_name()
            assert kname.startswith('k_transport_lean<%d,0,0,0>' % counting), kname
            if counting:
                c = solver.counters()
                out['counters'] = {k: int(c[k]) for k in COUNTERS}
            else:
                out['image'] = np.array(solver.radiance(n)[0])
    finally:
        solver.set_tuning(tile_cols=-1, tally_window=1)
    return out


_runs = {}


def run_once(solver, name, window):
    """(computed once, shared by the tests, not changed by them)"""
    if (name, window) not in _runs:
        _runs[(name, window)] = run(solver, name, window)
    return _runs[(name, window)]


def compare(tag, a, b, n):
    assert a['counters']['photons'] == n and a['counters']['killed'] + a['counters']['escaped'] + a['counters']['absorbed'] == n
    assert a['counters']['steps3d'] > 0 and a['counters']['scatter'] > 0
    for k in COUNTERS:
        assert a['counters'][k] == b['counters'][k], (tag, k, a['counters'][k], b['counters'][k])
    x, y = a['image'].astype(np.float64), b['image'].astype(np.float64)
    assert x.shape == y.shape and np.abs(y).max() > 0.0
    d, s = np.abs(x-y).max()/np.abs(y).max(), abs(x.sum()-y.sum())/abs(y.sum())
    print('%s: largest difference %.3e of the brightest pixel, sums differ by %.3e relative' % (tag, d, s))
    assert d <= 2e-5, tag
    assert s <= 1e-6, tag


@pytest.mark.parametrize('name', list(CASES))
def test_window_on_and_off_tally_the_same_image(solver, name):
    on, off = run_once(solver, name, 1), run_once(solver, name, 0)
    compare(name, on, off, CASES[name][3])
    # (the "on" run had a window exactly where the scene allows one)
    assert np.array_equal(on['image'], off['image']) == (not CASES[name][4]), name


def test_the_moving_window_gives_the_same_image_twice(solver):
    first, again = run_once(solver, '96x96', 1), run(solver, '96x96', 1)
    compare('96x96 twice', again, first, CASES['96x96'][3])
