"""
The order of a voxel step (mi3d_kernel_lean.hip: MI3D_LEAN_STEP_EARLY).

Phase A of the lean photon loop works out a step's geometry -- the face crossed, the cell behind it, its face parameter, the level
crossing's read of the layer table, the next record's place -- while the record of the cell the photon is in is still on its way, and
waits for the record last.  Same operations on the same operands: every history must stay bit for bit what it was.  A compile-time switch
cannot be flipped inside one library, so the yardstick is what the library of the commit BEFORE the reorder computed, recorded once on
the GPU into tests/golden/walk_step/ (tools/record_walk_golden.py; the README there says how to record again).

Bounds.  Same ids and seed are the same histories: the event counters are equal as integers.  The images differ by the order of their
float32 partial sums only (tally window, pending register, atomics): 2e-5 of the brightest pixel, the bound tests/test_gpu_parity.py and
tests/test_gpu_entry_short.py hold equal histories summed in another order to.

Cases: tests/walk_step_cases.py.  (A grid of 1 x 1 columns has no layer that varies from column to column, and the layer table makes every
such layer a horizontally uniform one: that case takes no voxel step at all, steps3d = 0, and holds the routes around the walk.  1 x 2 is
the case in which an x crossing wraps onto the column it left AND the layers are walked.)
"""

import os

import numpy as np
import pytest

from tests.walk_step_cases import CASES, FLUX_CASES, COUNTERS, run_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'walk_step')
ALL = {**CASES, **FLUX_CASES}
WALKED = [c for c in ALL if c != '1x1']


@pytest.mark.parametrize('name', list(ALL))
def test_histories_are_what_they_were_before_the_reorder(solver, name):
    _, n, begins, ends = ALL[name]
    want = np.load(os.path.join(GOLDEN, name + '.npz'))
    got = run_case(solver, name)
    assert got['kernel_counting'].startswith(begins % 1) and got['kernel_counting'].endswith(ends), got['kernel_counting']
    assert got['kernel'].startswith(begins % 0) and got['kernel'].endswith(ends), got['kernel']
    c, w = dict(zip(COUNTERS, got['counters'].tolist())), dict(zip(COUNTERS, want['counters'].tolist()))
    print('%s: %r' % (name, c))
    # (the fixture is of this case and does what the case is for)
    assert w['photons'] == n and w['killed'] + w['escaped'] + w['absorbed'] == n
    if n > 1:
        assert (w['steps3d'] > 0) == (name in WALKED), (name, w['steps3d'])
    for k in COUNTERS:
        assert c[k] == w[k], (name, k, c[k], w[k])
    a, b = got['image'].astype(np.float64), want['image'].astype(np.float64)
    assert a.shape == b.shape and (np.abs(b).max() > 0.0 or n == 1)
    print('%s: largest difference %.3e of the brightest pixel' % (name, np.abs(a-b).max()/np.abs(b).max()))
    assert np.abs(a-b).max() <= 2e-5*np.abs(b).max(), name
