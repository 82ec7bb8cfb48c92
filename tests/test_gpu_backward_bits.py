"""
The histories of the backward route, bit for bit (one launch path).

k_backward, k_backward_w and k_backward_v share one body of code, launched and given their LDS by one host path.  A change to how that
body is organised or launched -- the host path that replaced the ladder of launches, or a later move of the body into a device function --
must leave every history what it was, and a compile-time switch cannot be flipped inside one library: the yardstick is what the library
of the commit BEFORE such a change computed, recorded once on the GPU into tests/golden/backward_bits/
(tools/record_backward_golden.py; the README there says how to record again).  Cases: tests/backward_bits_cases.py.

Bounds.
  The debug entries write one history's start, direction and score per slot: equal as bytes.
  Same ids and seed are the same histories: the counters of a counting run and the capped count are equal as integers.
  A raw tally is a float64 sum of non-negative terms, taken in whatever order the atomics land: two orders of m terms differ by at most
  2 m 2^-53 of the sum.  m is the number of terms that can enter the element: for a pixel of the image its count of ids in the range, for an
  element of K_raw at most the cell steps of the whole run, the fixture's own step counter.  Both are worked out here from the fixture.
"""

import os

import numpy as np
import pytest

from tests.backward_bits_cases import CASES, COUNTERS, ID0, N_DEBUG, N_RUN, pixel_counts, run_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backward_bits')
U53 = 2.0**-53
_got = {}


def both(solver, name):
    """(what this library computes for the case, computed once; the fixture)"""
    if name not in _got:
        _got[name] = run_case(solver, name)
    return _got[name], np.load(os.path.join(GOLDEN, name + '.npz'))


def tags(name):
    _, sat, chunks = CASES[name]
    return ['_c%d' % c for c in chunks] if sat else ['']


def runs(name):
    """the production runs of a case: (key prefix, COUNT, the name that serves it)"""
    _, sat, chunks = CASES[name]
    if sat:
        return [('run%d_c%d' % (c, ch), c, 'k_backward<%d,V> [thermal]' % c) for ch in chunks for c in (0, 1)]
    return [('run%d' % c, c, 'k_backward<%d> [thermal]' % c) for c in (0, 1)] + \
           [('wgt%d_s%d' % (c, s), c, 'k_backward<%d,W> [thermal]' % c) for c in (0, 1) for s in (1, 0)]


@pytest.mark.parametrize('name', list(CASES))
def test_the_fixture_does_what_the_case_is_for(name):
    want = np.load(os.path.join(GOLDEN, name + '.npz'))
    for t in tags(name):
        c = dict(zip(COUNTERS, want['debug_counters'+t].tolist()))
        score = want['score'+t].view(np.float64)
        assert c['photons'] == N_DEBUG and c['scatter'] > 0 and c['surface'] > 0 and c['steps'] > c['steps3d'] > 0, (name, t, c)
        assert int(want['debug_capped'+t]) == 0 and score.size == N_DEBUG and np.all(np.isfinite(score)) and score.min() >= 0.0 and score.max() > 0.0
        assert np.all(np.isfinite(want['dir'+t].view(np.float32)))
        if 'start'+t in want:
            assert np.all(np.isfinite(want['start'+t].view(np.float32)))
    for key, count, kernel in runs(name):
        assert str(want[key+'_kernel']) == kernel and int(want[key+'_capped']) == 0, key
        assert np.all(np.isfinite(want[key+'_image'])) and want[key+'_image'].min() >= 0.0 and want[key+'_image'].max() > 0.0, key
        if count:
            c = dict(zip(COUNTERS, want[key+'_counters'].tolist()))
            assert c['photons'] == N_RUN and c['scatter'] > 0 and c['surface'] > 0 and c['steps'] > c['steps3d'] > 0, (key, c)
        if key.startswith('wgt'):
            K = want[key+'_K']
            assert int(want[key+'_staged']) == int(key[-1]) and np.all(np.isfinite(K)) and K.min() >= 0.0 and np.all(K.sum(axis=1) > 0.0), key


@pytest.mark.parametrize('name', list(CASES))
def test_debug_entries_write_the_bytes_they_wrote(solver, name):
    got, want = both(solver, name)
    for t in tags(name):
        for what in ('start', 'dir', 'score'):
            if what+t not in want:
                assert what == 'start' and not CASES[name][1]
                continue
            a, b = got[what+t], want[what+t]
            item = 8 if what == 'score' else 12
            differ = np.unique(np.nonzero(a != b)[0]//item) if a.shape == b.shape else None
            print('%s%s %s: %d bytes, %s ids differ' % (name, t, what, b.size, 'all' if differ is None else differ.size))
            assert np.array_equal(a, b), (name, t, what, None if differ is None else differ[:8] + ID0)
        assert int(got['debug_capped'+t]) == int(want['debug_capped'+t]) == 0
        assert np.array_equal(got['debug_counters'+t], want['debug_counters'+t]), (name, t)


@pytest.mark.parametrize('name', list(CASES))
def test_production_builds_tally_the_same_histories(solver, name):
    got, want = both(solver, name)
    sc = CASES[name][0]()
    m_pix = pixel_counts(sc.nview*sc.nxr*sc.nyr, ID0, N_RUN).astype(np.float64)
    for key, count, kernel in runs(name):
        assert str(got[key+'_kernel']) == kernel, (key, got[key+'_kernel'])
        assert int(got[key+'_capped']) == int(want[key+'_capped']) == 0, key
        if count:
            for k, a, b in zip(COUNTERS, got[key+'_counters'].tolist(), want[key+'_counters'].tolist()):
                assert a == b, (key, k, a, b)
        a, b = got[key+'_image'], want[key+'_image']
        bound = 2.0*m_pix*U53*b
        print('%s %s: image: largest |new - old| / old %.3e (allowed per pixel from %.3e)' % (name, key, np.abs(a-b).max()/b.max(), 2.0*m_pix.min()*U53))
        assert a.shape == b.shape and np.all(np.abs(a-b) <= bound), (key, np.abs(a-b).max())
        if key.startswith('wgt'):
            steps = float(dict(zip(COUNTERS, want['wgt1'+key[4:]+'_counters'].tolist()))['steps'])
            a, b = got[key+'_K'], want[key+'_K']
            assert int(got[key+'_staged']) == int(want[key+'_staged']), key
            print('%s %s: K_raw: largest |new - old| %.3e of its element (allowed %.3e)' % (name, key, (np.abs(a-b)/np.where(b > 0.0, b, 1.0)).max(), 2.0*steps*U53))
            assert a.shape == b.shape and np.all(np.abs(a-b) <= 2.0*steps*U53*b), (key, np.abs(a-b).max())
