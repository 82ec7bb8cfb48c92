"""
The builds of the forward routes, case by case (one selector per kernel family, one launch path).

Which build of k_transport_lean, k_rays, k_transport, k_transport_flux, k_tl_runs, k_tl_scatter and k_entry serves a launch is decided on
the host.  A change to how the host reaches its builds must leave every route with the build it had, and a wrong build -- another MIX,
P3D, HEST, SRC or HEAVY -- changes the histories or the estimator.  The yardstick is what the library of the commit BEFORE such a change
computed, recorded once on the GPU into tests/golden/forward_builds/ (tools/record_forward_golden.py; the README there says how to
record again).  Cases: tests/forward_builds_cases.py.

Bounds.
  Same ids and seed are the same histories: the route's name, the form of the entry records and the first 14 counters of a counting run
  (photons ... absorbed) are equal; the sched_* and ticks_* counters depend on scheduling and are not compared.
  A raw tally is a float64 sum of non-negative terms, taken in whatever order the atomics and the record sums land: two orders of n terms
  differ by at most n 2^-53 of the sum.  n: the tally events of the case's counting run, le_column + le_rays + flux_tally of the fixture,
  more than can enter any one element.  An element that is zero in the fixture is zero.  No cross-lane partial sum of a tally compared
  here is kept in float: the one float sum of the forward routes, the lean loop's tally window (mi3d_kernel_lean.hip: wbuf), needs 64 x 64
  columns and is not reached by these scenes.
"""

import os

import numpy as np
import pytest

from tests.forward_builds_cases import CASES, COUNTERS, run_once, tallies, tally_events

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'forward_builds')
U53 = 2.0**-53


def fixture_of(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


@pytest.mark.parametrize('name', list(CASES))
def test_the_fixture_does_what_the_case_is_for(name):
    case, want = CASES[name], fixture_of(name)
    c = dict(zip(COUNTERS, want['run1_counters'].tolist()))
    for count in (0, 1):
        assert str(want['run%d_kernel' % count]) == case['want'] % count, (name, str(want['run%d_kernel' % count]))
        if case['form'] is not None:
            assert int(want['run%d_form' % count]) == case['form'], (name, count, int(want['run%d_form' % count]))
    assert c['photons'] == case['n'] and c['scatter'] > 0 and c['surface'] > 0 and c['steps'] > c['steps3d'] > 0, (name, c)
    assert tally_events(name, want['run1_counters']) > 0, (name, c)
    if '+ k_rays' in case['want']:
        assert c['le_rays'] > 0, (name, c)
    t = tallies(want)
    assert t, name
    for key, (idx, val, size) in t.items():
        assert np.all(np.isfinite(val)) and val.min() >= 0.0 and val.max() > 0.0, (name, key)
        assert idx is None or (idx.size == val.size and np.all(np.diff(idx) > 0) and idx[-1] < size and np.all(val > 0.0)), (name, key)


@pytest.mark.parametrize('name', list(CASES))
def test_counting_builds_run_the_same_histories(solver, name):
    got, want = run_once(solver, name, True), fixture_of(name)
    assert got['kernel'] == str(want['run1_kernel']), (name, got['kernel'])
    assert got['form'] == int(want['run1_form']), (name, got['form'])
    for k, a, b in zip(COUNTERS, got['counters'].tolist(), want['run1_counters'].tolist()):
        assert a == b, (name, k, a, b)


@pytest.mark.parametrize('name', list(CASES))
def test_production_builds_tally_what_they_tallied(solver, name):
    want = fixture_of(name)
    got = {'run0_'+k: v for k, v in run_once(solver, name, False).items()}
    assert str(got['run0_kernel']) == str(want['run0_kernel']), (name, got['run0_kernel'])
    assert int(got['run0_form']) == int(want['run0_form']), (name, got['run0_form'])
    n = tally_events(name, want['run1_counters'])
    tg, tw = tallies(got), tallies(want)
    assert set(tg) == set(tw), (name, sorted(tg), sorted(tw))
    for key, (ib, b, size) in tw.items():
        ia, a, size_a = tg[key]
        assert size_a == size and (ia is None) == (ib is None), (name, key)
        if ib is not None:
            assert np.array_equal(ia, ib), (name, key, 'other elements are non-zero')
        assert a.shape == b.shape, (name, key)
        rel = np.abs(a-b)/np.where(b > 0.0, b, 1.0)
        print('%s %s: %d elements, %d non-zero; largest |new - old| / old %.3e (allowed %.3e = %d x 2^-53)' % (name, key, size, int((b > 0.0).sum()), rel.max(), n*U53, n))
        assert np.all(a[b == 0.0] == 0.0), (name, key, 'an element that was zero is not')
        assert np.all(np.abs(a-b) <= n*U53*b), (name, key, rel.max())
