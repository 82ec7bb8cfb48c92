"""
The phase tables without a GPU: what the inputs of tests/test_gpu_phase_functions.py hold, that the reference alone keeps inside the bounds
asserted there, and what float32 tables cost against the oracle's double ones.

- The edges the GPU tests aim at exist in the shipped inputs (er3t's default grid of 498 angles, er3t_amd.synth.pha_mie_synth): a zero-width
  last interval of the float32 mu grid, a bucket of 261 nodes (lean_tab_find's bisection), 345 empty buckets; runs of equal float32 CDF nodes
  where a table is zero; 98 zero-width intervals in a grid finer than float32 resolves.  Pinned here: a change of the sets that loses an
  edge fails.
- A correctly rounded float32 emulation of lean_phase_eval / lean_table_sample, searched through a numpy restatement of build_idx and
  lean_tab_find, against the float64 reference on every probe: the search never differs from searchsorted, the value stays within 8 units
  of 2^-24 max(p_lo, p_hi) (measured: 1.34), the sampled cosine within the sampling bound (measured: 0.42 of it).  The bounds of the GPU
  tests therefore leave the device a factor of six resp. 2.4 over exact float32 arithmetic and are not met by the reference by luck.
- The float32-table model against the oracle's double tables (orc_phase_table) on the 498-angle grid: the cosine grid is quantised at
  6e-8 in the diffraction peak, which moves P by up to 1.6e-4 relative there (measured maximum 1.55e-4, table 4, at mu = 0.999947).  The
  deviation is held to 4 (|dP/dmu| ulp32(mu) + 2^-24 P): the slope bound of a cosine off by one float32 ulp, and the rounding of the table
  values themselves to float32, without which the bound is zero wherever the table is flat (the measured deviation there is 3e-8 P, all of
  it rounding of p; the slope term alone is exceeded 31-fold at mu = -0.62).  Measured: 0.22 of the bound.
- build_tables accepts a grid whose float32 cosines do not ascend strictly (it checks the ascent on doubles): pinned, with what the
  device code then has to bear (tests/test_gpu_phase_functions.py runs it).
"""
import os

import numpy as np
import pytest

from tests.phase_ref import (EPS, F32, NB, SETS, bucket_mu, bucket_u, build_tables_np, eval_emul, eval_hull, eval_ref, index_np, interval,
                             lean_tab_find_np, mu_points, sample_bound, sample_emul, sample_ref, table_set, u_points, ulp32)
from tests.util import slab_scene


def tables(name):
    ang, pha = table_set(name)
    return build_tables_np(ang, pha)


def test_the_edges_exist_in_the_inputs():
    _, (mu, p, cdf) = tables('A')
    assert mu.size == 498 and p.shape == (4, 498)
    assert np.flatnonzero(np.diff(mu) == 0.0).tolist() == [496]                      # cos 0.01 deg rounds to 1.0f
    assert mu[495] == F32(1.0 - 2.0**-24)
    per_bucket = np.bincount(bucket_mu(mu), minlength=NB)
    assert per_bucket.max() == 261 and int((per_bucket == 0).sum()) == 345
    assert max(np.bincount(bucket_u(c), minlength=NB).max() for c in cdf) == 20
    _, (mu, p, cdf) = tables('C')
    assert int((np.diff(cdf[1]) == 0.0).sum()) == 238                                # P = 0 over a range: equal float32 CDF nodes
    assert p[2].max()/p[2].min() > 0.9e9
    _, (mu, p, cdf) = tables('D')
    assert int((np.diff(mu) == 0.0).sum()) == 98
    for name in ('B2', 'B3'):
        _, (mu, p, cdf) = tables(name)
        assert mu.size == int(name[1]) and index_np(mu, bucket_mu).max() == mu.size-2     # (no entry may point at the last node)


@pytest.mark.parametrize('name', SETS)
def test_float32_emulation_stays_inside_the_caps(name):
    _, (mu, p, cdf) = tables(name)
    mi = index_np(mu, bucket_mu)
    x = mu_points(mu, False)
    lo_s = lean_tab_find_np(mu, mi, x, bucket_mu(x))                                 # (lean_phase_eval searches with the cosine clamped into [-1, 1])
    assert np.array_equal(lo_s, interval(mu, x)), 'the bucket search of mu differs from searchsorted on %d probes' % int((lo_s != interval(mu, x)).sum())
    worst_e = worst_s = 0.0
    for t in range(p.shape[0]):
        ref, lo, zero = eval_ref(mu, p[t], x)
        em = eval_emul(mu, p[t], x, lo_s).astype(np.float64)
        assert np.all(np.isfinite(em))
        ok = ~zero
        assert np.array_equal(lo_s, lo)
        scale = EPS*np.maximum(p[t][lo], p[t][lo+1]).astype(np.float64)
        err = np.abs(em-ref)[ok]
        assert np.all(err[scale[ok] == 0.0] == 0.0)
        worst_e = max(worst_e, float((err[scale[ok] > 0.0]/scale[ok][scale[ok] > 0.0]).max()))
        hmin, hmax = eval_hull(mu, p[t], x[zero])
        assert np.all((em[zero] >= hmin*(1.0-4.0*EPS)) & (em[zero] <= hmax*(1.0+4.0*EPS)))
        # sampling
        u = u_points(cdf[t])
        ci = index_np(cdf[t], bucket_u)
        lo_u = lean_tab_find_np(cdf[t], ci, u, bucket_u(u))
        mref, lo, zero = sample_ref(mu, p[t], cdf[t], u)
        assert np.array_equal(lo_u, lo), 'the bucket search of the CDF of table %d differs from searchsorted on %d probes' % (t, int((lo_u != lo).sum()))
        sm = sample_emul(mu, p[t], cdf[t], u, lo_u).astype(np.float64)
        assert np.all(np.isfinite(sm)) and np.all((sm >= mu[lo]) & (sm <= mu[lo+1]))
        ok = ~zero
        worst_s = max(worst_s, float((np.abs(sm-mref)[ok]/sample_bound(mu, mref, lo)[ok]).max()))
    print('float32 emulation, set %s: evaluation %.3f units of 2^-24 max(p), sampling %.3f of its bound' % (name, worst_e, worst_s))
    assert worst_e <= 8.0 and worst_s <= 1.0
    assert worst_e <= 1.5 and worst_s <= 0.5          # what exact float32 arithmetic reaches on these sets (1.34, 0.42): the caps have room


def test_float32_tables_against_the_oracle_double_tables(oracle):
    ang, pha = table_set('A')
    (mu64, p64, _), (mu, p, _) = tables('A')
    x = mu_points(mu, False)
    sc = slab_scene(nz=1, apf=1.0, ang=ang, pha=pha)
    worst, worst_rel = 0.0, 0.0
    for t in range(p.shape[0]):
        po, _ = oracle.phase_table(sc, t, x.astype(np.float64), np.full(x.size, 0.5))
        ref, lo, zero = eval_ref(mu, p[t], x)
        # slope of the double table where x falls in the double grid and in the two intervals next to it (a cosine off by an ulp may cross a node)
        lod = np.clip(np.searchsorted(mu64, x.astype(np.float64), side='right')-1, 0, mu64.size-2)
        sl = np.pad(np.abs(np.diff(p64[t])/np.diff(mu64)), 1, mode='edge')
        slope = np.maximum(np.maximum(sl[lod], sl[lod+1]), sl[lod+2])
        bound = 4.0*(slope*ulp32(np.maximum(np.abs(mu[lo]), np.abs(mu[lo+1]))) + EPS*po)
        ok = ~zero
        dev = np.abs(ref-po)
        worst = max(worst, float((dev[ok]/bound[ok]).max()))
        worst_rel = max(worst_rel, float((dev[ok]/po[ok]).max()))
        # at mu = 1, where the float32 grid's last nodes coincide, the double table's value lies among theirs
        hmin, hmax = eval_hull(mu, p[t], x[zero])
        assert np.all((po[zero] >= hmin*(1.0-4.0*EPS)) & (po[zero] <= hmax*(1.0+4.0*EPS)))
    print('float32 tables against double tables: %.3f of the bound, at most %.3g relative' % (worst, worst_rel))
    assert worst <= 1.0
    assert 1.0e-5 < worst_rel < 4.0e-4          # the price of float32 tables in the diffraction peak (measured 1.55e-4)


def test_build_tables_takes_a_grid_finer_than_float32():
    """build_tables (er3t_amd/csrc/mi3d_api.hip) checks that the cosines ascend on DOUBLES and casts afterwards: set D passes it, and the
    float32 grid the kernels hold has 98 zero-width intervals.  This pins the acceptance (restated rule; the GPU module loads the set
    through mi3d_set_phase + mi3d_prepare and fails if the library refuses it) and its documented refusal for a grid that does not ascend."""
    ang, pha = table_set('D')
    (mu64, _, cdf64), (mu, _, cdf) = build_tables_np(ang, pha)
    assert np.all(np.diff(mu64) > 0.0) and int((np.diff(mu) == 0.0).sum()) == 98 and np.all(np.diff(mu) >= 0.0)
    assert np.all(np.diff(cdf64) > 0.0) and np.all(np.diff(cdf) >= 0.0)
    with pytest.raises(ValueError, match='ascend strictly'):
        build_tables_np(F32([0.0, 90.0, 90.0, 180.0]), np.ones((1, 4), dtype=F32))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'er3t_amd', 'csrc', 'mi3d_api.hip')).read()
    fn = src[src.index('int build_tables('):src.index('int needs_tables(')]
    assert 'std::vector<double> mu(n)' in fn and 'if (!(mu[j] > mu[j - 1])) return fail(MI3D_EINVAL, "phase-function angles must ascend strictly from 0 to 180")' in fn
