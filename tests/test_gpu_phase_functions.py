"""
The phase-function device code of er3t_amd/csrc/mi3d_device.h, point by point, against float64 numpy on the device's own float32 tables.

What every collision of every photon loop calls -- phase_eval / phase_sample (table_eval, table_sample, table_pick), their analytic
copies, and the lean kernels' lean_phase_eval / lean_phase_sample (lean_tab_find behind the 512-bucket index, stage_tables, lean_tab) --
is reached through two test hooks of the C-ABI, mi3d_debug_phase_tables and mi3d_debug_phase (include/mi3d.h): the tables as they stand
on the device, and the routines themselves on chosen points, on four paths (0 global tables, 1 LDS copy through phase_tab, 2 the lean
routines on stage_tables' copy, 3 the analytic copies).  No photon is run.  The table sets, the points, the float64 reference and the
bounds are those of tests/phase_ref.py; tests/test_phase_tables_host.py shows without a GPU that a correctly rounded float32 evaluation of
the same formulas stays inside the same bounds on the same points.

Bounds (EPS = 2^-24; interval of a point: searchsorted(side='right') - 1 on the float32 nodes, clipped to [0, nang - 2]):
  evaluation   |P - P_ref| <= 8 EPS max(p_lo, p_hi), 16 EPS max over both tables for a mixture; finite
  sampling     mu finite and inside [m_lo, m_hi] of the interval of u in the table `usel < fr` picks, exactly;
               |mu - mu_ref| <= 2 ulp32(mu_ref) + 16 EPS (mu_ref - m_lo)
  zero-width intervals of the float32 mu grid (sets A and D): finite and contained only -- a sampled cosine in [m_lo, m_hi], a value at
               the grid's end (mu >= 1 where the last nodes are equal) between the smallest and largest table value of those equal nodes
  analytic     per (function, selector): max(4 E_emul, 8 EPS), relative for P, absolute for mu, E_emul from the float32 emulation alone

Largest observed ratio to each bound on an MI355X (printed by every test below; a ratio above 1 fails):
  evaluation  path 0: 0.20   path 1: 0.20   path 2: 0.17      (0.20: set D; the float32 emulation of the lean formula reaches 0.17)
  sampling    path 0: 0.42   path 1: 0.42   path 2: 0.42      (set C, the table that is zero over a range; the emulation: 0.42)
  analytic P  path 0: 0.31   path 3: 0.31        analytic mu  path 0: 0.27   path 3: 0.27
Probes on zero-width intervals (contained and finite, no bound): 14 per table of set A and 547 in set D when sampling; 13 (set A) and
75 (set D) evaluations at mu >= 1.

Found by this module: lean_phase_eval clamped the cosine to 1 - 2^-24 before it looked the interval up AND before it took the weight, so
that P(mu = 1) was the value of the last node below 1 (er3t's grid: the node at 0.02 degrees, 5e-5 off the value at 0 degrees; a
0.25-degree grid: 2.96 of the bound).  It now clamps at 1 and the weight at 1 (mi3d_device.h).
Mutations (scratch builds, not committed): dropping `- lo * nang` from lean_tab's `op` fails 8 tests of this module; `a[lo + 1] < x` in
lean_tab_find's third probe fails it too; `a1 < x` in its first probe alone changes no result of the function -- the third probe,
`a[lo + 1] <= x`, takes the node it leaves out -- and is not detectable by any test.
"""
import numpy as np
import pytest

from tests.phase_ref import (ANALYTIC_SELECTORS, EPS, F32, SETS, analytic_bounds, analytic_points, bucket_mu, bucket_u, build_tables_np, eval_bound,
                       eval_hull, eval_ref, index_np, mu_points, pick, sample_bound, sample_ref, selectors, staged_ranges, table_set,
                       tables_touched, u_points, ulp32)
from tests.util import slab_scene

pytestmark = pytest.mark.gpu

_REF = {}        # per table set: the device's tables and the float64 reference on them, computed once
_LOADED = [None]


def load(solver, name):
    """the solver with table set `name` loaded (a one-layer slab carries it); returns the reference data of the set"""
    ang, pha = table_set(name)
    if _LOADED[0] != name:
        _LOADED[0] = None
        solver.load_scene(slab_scene(nz=1, ang=ang, pha=pha))
        _LOADED[0] = name
    mu, p, cdf, mi, ci = solver.debug_phase_tables(ang.size, pha.shape[0])
    if name in _REF:
        R = _REF[name]
        assert np.array_equal(R['mu'], mu) and np.array_equal(R['p'], p) and np.array_equal(R['cdf'], cdf)      # the same tables every time
        return R
    R = dict(mu=mu, p=p, cdf=cdf, mi=mi, ci=ci, npf=p.shape[0])
    for a in (mu, p, cdf, mi, ci):
        a.setflags(write=False)
    R['ev'] = {}
    for beyond in (False, True):
        x = mu_points(mu, beyond)
        per = []
        for t in range(R['npf']):
            ref, lo, zero = eval_ref(mu, p[t], x)
            hmin, hmax = np.full(x.size, np.nan), np.full(x.size, np.nan)
            hmin[zero], hmax[zero] = eval_hull(mu, p[t], x[zero])
            per.append((ref, eval_bound(p[t], lo), zero, hmin, hmax))
        R['ev'][beyond] = (x, per)
    R['sa'] = []
    for t in range(R['npf']):
        u = u_points(cdf[t])
        ref, lo, zero = sample_ref(mu, p[t], cdf[t], u)
        R['sa'].append((u, ref, mu[lo].astype(np.float64), mu[lo+1].astype(np.float64), sample_bound(mu, ref, lo), zero))
    _REF[name] = R
    return R


def ranges_of(path, npf):
    return staged_ranges(npf) if path in (1, 2) else [(0, 0)]


def allowed(path, apf, lo, n, npf):
    if path not in (1, 2):
        return True
    a, b = tables_touched(apf, npf)
    return lo <= a and b <= lo+n-1


@pytest.mark.parametrize('name', SETS + ('BIG',))
def test_tables_and_indices_as_the_device_holds_them(solver, name):
    ang, pha = table_set(name)
    solver.load_scene(slab_scene(nz=1, ang=ang, pha=pha)); _LOADED[0] = name
    mu, p, cdf, mi, ci = solver.debug_phase_tables(ang.size, pha.shape[0])
    _, (mu_n, p_n, cdf_n) = build_tables_np(ang, pha)
    for got, want, what in ((mu, mu_n, 'mu'), (p, p_n, 'p'), (cdf, cdf_n, 'cdf')):
        assert got.shape == want.shape and np.all(np.isfinite(got))
        d = np.abs(got.astype(np.float64)-want.astype(np.float64))
        assert np.all(d <= ulp32(want)), '%s: %d values differ from the float64 rebuild by more than one float32 ulp' % (what, int((d > ulp32(want)).sum()))
    assert mu[0] == -1.0 and mu[-1] == 1.0 and np.all(np.diff(mu) >= 0.0)
    assert np.all(cdf[:, 0] == 0.0) and np.all(cdf[:, -1] == 1.0) and np.all(np.diff(cdf, axis=1) >= 0.0)
    # the indices, from the device's own float32 values, bucket by bucket
    assert np.array_equal(mi.astype(np.int64), index_np(mu, bucket_mu))
    for t in range(pha.shape[0]):
        assert np.array_equal(ci[t].astype(np.int64), index_np(cdf[t], bucket_u)), 'CDF index of table %d' % t
    assert mi[513] == mi[512] and np.all(ci[:, 513] == ci[:, 512])


@pytest.mark.parametrize('path', [0, 1, 2])
@pytest.mark.parametrize('name', SETS)
def test_table_evaluation(solver, name, path):
    R = load(solver, name)
    npf = R['npf']
    x, per = R['ev'][path in (0, 1)]
    worst, nzero, npts = 0.0, 0, 0
    for lo, n in ranges_of(path, npf):
        apfs = sorted({float(a) for a, _ in selectors(npf) if allowed(path, a, lo, n, npf)})
        assert apfs
        P, _ = solver.debug_phase(path, np.repeat(F32(apfs), x.size), np.tile(x, len(apfs)), 0.0, lo, n)
        P = P.reshape(len(apfs), x.size).astype(np.float64)
        for k, apf in enumerate(apfs):
            i, fr, _ = pick(apf, 0.0, npf)
            ref, bound, zero, hmin, hmax = per[i]
            if fr > 0.0:
                r2, b2, z2, hmin2, hmax2 = per[i+1]
                w = float(fr)
                ref, bound = (1.0-w)*ref + w*r2, 2.0*np.maximum(bound, b2)
                hmin, hmax = (1.0-w)*hmin + w*hmin2, (1.0-w)*hmax + w*hmax2
            got = P[k]
            assert np.all(np.isfinite(got)), 'apf %g, tables %d+%d staged: %d values not finite' % (apf, lo, n, int((~np.isfinite(got)).sum()))
            ok = ~zero
            err = np.abs(got[ok]-ref[ok])
            with np.errstate(divide='ignore', invalid='ignore'):
                ratio = np.where(bound[ok] > 0.0, err/bound[ok], np.where(err == 0.0, 0.0, np.inf))      # (both nodes 0: the value is 0 exactly)
            worst = max(worst, float(ratio.max()))
            j = int(np.argmax(ratio))
            assert ratio[j] <= 1.0, 'path %d, apf %g, tables %d+%d staged: P(mu = %.9g) = %.9g, float64 %.9g, %.2f of the bound (%d points beyond it)' % (
                path, apf, lo, n, x[ok][j], got[ok][j], ref[ok][j], ratio[j], int((ratio > 1.0).sum()))
            slack = 4.0*EPS*np.abs(hmax[zero])
            inside = (got[zero] >= hmin[zero]-slack) & (got[zero] <= hmax[zero]+slack)
            assert np.all(inside), 'path %d, apf %g, tables %d+%d staged: at mu = %s (equal float32 nodes) P = %s lies outside [%s, %s]' % (
                path, apf, lo, n, x[zero][~inside][:3], got[zero][~inside][:3], hmin[zero][~inside][:3], hmax[zero][~inside][:3])
            nzero += int(zero.sum()); npts += x.size
    print('RATIO evaluation set %s path %d: %.3f of the bound over %d points (%d on equal nodes: contained)' % (name, path, worst, npts, nzero))


@pytest.mark.parametrize('path', [0, 1, 2])
@pytest.mark.parametrize('name', SETS)
def test_table_sampling(solver, name, path):
    R = load(solver, name)
    npf = R['npf']
    worst, nzero, npts = 0.0, 0, 0
    for lo, n in ranges_of(path, npf):
        sel = [(a, us) for a, us in selectors(npf) if allowed(path, a, lo, n, npf)]
        assert sel
        tabs = [pick(a, us, npf)[2] for a, us in sel]
        apf = np.concatenate([np.full(R['sa'][t][0].size, a, dtype=F32) for (a, _), t in zip(sel, tabs)])
        usel = np.concatenate([np.full(R['sa'][t][0].size, us, dtype=F32) for (_, us), t in zip(sel, tabs)])
        u = np.concatenate([R['sa'][t][0] for t in tabs])
        _, M = solver.debug_phase(path, apf, u, usel, lo, n)
        o = 0
        for (a, us), t in zip(sel, tabs):
            uu, ref, mlo, mhi, bound, zero = R['sa'][t]
            got = M[o:o+uu.size].astype(np.float64); o += uu.size
            what = 'path %d, apf %.7g, usel %.7g (table %d), tables %d+%d staged' % (path, a, us, t, lo, n)
            assert np.all(np.isfinite(got)), '%s: %d cosines not finite, first at u = %.9g' % (what, int((~np.isfinite(got)).sum()), uu[~np.isfinite(got)][0])
            inside = (got >= mlo) & (got <= mhi)
            assert np.all(inside), '%s: %d cosines outside the interval of u, first u = %.9g -> %.9g, interval [%.9g, %.9g]' % (
                what, int((~inside).sum()), uu[~inside][0], got[~inside][0], mlo[~inside][0], mhi[~inside][0])
            ok = ~zero
            ratio = np.abs(got[ok]-ref[ok])/bound[ok]
            j = int(np.argmax(ratio))
            worst = max(worst, float(ratio[j]))
            assert ratio[j] <= 1.0, '%s: mu(u = %.9g) = %.9g, float64 %.9g, %.2f of the bound (%d points beyond it)' % (
                what, uu[ok][j], got[ok][j], ref[ok][j], ratio[j], int((ratio > 1.0).sum()))
            nzero += int(zero.sum()); npts += uu.size
    print('RATIO sampling set %s path %d: %.3f of the bound over %d points (%d on zero-width intervals: contained)' % (name, path, worst, npts, nzero))


@pytest.mark.parametrize('path', [0, 3])
def test_analytic_phase_functions(solver, path):
    load(solver, 'B2')        # (path 0 with a table loaded: selectors below 1 must not look at it)
    mu, u = analytic_points()
    sel = ANALYTIC_SELECTORS
    P, _ = solver.debug_phase(path, np.repeat(F32(sel), mu.size), np.tile(mu, len(sel)))
    _, M = solver.debug_phase(path, np.repeat(F32(sel), u.size), np.tile(u, len(sel)))
    P = P.reshape(len(sel), -1).astype(np.float64); M = M.reshape(len(sel), -1).astype(np.float64)
    worst_p = worst_m = 0.0
    for k, apf in enumerate(sel):
        bp, bm, p64, m64 = analytic_bounds(apf, mu, u)
        assert np.all(np.isfinite(P[k])) and np.all(np.isfinite(M[k])) and np.all(np.abs(M[k]) <= 1.0 + 8.0*EPS)
        rp = np.abs(P[k]-p64)/p64/bp
        rm = np.abs(M[k]-m64)/bm
        worst_p = max(worst_p, float(rp.max())); worst_m = max(worst_m, float(rm.max()))
        assert rp.max() <= 1.0, 'path %d, apf %g: P(mu = %.9g) = %.9g, float64 %.9g: %.2f of the bound %.3g' % (
            path, apf, mu[np.argmax(rp)], P[k][np.argmax(rp)], p64[np.argmax(rp)], rp.max(), bp)
        assert rm.max() <= 1.0, 'path %d, apf %g: mu(u = %.9g) = %.9g, float64 %.9g: %.2f of the bound %.3g' % (
            path, apf, u[np.argmax(rm)], M[k][np.argmax(rm)], m64[np.argmax(rm)], rm.max(), bm)
    print('RATIO analytic path %d: P %.3f, mu %.3f of the bound' % (path, worst_p, worst_m))


def test_hooks_refuse_what_they_cannot_serve(solver):
    R = load(solver, 'A')
    one = F32([0.5])
    for path in (1, 2):
        for lo, n in ((1, 3), (0, 1)):
            for apf in ((1.0, 1.5) if lo == 1 else (1.5, 2.0, 7.0)):      # (7 clamps to the last table, which (0, 1) does not stage)
                with pytest.raises(OSError, match=r'code -1'):
                    solver.debug_phase(path, F32([apf]), one, 0.0, lo, n)
        for lo, n in ((3, 2), (-1, 2), (0, 0), (4, 1), (0, 5)):
            with pytest.raises(OSError, match=r'code -1'):
                solver.debug_phase(path, F32([-1.0]), one, 0.0, lo, n)
    with pytest.raises(OSError, match=r'code -1'):
        solver.debug_phase(3, F32([1.0]), one)
    with pytest.raises(OSError, match=r'code -1'):
        solver.debug_phase(4, F32([0.5]), one)
    with pytest.raises(OSError, match=r'code -1'):
        solver.debug_phase_tables(R['mu'].size+1, R['npf'])
    # tables that do not fit the LDS of a launch: the staged paths refuse, the global path serves
    ang, pha = table_set('BIG')
    load(solver, 'BIG')
    for path in (1, 2):
        for lo, n in ((0, 2), (0, 1), (1, 1)):
            with pytest.raises(OSError, match=r'code -1'):
                solver.debug_phase(path, F32([1.0+lo]), one, 0.0, lo, n)
    P, M = solver.debug_phase(0, F32([1.0, 2.0]), F32([0.5, 0.25]))
    assert np.allclose(P, 1.0, rtol=1e-6) and np.allclose(M, [0.0, -0.5], atol=1e-6)
    # a grid that does not ascend on doubles is refused by build_tables with its documented error (set D, finer than float32, is taken:
    # test_tables_and_indices_as_the_device_holds_them)
    bad = slab_scene(nz=1, ang=F32([0.0, 90.0, 90.0, 180.0]), pha=np.ones((1, 4), dtype=F32))
    _LOADED[0] = None
    with pytest.raises(OSError, match=r'ascend strictly from 0 to 180.*code -1'):
        solver.load_scene(bad)
    with pytest.raises(OSError, match=r'code -2'):
        solver.debug_phase(0, F32([1.0]), one)
    load(solver, 'B2')
