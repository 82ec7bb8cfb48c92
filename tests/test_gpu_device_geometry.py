"""
rotate_dir / sincos_turns and the surface device code of er3t_amd/csrc/mi3d_device.h (surface_R, lsrt_R, dsm_R, fresnel_unpolarised,
dsm_shadow_lambda), point by point, against float64 numpy.

Every collision of every photon loop ends in rotate_dir; every reflection off a non-Lambertian surface goes through surface_R.  Both are
reached through two test hooks of the C-ABI, mi3d_debug_rotate and mi3d_debug_surface (include/mi3d.h), which call the routines as the
photon loops inline them, one point per lane.  No photon is run and no scene is needed.  The points, the float64 references, the float32
emulations and the bounds are those of tests/geometry_ref.py; tests/test_device_geometry_host.py shows without a GPU that a correctly
rounded float32 evaluation of the same formulas stays inside half of the same bounds on the same points, and that the references agree
with the oracle's C code.

Bounds (EPS = 2^-24; h2 the squared horizontal part of the direction before the collision, st = sqrt(1 - mu^2)):
  rotation   everywhere: finite, | |new| - 1 | <= 4 EPS
             h2 >= 40 EPS: |new - ref| and |new . u - mu| <= 32 EPS + 4 EPS st / h2 + st E_SC (the frame from 1 - uz^2 mis-scales the
               perpendicular part by 2 EPS / h2: a float32 property of the formula; the factor 2 on the emulation's
               16 / 2 is for the 1-ulp rsq and the contractions)
             pole branch (|uz| = 1, or no horizontal part): |new - (st cos, st sin, mu sign uz)| <= 16 EPS + 2 sqrt(h2)
             between (the pole branch not taken, h2 < 40 EPS): finite and of unit length only -- 189715 chosen probes, none dropped
             a vertical direction one ulp short of unit length, (0, 0, +-(1 - 2^-24)), must leave the axis when st > 0
             the zero vector (0, 0, +-0) takes the pole branch as the upper pole: (st cos, st sin, +mu) within 16 EPS
  sincos     |s - sin 2 pi u|, |c - cos 2 pi u| <= E_SC = 2 x the largest error measured here, capped at 2^-16
  surfaces   per bin of a class: max(4 E_emul, 8 EPS) x the sum of the magnitudes of the terms of R at the point (E_emul: the float32
             emulation's largest scaled error in the bin; bins by max(sec), by the hot-spot distance D, by 1 + cos xi, by the facet
             exponent -- a bin of the mixture with fewer than 200 points also takes the figure of its exponent bin over the classes
             without an amplification of their own: geometry_ref._dsm_all); R finite and >= 0; reciprocity within twice the bound (the
             mixture: where the float64 formula is itself reciprocal on these float32 inputs within a hundredth of that; elsewhere no
             identity is checked, the value on the reciprocal pair is held to float64 on that pair); Lambert bit for bit; two
             calls bit-equal; Fresnel at normal incidence and at Brewster's angle

Largest ratio to each bound MEASURED on an MI355X (every test prints its own; above 1 fails; profiles/r16/device_geometry_tests.log):
  rotation  model bound: general 0.39 (cosine 0.25); rings at 0.3 / 0.1 / 0.03 / 0.01 / 3e-3 / 1.6e-3 rad: 0.08 / 0.05 / 0.04 / 0.04 / 0.13 / 0.12;
            axes 0.06 (the emulation: 0.41; 0.36 / 0.35 / 0.11 / 0.06 / 0.13 / 0.12; 0.40 -- the device's fused multiply-adds round less often)
            pole bound: poles 0.17, short 0.16, the band's 10285 points with |uz| = 1: 0.0003 (the emulation 0.83, with st's product fused 0.18)
            | |new| - 1 | <= 2.58 EPS; nothing locked; between: 189715 probes of the band and 50000 of `short`; the zero vector: 0.15
  sincos    1.2418e-07 = 2^-22.94 (the cosine of u = 0.0078061223; 200032 points): E_SC = 2.4836e-07, 2^-21.9, far below the cap of 2^-16
  lsrt      general 0.34, view_grazing 0.42, both_grazing 0.78, hotspot 0.44, near_vertical 0.16, plane_forward 0.26, plane_backward 0.37,
            clamped 0.32, guards 0.27; reciprocity 0.03 ... 0.16 of twice the bound
  dsm       general 0.32, view_grazing 0.30, both_grazing 0.39, hotspot 0.29, near_vertical 0.26, plane_forward 0.30, plane_backward 0.28,
            clamped 0.03, guards 0.36; reciprocity, on the 92254 ... 100000 points of a class where the float64 formula is reciprocal:
            0.00 ... 0.13 of twice the bound; the reciprocal pairs against float64 on those pairs: 0.03 ... 0.39 of their bound
            (points in bins of fewer than 200: 481, 5294, 4506, 186, 0, 1994, 315, 0, 6120 of 100000 a class)
  fresnel   0.25        shadow lambda 0.29

Found by this module: rotate_dir took its general branch for a direction on the axis whose uz is not exactly +-1 (den2 = 2^-23 for
uz = 1 - 2^-24): ux = uy = 0 zero every horizontal term, the photon stays on the axis whatever mu, with mu = 0 it turns round instead
of leaving sideways, and with mu = 0 and cos phi = 0 the zero vector is normalised to NaN (of 100000 such probes 89091 locked, 909 NaN).  The pole branch now also takes a direction without horizontal part (mi3d_device.h); nothing else of
rotate_dir's arithmetic changed, tests/test_gpu_walk_step.py passes on the fixtures as they were.
Mutations (scratch builds of the library from the committed source, not committed themselves; failing tests of this module as
committed, out of 28):
  `+ uy*sp` for `- uy*sp` in nx                   3 (rotation general, rings, exact)
  `uz > 0.0f` for `uz >= 0.0f` in the pole branch  1 (rotation_zero_vector; on a direction of unit length the two agree: the pole branch sees
                                                  uz = 0 for the zero vector alone, and the probes (0, 0, +-0) pin the convention there)
  the final normalisation dropped                 4 (all of rotation[...])
  `den` for `iden` in nx                          2 (rotation general, rings)
  `0.5f*kPi` for `0.25f*kPi` in kvol              10 (all nine of lsrt, surface_dispatch)
  `1.0f - cxi` in kgeo                            10 (the same)
  `mun2` for `mun2*mun2`                          8 (dsm but near_vertical and clamped, surface_dispatch)
  `rs` returned for `0.5(rs + rp)`                8 (dsm but hotspot, near_vertical and clamped; fresnel; surface_dispatch)
  the pole test back to `den2 < 1e-10f` alone     2 (rotation exact: of 100000 directions on the axis 89091 locked to it, 909 NaN; rotation_zero_vector)
  (profiles/r16/mutations.log)
"""
import numpy as np
import pytest

from tests import geometry_ref as G
from tests.geometry_ref import EPS, F32, F64

pytestmark = pytest.mark.gpu

SFC_LAMBERT, SFC_DSM, SFC_LSRT = 1, 2, 4


@pytest.mark.parametrize('group', ['general', 'rings', 'band', 'exact'])
def test_rotation(solver, group):
    names = {'general': ('general',), 'rings': tuple(n for n in G.ROT_CLASSES if n.startswith('ring')), 'band': ('band',),
             'exact': ('poles', 'axes', 'short')}[group]
    for name in names:
        d, mu, uphi = G.rotate_points(name)
        got, _ = solver.debug_rotate(d, mu, uphi)
        r = G.rotate_check(d, mu, uphi, got)
        print('RATIO rotation %-11s model %.3f (cosine %.3f) over %d points, pole %.3f over %d, between: %d probes, | |new| - 1 | %.2f EPS, locked %d' % (
            name, r['model'], r['cosine'], r['n_model'], r['pole'], r['n_pole'], r['n_between'], r['norm'], r['locked']))
        assert r['nonfinite'] == 0, '%s: %d directions not finite' % (name, r['nonfinite'])
        assert r['norm'] <= 4.0, '%s: | |new| - 1 | = %.2f EPS' % (name, r['norm'])
        i = r['worst_model']
        assert r['model'] <= 1.0, '%s: dir %s, mu %.9g, uphi %.9g -> %s: %.2f of the model bound' % (name, d[i], mu[i], uphi[i], got[i], r['model'])
        assert r['cosine'] <= 1.0, '%s: the realised scattering cosine is off by %.2f of the model bound' % (name, r['cosine'])
        i = r['worst_pole']
        assert r['pole'] <= 1.0, '%s: dir %s, mu %.9g, uphi %.9g -> %s: %.2f of the pole bound' % (name, d[i], mu[i], uphi[i], got[i], r['pole'])
        assert r['locked'] == 0, '%s: %d directions on the axis stay locked to it although st > 0' % (name, r['locked'])
        again, _ = solver.debug_rotate(d, mu, uphi)
        assert np.array_equal(got, again)


def test_rotation_zero_vector(solver):
    """no direction at all: the pole branch, read as the upper pole whatever the sign of the zero (pins `uz >= 0.0f`)"""
    d, mu, uphi, want = G.zero_vector_points()
    got, _ = solver.debug_rotate(d, mu, uphi)
    assert np.all(np.isfinite(got))
    r = np.linalg.norm(got.astype(F64) - want, axis=1)/(16.0*EPS)
    print('RATIO rotation zero vector: %.3f of the pole bound over %d points' % (r.max(), r.size))
    assert r.max() <= 1.0, 'dir %s, mu %.9g, uphi %.9g -> %s' % (d[np.argmax(r)], mu[np.argmax(r)], uphi[np.argmax(r)], got[np.argmax(r)])


def test_sincos_turns(solver):
    u = G.sincos_points()
    _, sc = solver.debug_rotate(np.tile(F32([0.0, 0.0, 1.0]), (u.size, 1)), 0.0, u)
    err = np.abs(sc.astype(F64) - G.sincos_ref(u))
    i = np.unravel_index(np.argmax(err), err.shape)
    print('MEASURED sincos_turns: largest |error| %.4e = 2^%.2f (%s of u = %.9g) over %d points; E_SC = %.4e, ratio %.3f' % (
        err.max(), np.log2(err.max()), ('sine', 'cosine')[i[1]], u[i[0]], u.size, G.E_SC, err.max()/G.E_SC))
    assert np.all(np.isfinite(sc)) and np.all(np.abs(sc) <= 1.0)
    assert G.E_SC <= G.E_SC_CAP
    assert err.max() <= G.E_SC
    # the rotation classes' own azimuths go through the same routine inside rotate_dir: the second output of the hook on them
    d, mu, uphi = G.rotate_points('general')
    _, sc2 = solver.debug_rotate(d, mu, uphi)
    assert np.abs(sc2.astype(F64) - G.sincos_ref(uphi)).max() <= G.E_SC


def _ratio(got, ref, bound):
    got = got.astype(F64)
    assert np.all(np.isfinite(got)), '%d values not finite' % int((~np.isfinite(got)).sum())
    assert np.all(got >= 0.0), '%d values negative' % int((got < 0.0).sum())
    return np.abs(got - ref)/bound


@pytest.mark.parametrize('name', G.SFC_CLASSES)
def test_lsrt(solver, name):
    C = G.lsrt_case(name)
    din, dout = C['din'], C['dout']
    rin, rout = G.reverse_pair(din, dout)
    worst = worst_rec = 0.0
    for p in C['per']:
        got = solver.debug_surface(0, SFC_LSRT, p['par'], din, dout)
        r = _ratio(got, p['ref'], p['bound'])
        i = int(np.argmax(r))
        worst = max(worst, float(r[i]))
        assert r[i] <= 1.0, 'LSRT %s %s: din %s dout %s: R = %.9g, float64 %.9g, %.2f of the bound %.3g (%d points beyond it)' % (
            name, p['par'], din[i], dout[i], got[i], p['ref'][i], r[i], p['bound'][i], int((r > 1.0).sum()))
        # reciprocity: the source and the viewer change places
        rec = solver.debug_surface(0, SFC_LSRT, p['par'], rin, rout)
        rr = np.abs(rec.astype(F64) - got.astype(F64))/(2.0*p['bound'])
        worst_rec = max(worst_rec, float(rr.max()))
        assert rr.max() <= 1.0, 'LSRT %s %s: reciprocity off by %.2f of twice the bound at din %s dout %s' % (name, p['par'], rr.max(), din[np.argmax(rr)], dout[np.argmax(rr)])
    print('RATIO lsrt %-14s %.3f of the bound, reciprocity %.3f of twice the bound, %d points x %d parameter sets' % (name, worst, worst_rec, din.shape[0], len(C['per'])))


@pytest.mark.parametrize('name', G.SFC_CLASSES)
def test_dsm(solver, name):
    C = G.dsm_case(name)
    worst = worst_rec = worst_rev = 0.0
    nstrict = nsmall = 0
    for p in C['per']:
        din, dout = C['din'][p['idx']], C['dout'][p['idx']]
        got = solver.debug_surface(0, SFC_DSM, p['par'], din, dout)
        r = _ratio(got, p['ref'], p['bound'])
        i = int(np.argmax(r))
        worst = max(worst, float(r[i]))
        assert r[i] <= 1.0, 'DSM %s %s: din %s dout %s: R = %.9g, float64 %.9g, %.2f of the bound %.3g (%d points beyond it)' % (
            name, p['par'], din[i], dout[i], got[i], p['ref'][i], r[i], p['bound'][i], int((r > 1.0).sum()))
        rin, rout = G.reverse_pair(din, dout)
        rec = solver.debug_surface(0, SFC_DSM, p['par'], rin, rout)
        # reciprocity where the float64 formula is reciprocal on these inputs: twice the bound.  Elsewhere (geometry_ref._dsm_all) the value on
        # the reciprocal pair is held to the float64 value on that pair: a direct comparison, not an identity.
        st = p['rec_strict']
        rr = np.abs(rec.astype(F64) - got.astype(F64))[st]/(2.0*p['bound'][st])
        rd = _ratio(rec, p['ref_rev'], p['bound_rev'])
        worst_rec = max(worst_rec, float(rr.max(initial=0.0))); worst_rev = max(worst_rev, float(rd.max())); nstrict += int(st.sum())
        assert rr.max(initial=0.0) <= 1.0, 'DSM %s %s: reciprocity off by %.2f of twice the bound at din %s dout %s' % (name, p['par'], rr.max(), din[st][np.argmax(rr)], dout[st][np.argmax(rr)])
        assert rd.max() <= 1.0, 'DSM %s %s: the reciprocal pair of din %s dout %s: R = %.9g, float64 %.9g, %.2f of the bound' % (
            name, p['par'], din[np.argmax(rd)], dout[np.argmax(rd)], rec[np.argmax(rd)], p['ref_rev'][np.argmax(rd)], rd.max())
        nsmall += int(p['small'].sum())
    print('RATIO dsm %-14s %.3f of the bound, reciprocity %.3f of twice the bound on %d points, the reciprocal pairs %.3f of their bound on all %d; %d points in bins below %d' % (
        name, worst, worst_rec, nstrict, worst_rev, C['din'].shape[0], nsmall, G.DSM_SMALL_BIN))


def test_fresnel(solver):
    c = G.fresnel_points()
    worst = 0.0
    for nr, ni in G.FRESNEL_INDICES:
        C = G.fresnel_case(nr, ni)
        got = solver.debug_surface(1, 0, (0.0, 0.0, nr, ni, 0.0), c)
        r = _ratio(got, C['ref'], C['bound'])
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, 'Fresnel m = %g + %gi: F(c = %.9g) = %.9g, float64 %.9g: %.2f of the bound' % (
            nr, ni, c[np.argmax(r)], got[np.argmax(r)], C['ref'][np.argmax(r)], r.max())
        assert np.all(got <= 1.0 + 4.0*EPS)
        # normal incidence: ((n - 1)^2 + k^2) / ((n + 1)^2 + k^2); Brewster's angle without absorption: the parallel part vanishes, R = rs / 2
        n, k = float(F32(nr)), float(F32(ni))
        f1 = float(solver.debug_surface(1, 0, (0.0, 0.0, nr, ni, 0.0), F32([1.0]))[0])
        assert abs(f1 - ((n - 1.0)**2 + k*k)/((n + 1.0)**2 + k*k)) <= 8.0*EPS*f1
        if ni == 0.0:
            cb = F32([np.cos(np.arctan(n))])
            fb = float(solver.debug_surface(1, 0, (0.0, 0.0, nr, ni, 0.0), cb)[0])
            rs = float(G.fresnel(nr, ni, cb, 'ref', part='s')[0])
            assert abs(fb - 0.5*rs) <= 8.0*EPS*rs, 'Brewster, n = %g: R = %.9g, rs / 2 = %.9g' % (nr, fb, 0.5*rs)
    print('RATIO fresnel %.3f of the bound over %d cosines x %d indices' % (worst, c.size, len(G.FRESNEL_INDICES)))


def test_shadow_lambda(solver):
    mu = G.lambda_points()
    worst = 0.0
    for s in G.SIGMAS:
        C = G.lambda_case(s)
        got = solver.debug_surface(2, 0, (s,), mu).astype(F64)
        assert np.all(np.isfinite(got)) and np.all(got[mu >= 1.0] == 0.0)
        r = np.abs(got - C['ref'])/C['bound']
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, 'Lambda(mu = %.9g, sigma = %g) = %.9g, float64 %.9g: %.2f of the bound' % (
            mu[np.argmax(r)], s, got[np.argmax(r)], C['ref'][np.argmax(r)], r.max())
    print('RATIO shadow lambda %.3f of the bound over %d cosines x %d slopes' % (worst, mu.size, len(G.SIGMAS)))


def test_surface_dispatch(solver):
    din, dout = G.surface_dirs('general')
    din, dout = din[:20000], dout[:20000]
    # Lambert: the albedo clamped into [0, 1], bit for bit, whatever the directions
    for a in (-0.5, 0.0, 0.3, F32(1.0) - F32(2.0**-24), 1.0, 1.5):
        got = solver.debug_surface(0, SFC_LAMBERT, (a, 0.7, 0.7, 0.7, 0.7), din, dout)
        assert np.all(got == np.clip(F32(a), F32(0.0), F32(1.0)))
    # any type code but 4 and 2 takes the Lambert branch
    for t in (0, 3, 5, 7, -1, 1 << 20):
        assert np.all(solver.debug_surface(0, t, LSRT0 + (0.0, 0.0), din, dout) == F32(LSRT0[0]))
    # types 4 and 2 take their routines, the same bits in two calls, and differ from each other and from Lambert
    l1 = solver.debug_surface(0, SFC_LSRT, LSRT0, din, dout); l2 = solver.debug_surface(0, SFC_LSRT, LSRT0, din, dout)
    d1 = solver.debug_surface(0, SFC_DSM, G.DSM_PARAMS[2], din, dout); d2 = solver.debug_surface(0, SFC_DSM, G.DSM_PARAMS[2], din, dout)
    assert np.array_equal(l1, l2) and np.array_equal(d1, d2)
    ref, _ = G.lsrt_R(LSRT0, G.lsrt_kernels(din, dout, 'ref'), 'ref')
    assert np.abs(l1 - ref).max() <= 1e-4 and np.abs(d1 - G.dsm_R(G.DSM_PARAMS[2], din, dout, 'ref')[0]).max() <= 1e-4*d1.max()
    assert (l1 != F32(LSRT0[0])).mean() > 0.99 and (d1 != l1).mean() > 0.99
    # the fourth and fifth parameter reach dsm_R: the index's imaginary part and the slope variance change the result
    assert (solver.debug_surface(0, SFC_DSM, G.DSM_PARAMS[6], din, dout) != solver.debug_surface(0, SFC_DSM, G.DSM_PARAMS[6][:3] + (0.0, 0.05), din, dout)).mean() > 0.9
    assert (solver.debug_surface(0, SFC_DSM, G.DSM_PARAMS[6], din, dout) != solver.debug_surface(0, SFC_DSM, G.DSM_PARAMS[6][:4] + (0.1,), din, dout)).mean() > 0.9


LSRT0 = G.LSRT_PARAMS[0]


def test_hooks_refuse_bad_arguments(solver):
    import ctypes as C
    lib, h = solver.lib, solver._h
    f = (C.c_float*6)(0.0, 0.0, 1.0, 0.0, 0.0, 1.0)
    fp = C.cast(f, C.POINTER(C.c_float))
    ok = lambda *a: lib.mi3d_debug_rotate(h, *a)
    assert ok(1, fp, fp, fp, fp, fp) == 0
    for args in ((0, fp, fp, fp, fp, fp), (-1, fp, fp, fp, fp, fp), ((1 << 26) + 1, fp, fp, fp, fp, fp), (1, None, fp, fp, fp, fp), (1, fp, None, fp, fp, fp),
                 (1, fp, fp, None, fp, fp), (1, fp, fp, fp, None, fp), (1, fp, fp, fp, fp, None)):
        assert ok(*args) == -1
    assert lib.mi3d_debug_rotate(None, 1, fp, fp, fp, fp, fp) < 0
    sf = lambda *a: lib.mi3d_debug_surface(h, *a)
    assert sf(0, 1, SFC_LSRT, fp, fp, fp, fp) == 0 and sf(1, 1, 0, fp, fp, None, fp) == 0 and sf(2, 1, 0, fp, fp, None, fp) == 0
    for args in ((-1, 1, 4, fp, fp, fp, fp), (3, 1, 4, fp, fp, fp, fp), (0, 0, 4, fp, fp, fp, fp), (0, (1 << 26) + 1, 4, fp, fp, fp, fp), (0, 1, 4, None, fp, fp, fp),
                 (0, 1, 4, fp, None, fp, fp), (0, 1, 4, fp, fp, None, fp), (0, 1, 4, fp, fp, fp, None), (1, 1, 4, fp, None, None, fp)):
        assert sf(*args) == -1
    assert lib.mi3d_debug_surface(None, 0, 1, 4, fp, fp, fp, fp) < 0
    with pytest.raises(OSError, match=r'code -1'):
        solver.debug_rotate(np.zeros((0, 3), dtype=F32), np.zeros(0, dtype=F32), np.zeros(0, dtype=F32))
