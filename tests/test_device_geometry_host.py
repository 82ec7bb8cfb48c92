"""
Without a GPU: what tests/test_gpu_device_geometry.py rests on (tests/geometry_ref.py).

  * a correctly rounded float32 evaluation of rotate_dir stays within half of every bound of the GPU test on every one of its points; the
    surface bounds are four times the emulation's own error per bin, so the emulation stays within a quarter of them by construction --
    what is checked there is that no bin is so wide that its bound stops meaning anything;
  * the float64 references agree with the oracle's C code (orc_rotate, orc_lsrt, orc_dsm, orc_fresnel) within 1e-12;
  * the edge classes hold the edges they are named after.

One bound cannot be met at half by an emulation that rounds every operation: the pole branch's 16 EPS.  st = sqrt(1 - mu * mu) with the
product rounded on its own is off by up to 2^-25 / (2 st), 13 EPS at 1 - mu = 1.7e-4 (below that the product is exact: mu = 1 - k 2^-24
squares to 1 - k 2^-23 + k^2 2^-48, on the float32 grid while k^2 < 2^23), and the pole branch passes st on unscaled: 0.83 of the bound.
The compiler contracts 1 - mu * mu to one fused multiply-add (v_fma_f32 in the hook's kernel), which rounds once: with that one operation
fused the emulation reaches 0.18.  Both are asserted: below 1 as written, below 0.5 with st fused.  The half margin therefore rests on
that contraction: a build that rounded the product on its own would stand at up to 0.83 of the GPU test's pole bound, not at 0.17.
"""
import numpy as np
import pytest

from tests import geometry_ref as G
from tests.geometry_ref import EPS, F32, F64


@pytest.mark.parametrize('name', G.ROT_CLASSES)
def test_float32_rotation_stays_within_half_of_the_bounds(name):
    d, mu, uphi = G.rotate_points(name)
    em, sc = G.rotate_emul(d, mu, uphi)
    r = G.rotate_check(d, mu, uphi, em, e_sc=0.0)
    rf = G.rotate_check(d, mu, uphi, G.rotate_emul(d, mu, uphi, fused_st=True)[0], e_sc=0.0)
    print('EMUL rotation %-11s model %.3f (cosine %.3f) over %d, pole %.3f (st fused: %.3f) over %d, between %d, norm %.2f EPS' % (
        name, r['model'], r['cosine'], r['n_model'], r['pole'], rf['pole'], r['n_pole'], r['n_between'], r['norm']))
    assert r['nonfinite'] == 0 and r['norm'] <= 4.0 and r['locked'] == 0
    assert r['model'] <= 0.5 and r['cosine'] <= 0.5
    assert r['pole'] <= 1.0 and rf['pole'] <= 0.5 and rf['model'] <= 0.5
    assert np.abs(sc.astype(F64) - G.sincos_ref(uphi)).max() <= EPS      # (the emulation's sine and cosine: rounded once)


def test_zero_vector_takes_the_upper_pole():
    d, mu, uphi, want = G.zero_vector_points()
    assert np.all(d == 0.0) and np.signbit(d[1::2, 2]).all() and not np.signbit(d[::2, 2]).any()
    for fused, cap in ((False, 1.0), (True, 0.5)):      # (the pole bound and the unfused st: the module's docstring)
        em, _ = G.rotate_emul(d, mu, uphi, fused_st=fused)
        assert np.all(np.isfinite(em)) and np.linalg.norm(em.astype(F64) - want, axis=1).max() <= cap*16.0*EPS


def test_rotation_classes_hold_their_edges():
    n_between = n_pole = 0
    for name in G.ROT_CLASSES:
        d, mu, uphi = G.rotate_points(name)
        assert d.shape == (G.N_ROT, 3) and d.dtype == F32
        assert (d[:, 2] > 0).any() and (d[:, 2] < 0).any() or name == 'axes'
        for v in G.MU_SPECIAL:
            for w in G.UPHI_SPECIAL:
                assert ((mu == v) & (uphi == w)).sum() >= 100, (name, v, w)
        R = G.rotate_ref(d, mu, uphi)
        pole = G.pole_branch(d)
        if name == 'general' or name.startswith('ring') or name == 'axes':
            assert not pole.any() and R['h2'].min() >= G.H2_MODEL
        if name.startswith('ring'):
            assert np.allclose(np.sqrt(R['h2']), np.sin(float(name[5:])), rtol=1e-4)
        if name == 'band':
            assert R['h2'].min() > EPS and R['h2'].max() < 41.0*EPS
            n_between += int((~pole).sum()); n_pole += int(pole.sum())
            # the float32 normalisation leaves the inputs of unit length within its own rounding
            assert np.abs(np.linalg.norm(d.astype(F64), axis=1) - 1.0).max() <= 3.0*EPS
        if name == 'poles':
            assert pole.all() and np.all(R['h2'] == 0.0)
        if name == 'short':
            assert np.all(np.abs(d[:, 2]) == G.ONE_M) and np.all(R['h2'] < 1e-18)
            assert pole.sum() == 3*G.N_ROT//4 and ((d[:, 0] == 0.0) & (d[:, 1] == 0.0)).sum() == G.N_ROT//2
            assert np.all(F32(1.0) - d[:, 2]*d[:, 2] == F32(2.0**-23))      # den2 is far above the 1e-10 threshold
        if name == 'axes':
            for ax in (0, 1):
                for s in (1.0, -1.0):
                    assert (d[:, ax] == s).sum() == G.N_ROT//4
    assert n_between > 100000 and n_pole > 1000      # the band feeds both sides of the pole branch's edge
    u = G.sincos_points()
    assert u.min() > 0.0 and u.max() == G.ONE_M and u.size > 200000
    for v in (2.0**-25, 0.25, 0.5, 0.75):
        assert (u == F32(v)).any()


def test_rotation_reference_against_the_oracle(oracle):
    """the oracle's rotate_dir takes its frame from 1 - uz^2 in float64: it agrees with the reference's frame from (ux, uy) within
    a few 1e-16 / h2 (the rounding of uz^2 against 1): held per point to 1e-13 + 1e-15 / h2, and on the pole branch (exact axis) to 1e-15"""
    for name in ('general', 'ring_0.3', 'ring_0.1', 'ring_0.03', 'axes'):
        d, mu, uphi = G.rotate_points(name)
        R = G.rotate_ref(d, mu, uphi)
        got = oracle.rotate(R['u'], mu.astype(F64), 2.0*np.pi*uphi.astype(F64))
        err = np.linalg.norm(got - R['new'], axis=1)
        assert np.all(err <= 1e-13 + 1e-15/R['h2']), (name, err.max())
    d, mu, uphi = G.rotate_points('poles')
    R = G.rotate_ref(d, mu, uphi)
    got = oracle.rotate(R['u'], mu.astype(F64), 2.0*np.pi*uphi.astype(F64))
    assert np.linalg.norm(got - R['new_pole'], axis=1).max() <= 1e-15


@pytest.mark.parametrize('name', G.SFC_CLASSES)
def test_lsrt_bounds_and_reference(oracle, name):
    C = G.lsrt_case(name)
    din, dout = C['din'], C['dout']
    sub = np.arange(0, din.shape[0], 37)
    K = G.lsrt_kernels(din[sub], dout[sub], 'oracle')
    worst = 0.0
    for p in C['per']:
        assert np.all(np.isfinite(p['ref'])) and np.all(np.isfinite(p['emul'])) and np.all(p['ref'] >= 0.0) and np.all(p['emul'] >= 0.0)
        ratio = np.abs(p['emul'].astype(F64) - p['ref'])/p['bound']
        assert ratio.max() <= 0.5
        worst = max(worst, float(p['e_emul'].max()))
        ref, _ = G.lsrt_R(p['par'], K, 'oracle')
        par = [float(F32(x)) for x in p['par']]
        orc = np.array([oracle.lsrt(par[0], par[1], par[2], din[i], dout[i]) for i in sub])
        assert np.all(np.abs(ref - orc) <= 1e-12*np.maximum(np.abs(orc), 1e-300)), (name, p['par'], np.abs(ref - orc).max())
    print('EMUL lsrt %-14s %d bins, largest E_emul %.2e' % (name, np.unique(C['bins']).size, worst))
    # no bound is so wide that it stops meaning anything: outside the probes of the 1e-6 clamps a tenth of a percent of the terms (the hot spot: D2 cancels)
    assert worst <= (0.1 if name == 'clamped' else 1e-3)


@pytest.mark.parametrize('name', G.SFC_CLASSES)
def test_dsm_bounds_and_reference(oracle, name):
    C = G.dsm_case(name)
    worst = 0.0
    for p in C['per']:
        assert np.all(np.isfinite(p['ref'])) and np.all(np.isfinite(p['emul'])) and np.all(p['ref'] >= 0.0) and np.all(p['emul'] >= 0.0)
        assert (np.abs(p['emul'].astype(F64) - p['ref'])/p['bound']).max() <= 0.5
        worst = max(worst, float(p['e_emul'].max()))
        st = p['rec_strict']      # reciprocity of the emulation, as the GPU test holds it
        assert (np.abs(p['emul_rev'].astype(F64) - p['emul'].astype(F64))[st]/(2.0*p['bound'][st])).max(initial=0.0) <= 0.5
        assert (np.abs(p['emul_rev'].astype(F64) - p['ref_rev'])/p['bound_rev']).max() <= 0.5
        sub = p['idx'][::23]
        ref, _, _ = G.dsm_R(p['par'], C['din'][sub], C['dout'][sub], 'oracle')
        par = [float(F32(x)) for x in p['par']]
        orc = np.array([oracle.dsm(par, C['din'][i], C['dout'][i])[0] for i in sub])
        assert np.all(np.abs(ref - orc) <= 1e-12*np.maximum(np.abs(orc), 1e-300)), (name, p['par'], np.abs(ref - orc).max())
    print('EMUL dsm %-14s largest E_emul %.2e' % (name, worst))
    assert worst <= 3e-3      # (slope variance 1e-4: the exponent (1 - mun2) / (mun2 s2) carries the rounding of 1 - mun2 over 1e-4)


def test_fresnel_and_shadow_bounds_and_reference(oracle):
    c = G.fresnel_points()
    for nr, ni in G.FRESNEL_INDICES:
        C = G.fresnel_case(nr, ni)
        assert np.all(np.isfinite(C['emul'])) and np.all(C['emul'] >= 0.0) and np.all(C['emul'] <= 1.0 + 4.0*EPS)
        assert (np.abs(C['emul'].astype(F64) - C['ref'])/C['bound']).max() <= 0.5 and C['e_emul'].max() <= 2e-6
        sub = np.arange(0, c.size, 29)
        ref = G.fresnel(nr, ni, c[sub], 'oracle')
        orc = np.array([oracle.fresnel(float(F32(nr)), float(F32(ni)), float(x)) for x in c[sub]])
        assert np.all(np.abs(ref - orc) <= 1e-12*orc)
        # normal incidence and, without absorption, Brewster's angle: the identities the GPU test holds the device to
        n, k = float(F32(nr)), float(F32(ni))
        assert abs(G.fresnel(nr, ni, F32([1.0]), 'ref')[0] - ((n - 1.0)**2 + k*k)/((n + 1.0)**2 + k*k)) <= 1e-15
        if ni == 0.0:
            cb = np.array([np.cos(np.arctan(n))])
            assert abs(G.fresnel(nr, ni, cb, 'ref')[0] - 0.5*G.fresnel(nr, ni, cb, 'ref', part='s')[0]) <= 1e-15
    assert (c < 1e-6).sum() > 1000 and (c > 1.0).sum() >= 2
    mu = G.lambda_points()
    assert (mu >= 1.0).sum() >= 3 and (mu < 1e-5).sum() > 1000
    for s in G.SIGMAS:
        C = G.lambda_case(s)
        assert np.all(np.isfinite(C['emul'])) and np.all(C['ref'][mu >= 1.0] == 0.0) and np.all(C['emul'][mu >= 1.0] == 0.0)
        assert (np.abs(C['emul'].astype(F64) - C['ref'])/C['bound']).max() <= 0.5 and C['e_emul'].max() <= 4e-6


def test_surface_classes_hold_their_edges():
    deg = np.pi/180.0
    zen = lambda d: np.arccos(np.clip(np.abs(d[:, 2].astype(F64)), 0.0, 1.0))
    din, dout = G.surface_dirs('view_grazing')
    assert zen(dout).min() >= 79.99*deg and zen(dout).max() > 89.8*deg
    din, dout = G.surface_dirs('both_grazing')
    assert min(zen(din).min(), zen(dout).min()) >= 84.99*deg and zen(din).max() > 89.9*deg and zen(dout).max() > 89.9*deg
    din, dout = G.surface_dirs('hotspot')
    assert np.all(dout[:1000] == -din[:1000])
    ang = np.linalg.norm(dout.astype(F64) + din.astype(F64), axis=1)
    assert ang.max() <= 2.5e-3 and (ang < 1e-6).sum() > 1000 and zen(din).max() > 79.0*deg
    K = G.lsrt_kernels(din, dout, 'ref')
    for lo in (1e-7, 1e-6, 1e-5, 1e-4):
        assert ((K['D'] >= lo) & (K['D'] < 10.0*lo)).sum() > 1000
    din, dout = G.surface_dirs('near_vertical')
    assert np.all(din[:2000, :2] == 0.0) and np.all(dout[1000:3000, :2] == 0.0) and max(zen(din).max(), zen(dout).max()) <= 1.1e-3
    for name, want in (('plane_forward', -1.0), ('plane_backward', 1.0)):
        K = G.lsrt_kernels(*G.surface_dirs(name), 'ref')
        d1, d2 = G.surface_dirs(name)
        cphi = -(d1[:, 0].astype(F64)*d2[:, 0] + d1[:, 1].astype(F64)*d2[:, 1])/np.hypot(d1[:, 0], d1[:, 1])/np.hypot(d2[:, 0], d2[:, 1])
        assert np.abs(cphi - want).max() <= 1e-6
    din, dout = G.surface_dirs('clamped')
    i = np.arange(din.shape[0]) % 3
    assert np.all(din[i != 1, 2] == 0.0) and np.all(dout[i != 0, 2] == 0.0) and np.all(din[i == 1, 2] < 0.0) and np.all(dout[i == 0, 2] > 0.0)
    din, dout = G.surface_dirs('guards')
    for z in (-din[:, 2], dout[:, 2]):
        assert (z < F32(1e-6)).sum() > 10000 and (z > F32(1e-6)).sum() > 10000
    # the diffuse-specular mixture: cos chi is reached on both sides of its clamp; mu_n = (mu_i + mu_v) / |h| >= (mu_i + mu_v) / 2 cannot fall
    # below its 1e-6 guard once both cosines have passed theirs, so that guard is approached from above only
    h = dout.astype(F64) - din.astype(F64)
    hn = np.linalg.norm(h, axis=1)
    mun = h[:, 2]/hn
    cchi = -(din.astype(F64)*h).sum(axis=1)/hn
    on = (-din[:, 2] > F32(1e-6)) & (dout[:, 2] > F32(1e-6))
    assert ((mun < 1e-6) & on).sum() == 0 and ((mun > 1e-6) & (mun < 3e-6) & on).sum() > 1000
    assert ((cchi < 1e-6) & on).sum() > 100 and ((cchi > 1e-6) & (cchi < 1e-5) & on).sum() > 50, (((cchi < 1e-6) & on).sum(), ((cchi > 1e-6) & (cchi < 1e-5) & on).sum())
    assert sorted({p[4] for p in G.DSM_PARAMS}) == [1e-4, 0.003, 0.05, 0.1] and {p[1] for p in G.DSM_PARAMS} == {0.0, 0.3, 1.0}
    assert {p[3] for p in G.DSM_PARAMS} == {0.0, 1e-8, 0.3}
    # a negative total among the LSRT sets (the clamp at 0), and each weight alone
    assert sum(1 for p in G.LSRT_PARAMS if sum(1 for x in p if x != 0.0) == 1) == 3
    C = G.lsrt_case('general')
    assert (C['per'][-1]['ref'] == 0.0).sum() > 1000 and (C['per'][-1]['ref'] > 0.0).sum() > 10


def test_sincos_bound_is_capped():
    assert G.E_SC == 2.0*G.E_SC_MEASURED and G.E_SC <= G.E_SC_CAP == 2.0**-16
