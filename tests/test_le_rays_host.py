"""
The reference, the prediction and the bounds of tests/test_gpu_le_rays.py, held on the host (tests/le_rays_ref.py):

  * the numpy Philox block equals the oracle's, bit for bit;
  * tau_ray against tau_line of tests/backward_sun_ref.py on the rays both can do (to the top, into the surface), 1e-12 relative; the
    column-bound ray against the free ray where the two are the same ray;
  * tau_ray against closed forms: a homogeneous slab (tau = beta dz / |v_z| for any start, view and sensor height), a single cloudy cell
    crossed by chosen rays of known chord lengths;
  * the prediction against the oracle: for every launch of the GPU module the oracle's raw image on the same photon ids equals the predicted
    image, contributions summed where pixels are shared, to 1e-10 relative, and is exactly 0 where the prediction is -- event points, pixels,
    contributions and the thermal launch are pinned without a GPU;
  * the drop list: at most 10 % of the arriving rays dropped, at least 1000 compared, no photon on the CDF margin, in every launch;
  * the scenes keep the issue's limits: neighbouring cells differ by 0 or by at least 1e-3 / m, cell edges of at least 100 m, every
    extinction exact in float32 whatever the order of its sum;
  * E_emul of every class (printed), and every ray's bound max(4 E_emul, (steps + 4) 2^-21) at most 1e-3 optical depths: two orders under
    the smallest one-cell mistake of these scenes (0.1).
"""

import numpy as np
import pytest

from tests import backward_sun_ref as bsun
from tests import le_rays_ref as L


def _unit(rng, n, zmin=0.05):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[:, 2] = np.where(np.abs(d[:, 2]) < zmin, zmin, d[:, 2])
    return d/np.linalg.norm(d, axis=1)[:, None]


def _points(sc, rng, n):
    return np.stack([rng.uniform(0.0, sc.nx*sc.dx, n), rng.uniform(0.0, sc.ny*sc.dy, n), rng.uniform(sc.zgrd[0], sc.zgrd[-1], n)], axis=-1)


def test_philox_block_is_the_oracles(oracle):
    for seed, ids, block in ((77, [0, 1, 5, 123456789], 0), (2**40 + 3, [2**33 + 7, 99], 1)):
        mine = L.philox(seed, ids, block)
        for row, i in zip(mine, ids):
            assert (row == oracle.philox(seed, i, block)).all()
    assert L.u01(np.uint32([0, 0xFFFFFFFF])).tolist() == [2.0**-24, 1.0 - 2.0**-24]


@pytest.mark.parametrize('variant', L.VARIANTS)
def test_tau_ray_agrees_with_tau_line(variant):
    sc = L.scene(variant)
    rng = np.random.default_rng(11)
    n = 4000
    org, d = _points(sc, rng, n), _unit(rng, n)
    d[:40] = [0.0, 0.0, 1.0]; d[40:80] = [0.0, 0.0, -1.0]                     # exactly vertical
    d[80:120, 1] = 0.0; d[80:120] /= np.linalg.norm(d[80:120], axis=1)[:, None]   # in the x-z plane
    org[120:160, 2] = 0.0; d[120:160, 2] = np.abs(d[120:160, 2])              # from the surface
    zend = np.where(d[:, 2] > 0.0, sc.zgrd[-1], sc.zgrd[0])
    tau, tend, cuts = L.tau_ray(sc, org, d, zend)
    ref, _ = bsun.tau_line(sc, org, d)
    assert np.max(np.abs(tau - ref)/np.maximum(ref, 1e-300)) <= 1e-12
    assert cuts.max() > 10 or variant == 'none_varying'
    # the column-bound ray: the free ray where that stays in its column -- vertical ones -- and in a scene one column across
    v = np.abs(d[:, 0]) + np.abs(d[:, 1]) == 0.0
    col, _, _ = L.tau_ray(sc, org, d, zend, column=True)
    assert v.sum() == 80 and np.max(np.abs(col[v] - tau[v])) <= 1e-12*tau.max()
    if variant == 'none_varying':
        assert np.max(np.abs(col - tau)) <= 1e-12*tau.max()
    else:
        assert np.max(np.abs(col - tau)) > 0.1


def test_tau_ray_in_a_homogeneous_slab():
    rng = np.random.default_rng(12)
    n = 3000
    for sc in (L.slab_scene(0.003), L.slab_scene(0.003, nz3=3)):
        beta = float(np.float32(0.003))
        org, d = _points(sc, rng, n), _unit(rng, n)
        zs = rng.uniform(-200.0, 1700.0, n)
        zs[:100] = rng.choice(sc.zgrd, 100)                                  # sensors exactly on a level
        ahead = np.where(d[:, 2] > 0.0, zs > org[:, 2], zs < org[:, 2])
        for column in (False, True):
            tau, tend, _ = L.tau_ray(sc, org, d, zs, column=column)
            want = np.where(ahead, beta*np.abs(np.clip(zs, 0.0, 1500.0) - org[:, 2])/np.abs(d[:, 2]), 0.0)
            assert np.max(np.abs(tau - want)) <= 1e-12*want.max()


def test_tau_ray_through_one_cloudy_cell():
    """the cell x 240..360, y 100..200, z 600..850 of a vacuum; chords worked out by hand"""
    sc = L.one_cell_scene()
    beta = 1.0/128.0
    rays = [((300.0, 150.0, 0.0), (0.0, 0.0, 1.0), 1500.0, 250.0),            # straight up through it
            ((300.0, 150.0, 1500.0), (0.0, 0.0, -1.0), 0.0, 250.0),           # straight down
            ((300.0, 150.0, 0.0), (0.0, 0.0, 1.0), 700.0, 100.0),             # a sensor inside the cell
            ((300.0, 150.0, 650.0), (0.0, 0.0, -1.0), 0.0, 50.0),             # from inside, downwards
            ((250.0, 150.0, 0.0), (0.6, 0.0, 0.8), 1500.0, 1062.5 - 590.0/0.6),    # once round the domain, in through the x face at 840
            ((300.0, 50.0, 600.0), (0.0, 0.6, 0.8), 1500.0, 250.0 - 250.0/3.0),    # in and out through the y faces
            ((10.0, 150.0, 600.0), (-0.8, 0.0, 0.6), 1500.0, 1250.0/3.0 - 312.5),  # backwards across the wrap, in through the face at 360
            ((590.0, 150.0, 600.0), (0.6, 0.0, 0.8), 1500.0, 0.0),            # across the wrap, past below the cell's x range in time
            ((300.0, 150.0, 600.0), (0.0, 0.0, 1.0), 600.0, 0.0),             # a sensor on the event's own level
            ((230.0, 150.0, 500.0), (0.6, 0.0, 0.8), 1500.0, 200.0/0.6 - 125.0 - 350.0/3.0)]   # from the column beside it: in through the bottom at x = 305, out through the x face at 360
    for org, d, zs, chord in rays:
        tau, _, _ = L.tau_ray(sc, [org], [d], zs)
        assert abs(tau[0] - beta*chord) <= 1e-12*beta*250.0, (org, d, zs, tau[0]/beta, chord)
    # bound to its column, the last ray starts beside the cell and never meets it; a slant one from below the cell stays inside
    assert L.tau_ray(sc, [rays[-1][0]], [rays[-1][1]], 1500.0, column=True)[0][0] == 0.0
    assert abs(L.tau_ray(sc, [rays[0][0]], [(0.6, 0.0, 0.8)], 1500.0, column=True)[0][0] - beta*250.0/0.8) <= 1e-12


@pytest.mark.parametrize('variant', L.VARIANTS)
def test_scenes_keep_their_limits(variant):
    for source in ('solar', 'thermal'):
        sc = L.scene(variant, source)
        ke = L.extinction(sc)
        assert np.array_equal(L.extinction32(sc).astype(np.float64), ke)          # exact in float32 whatever the order of the sum
        assert np.array_equal(np.round(ke/L.Q), ke/L.Q)
        for ax, cyclic in ((0, False), (1, True), (2, True)):
            d = np.abs(np.diff(ke, axis=ax, append=ke.take([0], axis=ax)) if cyclic else np.diff(ke, axis=ax))
            assert np.all((d == 0.0) | (d >= 1.0e-3)), (variant, ax)
        assert min(sc.dx, sc.dy, np.diff(sc.zgrd).min()) >= 100.0
        col = (ke*np.diff(sc.zgrd)[:, None, None]).sum(axis=0)
        assert col.max() <= 7.0 and (variant == 'none_varying' or col.max() - col.min() >= 0.7)
        assert not np.any(sc.omg1d) and not np.any(sc.omgp) and sc.le_tau1 == 0.0 and sc.le_cmin == 0.0
        want = np.zeros(sc.nz, dtype=bool)
        if variant != 'none_varying':
            k0 = sc.iz3l - 1
            want[[k0] if sc.nz3 == 1 else [k0, k0 + 1, k0 + 2] if variant == 'stacked' else [k0, k0 + 2]] = True    # (else the middle voxel layer is uniform)
        assert np.array_equal(L.walked_layers(sc), want)


@pytest.mark.parametrize('case', L.CASES, ids=L.CASE_IDS)
def test_prediction_is_the_oracles_image(case, oracle):
    sc = case.scene()
    r = L.predict(sc, case.n, case.seed, case.offset, rounded=False)
    raw, _, cnt = oracle.run_raw(sc, case.n, case.seed, case.offset)
    img = r.image()
    assert np.array_equal(raw != 0.0, img != 0.0)
    lit = img != 0.0
    rel = np.max(np.abs(raw[lit] - img[lit])/img[lit])
    print('%s: %d lit pixels, largest relative difference %.2e' % (case.name, lit.sum(), rel))
    assert lit.sum() >= 1000 and rel <= 1e-10
    counters = dict(zip(oracle.COUNTER_NAMES, (int(c) for c in cnt)))
    if case.route != 'thermal':
        assert counters['surface'] == r.n_surface
    assert counters['le_rays'] == int(r.sure.sum()) and counters['absorbed'] + counters['escaped'] + counters['killed'] == case.n


@pytest.mark.parametrize('case', L.CASES, ids=L.CASE_IDS)
def test_drop_list_and_bounds(case):
    sc, r, te, st, bound, E = L.evaluate(case)
    cmp_ = r.compared()
    by = {name: int(((r.drop & bit) != 0).sum()) for name, bit in (('fate', L.D_FATE), ('pixel edge', L.D_PIXEL), ('cdf', L.D_CDF),
                                                                   ('shared', L.D_SHARED), ('plane', L.D_PLANE), ('column face', L.D_COLUMN))}
    print('%s: %d arriving rays, %.1f %% dropped %s, %d compared, %d beyond 16.1; E_emul per view %s; largest bound %.2e'
          % (case.name, r.m, 100.0*r.dropped_share(), by, cmp_.sum(), r.dark().sum(),
             ' '.join('%d:%.1e' % (iv, e) for iv, e in sorted(E.items())), np.max(bound[cmp_])))
    assert r.dropped_share() <= 0.10 and cmp_.sum() >= 1000 and r.n_cdf == 0
    assert np.all(np.isfinite(te[cmp_])) and np.max(bound[cmp_]) <= 1.0e-3
    # every view of the launch takes part, and its rays see what it is there for
    assert set(np.unique(r.iv[cmp_])) == set(range(sc.nview))
